// gm_host_pass2.inc -- pass 2 as a seam: gm_read_mappings (reads to mappings in one call); part of gm_host.hip.
//
// The front is gm_read_hits' (read_hits_impl, gm_host_pass1.inc).  While a sub-batch's hits are still on the device, pass2_batch runs the rule of hit_run_full_sw (ref:
// mapping.c:332-402) on them -- k_p2_items, k_sw_vector_items, k_p2_compact and k_p2_scatter, k_sw_full_batch in its by-row form over the compacted list only, k_p2_records -- then the
// rules of gm_select_pass2: score, rmapped and score_max of every hit come down (12 bytes a hit), the host's libm answers with score_full, the key and the threshold
// compare through the functions gm_select_pass2 calls, k_p2_sel_items and k_sel_pass2 leave the order of every read's final mappings, and the host adds z0 / z1 / mqv.
// Last, k_sw_text (sizing launch, host scan of the lengths, writing launch) over the hits that are mappings.  The second scores, the records and the text come down; the
// operations only on request.  Every buffer is sized by the sub-batch: a fixed number of allocations, copies and launches.  The checks are made on the host before
// anything is uploaded.

extern "C" int gm_read_mappings_size(void) { return (int)sizeof(gm_read_mappings_t); }

extern "C" void gm_read_mappings_free(gm_read_mappings_t* out) {
  if (!out) return;
  void* ptrs[] = {out->hits, out->hit_off, out->score_vector, out->recs, out->maps, out->map_off, out->cigar, out->cigar_off, out->edit, out->edit_off, out->ops};
  for (void* p : ptrs) free(p);
  memset(out, 0, sizeof *out);
}

// thresh of hit_run_full_sw: (int)abs_or_pct(sw_full_threshold, score_max), the double expression of gm_full_threshold truncated (ref: common/util.h:53, mapping.c:384)
static inline int gm_full_thresh_int(const gm_params_t& P, int score_max) { return (int)gm_full_threshold(P, score_max); }

namespace {
// the call's state across its sub-batches: the results so far, on the host
struct Pass2Call {
  gm_session_t* s = nullptr; int read_len = 0, read_words = 0, W = 0, ops_cap = 0; bool want_ops = false, want_edit = false;
  int* d_thresh_tab = nullptr;                                  // (the call's GmDevMem owns it)
  std::vector<int32_t> sv; std::vector<gm_sw_full_rec_t> recs; std::vector<gm_mapping_t> maps;
  std::vector<uint64_t> map_off, cigar_off, edit_off;           // map_off[r + 1] / cigar_off[i + 1] are appended as reads / hits are answered; [0] = 0
  std::vector<char> cigar, edit; std::vector<uint8_t> ops;
  uint64_t ops_len = 0, full_calls = 0, full_cells = 0;
};
}  // namespace

static int pass2_batch(void* ctx, const Pass1Batch& b) {
  Pass2Call& C = *(Pass2Call*)ctx;
  gm_session_t* s = C.s; const gm_params_t& P = s->P; const gm_index* ix = s->ix;
  const int n = b.n; const uint64_t nh = b.nh;
  const uint64_t maps_before = C.maps.size();
  if (nh == 0) { for (int r = 0; r < n; r++) C.map_off.push_back(maps_before); return GM_OK; }
  hipStream_t q = s->stream;
  const int read_len = C.read_len, read_words = C.read_words, W = C.W, ops_cap = C.ops_cap, N = (int)nh;
  GmDevMem mem;
  GmFullItem *d_items = nullptr, *d_work = nullptr; int *d_sv = nullptr, *d_pos = nullptr, *d_thr = nullptr; uint32_t* d_nwork = nullptr; GmFullOut* d_out = nullptr;
  gm_sw_full_rec_t* d_recs = nullptr; GmP2In* d_p2in = nullptr; uint8_t *d_ops = nullptr, *d_back = nullptr;
  GM_HIP(mem.get(&d_items, (size_t)nh * sizeof(GmFullItem))); GM_HIP(mem.get(&d_work, (size_t)nh * sizeof(GmFullItem)));
  GM_HIP(mem.get(&d_sv, (size_t)nh * 4)); GM_HIP(mem.get(&d_pos, (size_t)nh * 4)); GM_HIP(mem.get(&d_thr, (size_t)nh * 4)); GM_HIP(mem.get(&d_nwork, 4));
  GM_HIP(mem.get(&d_out, (size_t)nh * sizeof(GmFullOut))); GM_HIP(mem.get(&d_recs, (size_t)nh * sizeof(gm_sw_full_rec_t))); GM_HIP(mem.get(&d_p2in, (size_t)nh * sizeof(GmP2In)));
  // the items, the second vector score on the turned hit, the work list
  int rc = gm_launch_p2_items(N, b.d_hits, b.base, read_len, ix->d_contig_off, ix->d_contig_rna, C.d_thresh_tab, P.tiebreak_rev ? 1 : 0, ops_cap, d_items, d_thr, q); if (rc) return rc;
  rc = gm_launch_sw_vector_items(s->sc, N, d_items, ix->d_genome, b.D->d_reads, read_words, W, read_len, d_sv, q); if (rc) return rc;
  rc = gm_launch_p2_compact(N, d_items, d_thr, d_sv, d_work, d_pos, d_nwork, q); if (rc) return rc;
  uint32_t n_work = 0;
  GM_HIP(hipMemcpyAsync(&n_work, d_nwork, 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  if (n_work > nh) { gm_set_error("gm_read_mappings: %u of %llu hits in the work list", n_work, (unsigned long long)nh); return GM_E_OVERFLOW; }
  // the full alignment of the work list only, by as many waves as the back-pointer budget allows (swf_plan's rule for one class)
  if (n_work) {
    const size_t stride = ((size_t)W * (size_t)read_len + 256 + 15) & ~(size_t)15;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min<uint32_t>(n_work, (uint32_t)GM_SWF_MAX_GRID), GM_SWF_BACK_BUDGET / stride));
    GM_HIP(mem.get(&d_back, (size_t)grid * stride)); GM_HIP(mem.get(&d_ops, (size_t)n_work * (size_t)ops_cap + 16));
    rc = gm_launch_sw_full_batch(s->sc, 0, (int)n_work, grid, d_work, ix->d_genome, b.D->d_reads, read_words, W, read_len, d_back, stride, d_out, d_ops, P.local_alignment ? 1 : 0, q, 1, 1);
    if (rc) return rc;
  }
  rc = gm_launch_p2_records(N, b.d_hits, d_pos, d_out, ops_cap, d_recs, d_p2in, q); if (rc) return rc;
  std::vector<GmP2In> p2in((size_t)nh);
  GM_HIP(hipMemcpyAsync(p2in.data(), d_p2in, (size_t)nh * sizeof(GmP2In), hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  // hit_run_post_sw per hit, letter space (ref: mapping.c:1609-1625), and the threshold compare: the functions gm_select_pass2 calls
  const bool mqv_on = gm_mqv_on(P);
  const double al = s->score_alpha, be = s->score_beta;
  std::vector<GmP2Host> ans((size_t)nh); std::vector<double> posterior((size_t)nh, 0.0);
  for (uint64_t i = 0; i < nh; i++) {
    const GmP2In& in = p2in[i];
    if (in.score_max < 1) { gm_set_error("gm_read_mappings: hit %llu: score_max %d", (unsigned long long)(b.hits_before + i), in.score_max); return GM_E_ARG; }
    int sf = in.score;
    if (sf > 0 && mqv_on) { posterior[i] = gm_ls_posterior(al, be, in.score, in.rmapped); int ps = gm_post_score(al, be, posterior[i], in.rmapped); if (ps < 0) ps = 0; sf = ps; }
    const int pct = (1000 * 100 * sf) / in.score_max;                    // ref: mapping.c:400-401
    ans[i].score_full = sf; ans[i].key = P.sw_full_threshold < 0 ? sf : pct;
    ans[i].keep = (double)sf >= gm_full_threshold(P, in.score_max) ? 1 : 0;      // ref: mapping.c:1661 (double compare)
  }
  GmP2Host* d_ans = nullptr; GmSel2Item* d_sel = nullptr; unsigned long long* d_hoff = nullptr; int32_t* d_order = nullptr; uint32_t* d_cnt = nullptr;
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "offsets are copied as they are");
  GM_HIP(mem.up(&d_ans, ans.data(), (size_t)nh, q)); GM_HIP(mem.up(&d_hoff, b.hit_off, (size_t)n + 1, q));
  GM_HIP(mem.get(&d_sel, (size_t)nh * sizeof(GmSel2Item))); GM_HIP(mem.get(&d_order, (size_t)nh * 4)); GM_HIP(mem.get(&d_cnt, (size_t)n * 4));
  rc = gm_launch_p2_sel_items(N, b.d_hits, d_recs, d_ans, d_sel, q); if (rc) return rc;
  rc = gm_launch_sel_pass2(n, P.num_outputs, P.strata ? 1 : 0, P.max_alignments, d_hoff, d_sel, d_order, d_cnt, q); if (rc) return rc;
  std::vector<int32_t> order((size_t)nh); std::vector<uint32_t> cnt((size_t)n);
  const size_t h0 = C.recs.size();                                       // == b.hits_before
  C.recs.resize(h0 + (size_t)nh); C.sv.resize(h0 + (size_t)nh);
  GM_HIP(hipMemcpyAsync(order.data(), d_order, (size_t)nh * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipMemcpyAsync(C.recs.data() + h0, d_recs, (size_t)nh * sizeof(gm_sw_full_rec_t), hipMemcpyDeviceToHost, q));
  GM_HIP(hipMemcpyAsync(C.sv.data() + h0, d_sv, (size_t)nh * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  // the mappings in the reference's output order, z0 / z1 / mqv (compute_unpaired_mqv, ref: output.c:777-793,975-984): as gm_select_pass2 makes them
  for (int r = 0; r < n; r++) {
    const uint64_t base = b.hit_off[r]; const uint64_t have = b.hit_off[r + 1] - base; const int m = (int)cnt[r];
    if ((uint64_t)m > have) { gm_set_error("gm_read_mappings: read %d: %d mappings of %llu hits", b.base + r, m, (unsigned long long)have); return GM_E_OVERFLOW; }
    const size_t first = C.maps.size();
    for (int k = 0; k < m; k++) {
      const int32_t ord = order[base + k];
      if (ord < 0 || (uint64_t)ord >= have) { gm_set_error("gm_read_mappings: read %d: mapping %d names hit %d of %llu", b.base + r, k, ord, (unsigned long long)have); return GM_E_OVERFLOW; }
      const uint64_t i = base + (uint64_t)ord;
      gm_mapping_t o; o.read = b.base + r; o.hit = (int32_t)(b.hits_before + i); o.score_full = ans[i].score_full; o.pct_score_full = (1000 * 100 * ans[i].score_full) / p2in[i].score_max;
      o.mqv = 255; o.flags = 0; o.posterior = posterior[i]; o.z0 = o.z1 = 0;
      C.maps.push_back(o);
    }
    if (m && mqv_on) {
      double z1 = 0.0;
      for (size_t k = first; k < C.maps.size(); k++) z1 += C.maps[k].posterior;
      for (size_t k = first; k < C.maps.size(); k++) { gm_mapping_t& o = C.maps[k]; o.z0 = o.posterior; o.z1 = z1; o.mqv = gm_unpaired_mqv(o.posterior, z1); }
      if (P.single_best_mapping) {                                       // the first mapping with the highest quality
        size_t mx = first;
        for (size_t k = first + 1; k < C.maps.size(); k++) if (C.maps[k].mqv > C.maps[mx].mqv) mx = k;
        C.maps[first] = C.maps[mx]; C.maps.resize(first + 1);
      }
    } else for (size_t k = first; k < C.maps.size(); k++) C.maps[k].posterior = 0;
    C.map_off.push_back(C.maps.size());
  }
  // the text of the hits that are mappings, in hit order; tail: the read positions behind the alignment (letter space: rmapped is the alignment's read positions)
  std::vector<uint8_t> mapped((size_t)nh, 0);
  for (size_t k = maps_before; k < C.maps.size(); k++) mapped[(size_t)((uint64_t)C.maps[k].hit - b.hits_before)] = 1;
  std::vector<GmTextItem> titems; std::vector<uint32_t> towner;
  for (uint64_t i = 0; i < nh; i++) {
    if (!mapped[i]) continue;
    const gm_pass1_hit_t& h = b.h_hits[i]; const gm_sw_full_rec_t& R = C.recs[h0 + i];
    const long long clen = (long long)ix->contig_off[h.cn + 1] - (long long)ix->contig_off[h.cn];
    if (R.score <= 0 || (uint64_t)R.n_ops > (uint64_t)ops_cap || R.genome_start < 0 || R.read_start < 0 || R.read_start + R.rmapped > read_len || R.genome_start + R.gmapped > clen) {
      gm_set_error("gm_read_mappings: hit %llu: a mapping whose record lies outside its window", (unsigned long long)(b.hits_before + i)); return GM_E_OVERFLOW; }
    GmTextItem it; memset(&it, 0, sizeof it);
    it.ops_off = R.ops_off; it.n_ops = R.n_ops; it.genome_start = R.genome_start; it.read_start = R.read_start; it.tail = read_len - R.read_start - R.rmapped;
    it.idx = h.read - b.base;                                            // the row of the sub-batch's reads
    it.gbase = (long long)ix->contig_off[h.cn] + (h.gen_st ? clen - 1 : 0);
    it.flags = (h.gen_st ? 1 | 4 : 0) | ((ix->rna_ready && ix->contig_rna[h.cn]) ? 2 : 0);      // strand 1 of the contig, printed as a reverse-strand mapping
    titems.push_back(it); towner.push_back((uint32_t)i);
  }
  const size_t m = titems.size();
  const int what = GM_TEXT_CIGAR | (C.want_edit ? GM_TEXT_EDIT : 0);
  std::vector<uint32_t> lens(m * 2, 0); std::vector<unsigned long long> offs(m * 2, 0);
  uint64_t cig_total = 0, edit_total = 0;
  const size_t cig0 = C.cigar.size(), ed0 = C.edit.size();
  if (m) {
    GmTextItem* d_ti = nullptr; uint32_t* d_lens = nullptr; unsigned long long* d_offs = nullptr; uint8_t *d_cig = nullptr, *d_ed = nullptr;
    GM_HIP(mem.up(&d_ti, titems.data(), m, q)); GM_HIP(mem.get(&d_lens, m * 2 * sizeof(uint32_t))); GM_HIP(mem.get(&d_offs, m * 2 * sizeof(unsigned long long)));
    rc = gm_launch_sw_text((int)m, d_ti, 0, what, 0, d_ops, ix->d_genome, b.D->d_reads, read_words, 0, nullptr, 'S', d_lens, d_offs, nullptr, nullptr, nullptr, nullptr, q, 1);
    if (rc != GM_OK) { gm_set_error("gm_read_mappings: the text kernel's launch failed"); return rc; }
    GM_HIP(hipMemcpyAsync(lens.data(), d_lens, m * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    for (size_t k = 0; k < m; k++) { offs[2 * k] = cig_total; offs[2 * k + 1] = edit_total; cig_total += lens[2 * k]; edit_total += lens[2 * k + 1]; }
    GM_HIP(hipMemcpyAsync(d_offs, offs.data(), m * 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, q));
    GM_HIP(mem.get(&d_cig, (size_t)cig_total + 16));
    if (C.want_edit) GM_HIP(mem.get(&d_ed, (size_t)edit_total + 16));
    rc = gm_launch_sw_text((int)m, d_ti, 0, what, 1, d_ops, ix->d_genome, b.D->d_reads, read_words, 0, nullptr, 'S', d_lens, d_offs, nullptr, nullptr, d_cig, d_ed, q, 1);
    if (rc != GM_OK) { gm_set_error("gm_read_mappings: the text kernel's launch failed"); return rc; }
    C.cigar.resize(cig0 + (size_t)cig_total); C.edit.resize(ed0 + (size_t)edit_total);
    if (cig_total) GM_HIP(hipMemcpyAsync(C.cigar.data() + cig0, d_cig, (size_t)cig_total, hipMemcpyDeviceToHost, q));
    if (C.want_edit && edit_total) GM_HIP(hipMemcpyAsync(C.edit.data() + ed0, d_ed, (size_t)edit_total, hipMemcpyDeviceToHost, q));
  }
  std::vector<uint8_t> loose;
  if (C.want_ops && n_work) { loose.resize((size_t)n_work * (size_t)ops_cap); GM_HIP(hipMemcpyAsync(loose.data(), d_ops, loose.size(), hipMemcpyDeviceToHost, q)); }
  GM_HIP(hipStreamSynchronize(q));
  // n_hits + 1 offsets: a hit that is no mapping has an empty slice
  {
    size_t k = 0; uint64_t c = cig0, e = ed0;
    for (uint64_t i = 0; i < nh; i++) {
      if (k < m && towner[k] == (uint32_t)i) { c += lens[2 * k]; e += lens[2 * k + 1]; k++; }
      C.cigar_off.push_back(c); if (C.want_edit) C.edit_off.push_back(e);
    }
  }
  // the operations, compacted in hit order: the records point into that buffer whether or not it comes down
  for (uint64_t i = 0; i < nh; i++) {
    gm_sw_full_rec_t& R = C.recs[h0 + i];
    const uint64_t dev_off = R.ops_off;
    R.ops_off = C.ops_len;
    if (R.n_ops) {
      if (C.want_ops) C.ops.insert(C.ops.end(), loose.begin() + (size_t)dev_off, loose.begin() + (size_t)dev_off + R.n_ops);
      C.ops_len += R.n_ops;
    }
    if (C.sv[h0 + i] >= gm_full_thresh_int(P, b.h_hits[i].score_max)) { C.full_calls++; C.full_cells += (uint64_t)b.h_hits[i].w_len * (uint64_t)read_len; }
  }
  return GM_OK;
}

// a result array of the C heap from a vector (null when empty); false: out of memory
template <class T, class U> static bool pass2_give(const std::vector<T>& v, U** out) {
  *out = nullptr;
  if (v.empty()) return true;
  void* p = malloc(v.size() * sizeof(T));
  if (!p) return false;
  memcpy(p, v.data(), v.size() * sizeof(T)); *out = (U*)p;
  return true;
}

extern "C" int gm_read_mappings(gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const uint8_t* initbp, int want_ops, gm_read_mappings_t* out,
                                gm_map_stats_t* stats) {
  if (!s || !out) { gm_set_error("gm_read_mappings: bad arguments (the session and the result struct are required)"); return GM_E_ARG; }
  memset(out, 0, sizeof *out);
  if (stats) memset(stats, 0, sizeof *stats);
  if (s->P.colour_space) {
    gm_set_error("gm_read_mappings: a colour-space session: pass 2 there needs post_sw and its host re-dos between the full alignment and the selection -- use the chain of "
                 "seams (gm_read_hits, gm_sw_full_cs_batch_ix, gm_post_sw_batch_ix, gm_select_pass2, gm_sw_full_batch_text_ix)");
    return GM_E_ARG;
  }
  Pass2Call C; C.s = s; C.want_ops = want_ops != 0; C.want_edit = s->P.extra_sam_fields != 0;
  C.map_off.push_back(0); C.cigar_off.push_back(0); if (C.want_edit) C.edit_off.push_back(0);
  const int nr = std::max(n_reads, 0);
  std::vector<uint64_t> hit_off((size_t)nr + 1, 0);
  gm_pass1_hit_t* hits = nullptr; uint64_t n_hits = 0;
  struct HitsGuard { gm_pass1_hit_t*& p; ~HitsGuard() { free(p); } } guard{hits};
  if (n_reads > 0) {
    if (int rc = pass1_reads_check("gm_read_mappings", s, n_reads, read_len, reads_packed, initbp)) return rc;
    if (int rc = pass1_k_check("gm_read_mappings", s)) return rc;
    const int W = window_len_of(s->P, read_len);
    if (gm_score_windows_lds(0, read_len, W) > GM_SCORE_WIN_LDS_LIMIT) { gm_set_error("gm_read_mappings: windows of %d positions beside reads of %d are beyond the scoring kernel's LDS", W, read_len); return GM_E_RANGE; }
    if (gm_sw_full_batch_lds(W, read_len) > GM_SWF_LDS_LIMIT) { gm_set_error("gm_read_mappings: windows of %d positions beside reads of %d are beyond the full-alignment kernel's LDS", W, read_len); return GM_E_RANGE; }
    C.read_len = read_len; C.read_words = (read_len + 7) / 8; C.W = W; C.ops_cap = W + read_len + 8;
    // thresh per possible score_max = min(read_len, w_len) * match, in the host's own double expression
    std::vector<int> tab((size_t)read_len + 1);
    for (int m = 0; m <= read_len; m++) tab[m] = gm_full_thresh_int(s->P, m * s->P.match_score);
    GmDevMem mem;
    {
      GmDevTurn dev_turn(s);
      GM_HIP(hipSetDevice(s->ix->device));
      GM_HIP(mem.up(&C.d_thresh_tab, tab.data(), tab.size(), gm_sync));
    }
    const int rc = read_hits_impl("gm_read_mappings", s, n_reads, read_len, reads_packed, initbp, &hits, &n_hits, hit_off.data(), nullptr, nullptr, nullptr, nullptr, stats, pass2_batch, &C);
    if (rc) { if (stats) memset(stats, 0, sizeof *stats); return rc; }
    if (C.recs.size() != n_hits || C.map_off.size() != (size_t)n_reads + 1 || C.cigar_off.size() != (size_t)n_hits + 1) {
      gm_set_error("gm_read_mappings: %zu records of %llu hits, %zu map offsets of %d reads", C.recs.size(), (unsigned long long)n_hits, C.map_off.size(), n_reads); return GM_E_OVERFLOW; }
  }
  gm_read_mappings_t R; memset(&R, 0, sizeof R);
  R.n_reads = nr; R.has_edit = C.want_edit ? 1 : 0; R.n_hits = n_hits; R.n_maps = C.maps.size(); R.cigar_len = C.cigar.size(); R.edit_len = C.edit.size(); R.ops_len = C.ops_len;
  const bool ok = pass2_give(hit_off, &R.hit_off) && pass2_give(C.sv, &R.score_vector) && pass2_give(C.recs, &R.recs) && pass2_give(C.maps, &R.maps) &&
                  pass2_give(C.map_off, &R.map_off) && pass2_give(C.cigar, &R.cigar) && pass2_give(C.cigar_off, &R.cigar_off) && pass2_give(C.edit, &R.edit) &&
                  pass2_give(C.edit_off, &R.edit_off) && pass2_give(C.ops, &R.ops);
  if (!ok) { gm_read_mappings_free(&R); gm_set_error("gm_read_mappings: out of memory at %llu hits", (unsigned long long)n_hits); return GM_E_NOMEM; }
  R.hits = hits; hits = nullptr;
  if (stats) { stats->full_calls = C.full_calls; stats->full_cells = C.full_cells; }
  *out = R;
  return GM_OK;
}
