// gm_host_pass2.inc -- pass 2 as a seam: gm_read_mappings (reads to mappings in one call); part of gm_host.hip.
//
// The front is gm_read_hits' (read_hits_impl, gm_host_pass1.inc).  While a sub-batch's hits are still on the device, pass2_batch runs the rule of hit_run_full_sw (ref:
// mapping.c:332-402) on them -- k_p2_items, k_sw_vector_items, k_p2_compact and k_p2_scatter, k_sw_full_batch in its by-row form over the compacted list only, k_p2_records -- then the
// rules of gm_select_pass2: score, rmapped and score_max of every hit come down (12 bytes a hit), the host's libm answers with score_full, the key and the threshold
// compare through the functions gm_select_pass2 calls, k_p2_sel_items and k_sel_pass2 leave the order of every read's final mappings, and the host adds z0 / z1 / mqv.
// Last, k_sw_text (sizing launch, host scan of the lengths, writing launch) over the hits that are mappings.  The second scores, the records and the text come down; the
// operations only on request.  Every buffer is sized by the sub-batch: a fixed number of allocations, copies and launches.  The checks are made on the host before
// anything is uploaded.
// The stages behind the records -- the selection with the mapping loop (pass2_select), the text of the mappings (pass2_text), the compaction of the operations
// (pass2_compact) and the hand-over of the arrays (pass2_give, pass2_fill) -- are shared with the colour-space entry, gm_read_mappings_cs (gm_host_pass2_cs.inc).

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
  const char* who = "gm_read_mappings";
  gm_session_t* s = nullptr; int read_len = 0, read_words = 0, W = 0, ops_cap = 0; bool want_ops = false, want_edit = false;
  int* d_thresh_tab = nullptr;                                  // (the call's GmDevMem owns it)
  std::vector<int32_t> sv; std::vector<gm_sw_full_rec_t> recs; std::vector<gm_mapping_t> maps;
  std::vector<uint64_t> map_off, cigar_off, edit_off;           // map_off[r + 1] / cigar_off[i + 1] are appended as reads / hits are answered; [0] = 0
  std::vector<char> cigar, edit; std::vector<uint8_t> ops;
  uint64_t ops_len = 0, full_calls = 0, full_cells = 0;
  // colour space (gm_read_mappings_cs): the caller's reads, primer letters and QV lines; per-read crossover and QV rows on the device (the call's GmDevMem owns them); post_sw
  bool colour = false, post_on = false, use_q = false; int is_rna = 0, qual_delta = 33, xstride = 0; double guard_tol = 1e-7;
  const uint32_t* reads_host = nullptr; const uint8_t* initbp_host = nullptr; std::vector<const char*> qptr;
  int8_t* d_xrows = nullptr; uint8_t* d_qv = nullptr; double* d_qtab = nullptr;
  std::vector<gm_post_rec_t> post; std::vector<char> post_quals, qralign; uint64_t post_redo = 0;
};
// the selection's device buffers of one sub-batch: allocated by its first selection, used again by the one behind a rounding-guard re-do
struct Pass2SelDev { GmP2Host* d_ans = nullptr; GmSel2Item* d_sel = nullptr; unsigned long long* d_hoff = nullptr; int32_t* d_order = nullptr; uint32_t* d_cnt = nullptr; };
}  // namespace

// hit_run_post_sw's tail per hit (ref: mapping.c:1609-1625) and the threshold compare, through the functions gm_select_pass2 calls: posterior[i] is the hit's
// posterior where it has one (score > 0 and mapping qualities on)
static inline GmP2Host pass2_answer(const gm_params_t& P, double al, double be, bool mqv_on, const GmP2In& in, double posterior) {
  int sf = in.score;
  if (sf > 0 && mqv_on) { int ps = gm_post_score(al, be, posterior, in.rmapped); if (ps < 0) ps = 0; sf = ps; }
  const int pct = (1000 * 100 * sf) / in.score_max;                      // ref: mapping.c:400-401
  GmP2Host a; a.score_full = sf; a.key = P.sw_full_threshold < 0 ? sf : pct;
  a.keep = (double)sf >= gm_full_threshold(P, in.score_max) ? 1 : 0;     // ref: mapping.c:1661 (double compare)
  return a;
}

// k_p2_sel_items and k_sel_pass2 on the host's answers, then the mappings of the sub-batch's reads in the reference's output order with z0 / z1 / mqv
// (compute_unpaired_mqv, ref: output.c:777-793,975-984), as gm_select_pass2 makes them.  Whatever an earlier selection of this sub-batch appended is dropped first.
// dev_post (colour space; else null): hit i's posterior is the device's -- the rounding guard of gm_select_pass2 is applied with the call's tolerance: near_read[r] says
// AS of one of read r's device posteriors lies at a rounding boundary, flag bit 0 marks the device mappings of a read at a boundary, *flagged lists those reads.
static int pass2_select(Pass2Call& C, const Pass1Batch& b, GmDevMem& mem, Pass2SelDev& sd, const gm_sw_full_rec_t* d_recs, const std::vector<GmP2In>& p2in,
                        const std::vector<GmP2Host>& ans, const std::vector<double>& posterior, size_t maps_before, const uint8_t* dev_post, const uint8_t* near_read,
                        std::vector<int>* flagged) {
  gm_session_t* s = C.s; const gm_params_t& P = s->P; hipStream_t q = s->stream;
  const int n = b.n, N = (int)b.nh; const uint64_t nh = b.nh;
  const bool mqv_on = gm_mqv_on(P); const double tol = C.guard_tol;
  C.maps.resize(maps_before); C.map_off.resize((size_t)b.base + 1);
  if (flagged) flagged->clear();
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "offsets are copied as they are");
  if (!sd.d_ans) {
    GM_HIP(mem.get(&sd.d_ans, (size_t)nh * sizeof(GmP2Host))); GM_HIP(mem.up(&sd.d_hoff, b.hit_off, (size_t)n + 1, q));
    GM_HIP(mem.get(&sd.d_sel, (size_t)nh * sizeof(GmSel2Item))); GM_HIP(mem.get(&sd.d_order, (size_t)nh * 4)); GM_HIP(mem.get(&sd.d_cnt, (size_t)n * 4));
  }
  GM_HIP(hipMemcpyAsync(sd.d_ans, ans.data(), (size_t)nh * sizeof(GmP2Host), hipMemcpyHostToDevice, q));
  int rc = gm_launch_p2_sel_items(N, b.d_hits, d_recs, sd.d_ans, sd.d_sel, q); if (rc) return rc;
  rc = gm_launch_sel_pass2(n, P.num_outputs, P.strata ? 1 : 0, P.max_alignments, sd.d_hoff, sd.d_sel, sd.d_order, sd.d_cnt, q); if (rc) return rc;
  std::vector<int32_t> order((size_t)nh); std::vector<uint32_t> cnt((size_t)n);
  GM_HIP(hipMemcpyAsync(order.data(), sd.d_order, (size_t)nh * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipMemcpyAsync(cnt.data(), sd.d_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  for (int r = 0; r < n; r++) {
    const uint64_t base = b.hit_off[r]; const uint64_t have = b.hit_off[r + 1] - base; const int m = (int)cnt[r];
    if ((uint64_t)m > have) { gm_set_error("%s: read %d: %d mappings of %llu hits", C.who, b.base + r, m, (unsigned long long)have); return GM_E_OVERFLOW; }
    const size_t first = C.maps.size();
    for (int k = 0; k < m; k++) {
      const int32_t ord = order[base + k];
      if (ord < 0 || (uint64_t)ord >= have) { gm_set_error("%s: read %d: mapping %d names hit %d of %llu", C.who, b.base + r, k, ord, (unsigned long long)have); return GM_E_OVERFLOW; }
      const uint64_t i = base + (uint64_t)ord;
      gm_mapping_t o; o.read = b.base + r; o.hit = (int32_t)(b.hits_before + i); o.score_full = ans[i].score_full; o.pct_score_full = (1000 * 100 * ans[i].score_full) / p2in[i].score_max;
      o.mqv = 255; o.flags = 0; o.posterior = posterior[i]; o.z0 = o.z1 = 0;
      C.maps.push_back(o);
    }
    if (m && mqv_on) {
      double z1 = 0.0;
      for (size_t k = first; k < C.maps.size(); k++) z1 += C.maps[k].posterior;
      for (size_t k = first; k < C.maps.size(); k++) { gm_mapping_t& o = C.maps[k]; o.z0 = o.posterior; o.z1 = z1; o.mqv = gm_unpaired_mqv(o.posterior, z1); }
      if (dev_post) {                                                    // the rounding guard, as gm_select_pass2 states it
        auto is_dev = [&](const gm_mapping_t& o) { return dev_post[(size_t)((uint64_t)o.hit - b.hits_before)] != 0; };
        bool dev = false, near = near_read[r] != 0;
        for (size_t k = first; k < C.maps.size(); k++) dev = dev || is_dev(C.maps[k]);
        if (dev) {
          near = near || gm_near_trunc(1000.0 * -log(z1), tol);
          for (size_t k = first; k < C.maps.size(); k++) near = near || gm_near_qv(C.maps[k].posterior / z1, tol) || gm_near_trunc(1000.0 * -log(C.maps[k].z0), tol);
        }
        if (near) for (size_t k = first; k < C.maps.size(); k++) if (is_dev(C.maps[k])) C.maps[k].flags |= 1;
      }
      if (P.single_best_mapping) {                                       // the first mapping with the highest quality
        size_t mx = first;
        for (size_t k = first + 1; k < C.maps.size(); k++) if (C.maps[k].mqv > C.maps[mx].mqv) mx = k;
        C.maps[first] = C.maps[mx]; C.maps.resize(first + 1);
      }
      if (flagged) { bool f = false; for (size_t k = first; k < C.maps.size(); k++) f = f || (C.maps[k].flags & 1); if (f) flagged->push_back(r); }
    } else for (size_t k = first; k < C.maps.size(); k++) C.maps[k].posterior = 0;
    C.map_off.push_back(C.maps.size());
  }
  return GM_OK;
}

// The text of the sub-batch's hits that are mappings, in hit order: k_sw_text's sizing launch, the host scan of the lengths and the writing launch; the CIGAR and edit
// bytes and the n_hits offsets are appended to the call's.  tail: the read positions behind the alignment (rmapped is the alignment's read positions in both spaces).
// Letter space: clip 'S', d_qin / d_db / d_qr null.  Colour space: clip 'H'; d_qin = post_sw's re-called qralign at the place of the operations, or, without post_sw,
// null and d_db / d_qr (zeroed, as large as the operations) to receive the strings rebuilt from the operations.  The copies of the bytes are queued: the caller
// synchronises; offs is the caller's for that reason (the scanned offsets on their way up).  h0: the index of the sub-batch's first record in C.recs.
static int pass2_text(Pass2Call& C, const Pass1Batch& b, GmDevMem& mem, size_t maps_before, size_t h0, const uint8_t* d_ops, const uint8_t* d_qin, uint8_t* d_db, uint8_t* d_qr,
                      int clip_char, std::vector<unsigned long long>& offs) {
  gm_session_t* s = C.s; const gm_index* ix = s->ix; hipStream_t q = s->stream;
  const uint64_t nh = b.nh; const int read_len = C.read_len, read_words = C.read_words, ops_cap = C.ops_cap;
  std::vector<uint8_t> mapped((size_t)nh, 0);
  for (size_t k = maps_before; k < C.maps.size(); k++) mapped[(size_t)((uint64_t)C.maps[k].hit - b.hits_before)] = 1;
  std::vector<GmTextItem> titems; std::vector<uint32_t> towner;
  for (uint64_t i = 0; i < nh; i++) {
    if (!mapped[i]) continue;
    const gm_pass1_hit_t& h = b.h_hits[i]; const gm_sw_full_rec_t& R = C.recs[h0 + i];
    const long long clen = (long long)ix->contig_off[h.cn + 1] - (long long)ix->contig_off[h.cn];
    if (R.score <= 0 || (uint64_t)R.n_ops > (uint64_t)ops_cap || R.genome_start < 0 || R.read_start < 0 || R.read_start + R.rmapped > read_len || R.genome_start + R.gmapped > clen) {
      gm_set_error("%s: hit %llu: a mapping whose record lies outside its window", C.who, (unsigned long long)(b.hits_before + i)); return GM_E_OVERFLOW; }
    GmTextItem it; memset(&it, 0, sizeof it);
    it.ops_off = R.ops_off; it.n_ops = R.n_ops; it.genome_start = R.genome_start; it.read_start = R.read_start; it.tail = read_len - R.read_start - R.rmapped;
    it.idx = h.read - b.base;                                            // the row of the sub-batch's reads
    if (C.colour && !d_qin) it.initbp = C.initbp_host[h.read];           // (the letters are translated from the colours)
    it.gbase = (long long)ix->contig_off[h.cn] + (h.gen_st ? clen - 1 : 0);
    it.flags = (h.gen_st ? 1 | 4 : 0) | ((ix->rna_ready && ix->contig_rna[h.cn]) ? 2 : 0);      // strand 1 of the contig, printed as a reverse-strand mapping
    titems.push_back(it); towner.push_back((uint32_t)i);
  }
  const size_t m = titems.size();
  const int what = GM_TEXT_CIGAR | (C.want_edit ? GM_TEXT_EDIT : 0) | (d_qr ? GM_TEXT_ALIGN : 0);
  const int colour = C.colour ? 1 : 0, is_rna = C.colour ? C.is_rna : 0;
  std::vector<uint32_t> lens(m * 2, 0); offs.assign(m * 2, 0);
  uint64_t cig_total = 0, edit_total = 0;
  const size_t cig0 = C.cigar.size(), ed0 = C.edit.size();
  if (m) {
    GmTextItem* d_ti = nullptr; uint32_t* d_lens = nullptr; unsigned long long* d_offs = nullptr; uint8_t *d_cig = nullptr, *d_ed = nullptr;
    GM_HIP(mem.up(&d_ti, titems.data(), m, q)); GM_HIP(mem.get(&d_lens, m * 2 * sizeof(uint32_t))); GM_HIP(mem.get(&d_offs, m * 2 * sizeof(unsigned long long)));
    int rc = gm_launch_sw_text((int)m, d_ti, colour, what, 0, d_ops, ix->d_genome, b.D->d_reads, read_words, is_rna, d_qin, clip_char, d_lens, d_offs, nullptr, nullptr, nullptr, nullptr, q, 1);
    if (rc != GM_OK) { gm_set_error("%s: the text kernel's launch failed", C.who); return rc; }
    GM_HIP(hipMemcpyAsync(lens.data(), d_lens, m * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    for (size_t k = 0; k < m; k++) { offs[2 * k] = cig_total; offs[2 * k + 1] = edit_total; cig_total += lens[2 * k]; edit_total += lens[2 * k + 1]; }
    GM_HIP(hipMemcpyAsync(d_offs, offs.data(), m * 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, q));
    GM_HIP(mem.get(&d_cig, (size_t)cig_total + 16));
    if (C.want_edit) GM_HIP(mem.get(&d_ed, (size_t)edit_total + 16));
    rc = gm_launch_sw_text((int)m, d_ti, colour, what, 1, d_ops, ix->d_genome, b.D->d_reads, read_words, is_rna, d_qin, clip_char, d_lens, d_offs, d_db, d_qr, d_cig, d_ed, q, 1);
    if (rc != GM_OK) { gm_set_error("%s: the text kernel's launch failed", C.who); return rc; }
    C.cigar.resize(cig0 + (size_t)cig_total); C.edit.resize(ed0 + (size_t)edit_total);
    if (cig_total) GM_HIP(hipMemcpyAsync(C.cigar.data() + cig0, d_cig, (size_t)cig_total, hipMemcpyDeviceToHost, q));
    if (C.want_edit && edit_total) GM_HIP(hipMemcpyAsync(C.edit.data() + ed0, d_ed, (size_t)edit_total, hipMemcpyDeviceToHost, q));
  }
  // n_hits + 1 offsets: a hit that is no mapping has an empty slice
  size_t k = 0; uint64_t c = cig0, e = ed0;
  for (uint64_t i = 0; i < nh; i++) {
    if (k < m && towner[k] == (uint32_t)i) { c += lens[2 * k]; e += lens[2 * k + 1]; k++; }
    C.cigar_off.push_back(c); if (C.want_edit) C.edit_off.push_back(e);
  }
  return GM_OK;
}

// The operations, compacted in hit order: the records point into that buffer whether or not it comes down.  loose: the device's operations (want_ops; else empty), hit
// i's at its record's ops_off; loose_qr (colour space; else null): the qralign bytes at the same places, compacted beside them.
static void pass2_compact(Pass2Call& C, const Pass1Batch& b, size_t h0, const std::vector<uint8_t>& loose, const std::vector<uint8_t>* loose_qr) {
  for (uint64_t i = 0; i < b.nh; i++) {
    gm_sw_full_rec_t& R = C.recs[h0 + i];
    const uint64_t dev_off = R.ops_off;
    R.ops_off = C.ops_len;
    if (R.n_ops) {
      if (C.want_ops) C.ops.insert(C.ops.end(), loose.begin() + (size_t)dev_off, loose.begin() + (size_t)dev_off + R.n_ops);
      if (loose_qr) C.qralign.insert(C.qralign.end(), loose_qr->begin() + (size_t)dev_off, loose_qr->begin() + (size_t)dev_off + R.n_ops);
      C.ops_len += R.n_ops;
    }
  }
}

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
    if (in.score > 0 && mqv_on) posterior[i] = gm_ls_posterior(al, be, in.score, in.rmapped);
    ans[i] = pass2_answer(P, al, be, mqv_on, in, posterior[i]);
  }
  const size_t h0 = C.recs.size();                                       // == b.hits_before
  C.recs.resize(h0 + (size_t)nh); C.sv.resize(h0 + (size_t)nh);
  GM_HIP(hipMemcpyAsync(C.recs.data() + h0, d_recs, (size_t)nh * sizeof(gm_sw_full_rec_t), hipMemcpyDeviceToHost, q));
  GM_HIP(hipMemcpyAsync(C.sv.data() + h0, d_sv, (size_t)nh * 4, hipMemcpyDeviceToHost, q));
  Pass2SelDev sd;
  rc = pass2_select(C, b, mem, sd, d_recs, p2in, ans, posterior, (size_t)maps_before, nullptr, nullptr, nullptr); if (rc) return rc;
  std::vector<unsigned long long> toffs;
  rc = pass2_text(C, b, mem, (size_t)maps_before, h0, d_ops, nullptr, nullptr, nullptr, 'S', toffs); if (rc) return rc;
  std::vector<uint8_t> loose;
  if (C.want_ops && n_work) { loose.resize((size_t)n_work * (size_t)ops_cap); GM_HIP(hipMemcpyAsync(loose.data(), d_ops, loose.size(), hipMemcpyDeviceToHost, q)); }
  GM_HIP(hipStreamSynchronize(q));
  pass2_compact(C, b, h0, loose, nullptr);
  for (uint64_t i = 0; i < nh; i++)
    if (C.sv[h0 + i] >= gm_full_thresh_int(P, b.h_hits[i].score_max)) { C.full_calls++; C.full_cells += (uint64_t)b.h_hits[i].w_len * (uint64_t)read_len; }
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

// the fields gm_read_mappings_t and gm_read_mappings_cs_t share, from the call's vectors (R zeroed by the caller; hits stay the caller's to hand over); false: out of memory
template <class Res> static bool pass2_fill(const Pass2Call& C, int n_reads, uint64_t n_hits, const std::vector<uint64_t>& hit_off, Res& R) {
  R.n_reads = n_reads; R.has_edit = C.want_edit ? 1 : 0; R.n_hits = n_hits; R.n_maps = C.maps.size(); R.cigar_len = C.cigar.size(); R.edit_len = C.edit.size(); R.ops_len = C.ops_len;
  return pass2_give(hit_off, &R.hit_off) && pass2_give(C.sv, &R.score_vector) && pass2_give(C.recs, &R.recs) && pass2_give(C.maps, &R.maps) &&
         pass2_give(C.map_off, &R.map_off) && pass2_give(C.cigar, &R.cigar) && pass2_give(C.cigar_off, &R.cigar_off) && pass2_give(C.edit, &R.edit) &&
         pass2_give(C.edit_off, &R.edit_off) && pass2_give(C.ops, &R.ops);
}

// thresh per possible score_max = min(read_len, w_len) * match, in the host's own double expression: the table k_p2_items reads, under the call's owner
static int pass2_thresh_table(gm_session_t* s, int read_len, GmDevMem& mem, int** d_tab) {
  std::vector<int> tab((size_t)read_len + 1);
  for (int m = 0; m <= read_len; m++) tab[m] = gm_full_thresh_int(s->P, m * s->P.match_score);
  GM_HIP(mem.up(d_tab, tab.data(), tab.size(), gm_sync));
  return GM_OK;
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
    GmDevMem mem;
    {
      GmDevTurn dev_turn(s);
      GM_HIP(hipSetDevice(s->ix->device));
      if (int rc = pass2_thresh_table(s, read_len, mem, &C.d_thresh_tab)) return rc;
    }
    const int rc = read_hits_impl("gm_read_mappings", s, n_reads, read_len, reads_packed, initbp, &hits, &n_hits, hit_off.data(), nullptr, nullptr, nullptr, nullptr, stats, pass2_batch, &C);
    if (rc) { if (stats) memset(stats, 0, sizeof *stats); return rc; }
    if (C.recs.size() != n_hits || C.map_off.size() != (size_t)n_reads + 1 || C.cigar_off.size() != (size_t)n_hits + 1) {
      gm_set_error("gm_read_mappings: %zu records of %llu hits, %zu map offsets of %d reads", C.recs.size(), (unsigned long long)n_hits, C.map_off.size(), n_reads); return GM_E_OVERFLOW; }
  }
  gm_read_mappings_t R; memset(&R, 0, sizeof R);
  if (!pass2_fill(C, nr, n_hits, hit_off, R)) { gm_read_mappings_free(&R); gm_set_error("gm_read_mappings: out of memory at %llu hits", (unsigned long long)n_hits); return GM_E_NOMEM; }
  R.hits = hits; hits = nullptr;
  if (stats) { stats->full_calls = C.full_calls; stats->full_cells = C.full_cells; }
  *out = R;
  return GM_OK;
}
