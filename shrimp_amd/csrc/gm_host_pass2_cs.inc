// gm_host_pass2_cs.inc -- colour-space pass 2 as a seam: gm_read_mappings_cs (colour reads to mappings in one call); part of gm_host.hip.
//
// Behind the front of gm_read_hits, per sub-batch, on hits that stay on the device (ref: mapping.c:375-379, 1609-1625):
//   k_p2_items_cs          the colour-space by-row items: every hit, no second score, no compaction;
//   k_sw_full_cs_batch     in its by-row form (the read and its crossover row by the ROW of the sub-batch's reads; one row a read went up once per call);
//   k_p2_records_cs        the records gm_sw_full_cs_batch_ix leaves, the three integers of the host's double functions, the read positions post_sw takes;
//   the records come down and are checked against their windows (the device made them: a record outside its window is a bug, GM_E_OVERFLOW);
//   k_win_scan             the exclusive scan of those read positions: where every hit's base qualities go (no atomics);
//   k_p2_post_items        post_sw's items from the device records;
//   k_post_sw_batch<true>  one launch (one length class: the reads of a call have one length), thread slots by post_plan's budget rule, under the SESSION's constants
//                          (cs_post_consts(s), the session's QV table) on the operations k_sw_full_cs_batch left in device memory;
//   the answers (GmPostRes, 24 bytes a hit) come down; an item the kernel flags (valid == 2) is redone by cs_post_sw on the host -- its operations are gathered on the
//   device and come down packed, its genome stretch through gm_index_get_windows, its read is the caller's: bytes bounded by the flagged items;
//   pass2_select           the selection and the mappings with the rounding guard inside; a read whose mappings come out with flag bit 0 has its device posteriors redone
//                          on the host and the selection runs once more (after it every hit of those reads is by_host, so no flag is left);
//   pass2_text             k_sw_text with colour = 1 and clip 'H' over the mappings, d_qin = post_sw's re-called qralign (without post_sw: the strings rebuilt from the
//                          operations, whose qralign is the result's);
//   pass2_compact          the operations and the qralign bytes compacted in hit order.
// A fixed number of allocations, copies and launches a sub-batch (one more selection when the guard fires).  The checks are made on the host before anything is uploaded.

extern "C" int gm_read_mappings_cs_size(void) { return (int)sizeof(gm_read_mappings_cs_t); }

extern "C" void gm_read_mappings_cs_free(gm_read_mappings_cs_t* out) {
  if (!out) return;
  void* ptrs[] = {out->hits, out->hit_off, out->score_vector, out->recs, out->maps, out->map_off, out->cigar, out->cigar_off, out->edit, out->edit_off, out->ops,
                  out->post, out->post_quals, out->qralign};
  for (void* p : ptrs) free(p);
  memset(out, 0, sizeof *out);
}

// (the front's own limit on the read length: pass2_front_prune_lds, beside check_read_len in gm_host.hip)
namespace {
// one sub-batch of gm_read_mappings_cs behind its records: post_sw's answers per hit and the host re-dos
struct Pass2CsBatch {
  Pass2Call& C; const Pass1Batch& b; GmDevMem& mem; size_t h0;
  uint8_t *d_ops = nullptr, *d_qa = nullptr, *d_quals = nullptr;
  std::vector<unsigned long long> qoff;                        // the exclusive scan of the read positions, as k_win_scan leaves it
  std::vector<gm_post_rec_t> post; std::vector<double> posterior; std::vector<uint8_t> dev_post;
  Pass2CsBatch(Pass2Call& C_, const Pass1Batch& b_, GmDevMem& mem_, size_t h0_) : C(C_), b(b_), mem(mem_), h0(h0_) {}

  // cs_post_sw for the hits `list` (indices within the sub-batch, ascending), as gm_post_sw_batch_ix redoes an item: the strings from the record, the host routine, the
  // re-called qralign and the base qualities back to their places in d_qa / d_quals
  int redo(const std::vector<uint32_t>& list) {
    if (list.empty()) return GM_OK;
    gm_session_t* s = C.s; const gm_index* ix = s->ix; hipStream_t q = s->stream;
    const size_t m = list.size();
    std::vector<GmP2Seg> segs(m); uint64_t total = 0;
    for (size_t k = 0; k < m; k++) { const gm_sw_full_rec_t& R = C.recs[h0 + list[k]]; segs[k].src = R.ops_off; segs[k].dst = total; segs[k].len = R.n_ops; segs[k].pad = 0; total += R.n_ops; }
    GmP2Seg* d_segs = nullptr; uint8_t* d_pack = nullptr;
    GM_HIP(mem.up(&d_segs, segs.data(), m, q)); GM_HIP(mem.get(&d_pack, (size_t)total + 16));
    int rc = gm_launch_p2_move((int)m, d_segs, d_ops, d_pack, q); if (rc) return rc;
    std::vector<uint8_t> pack((size_t)total + 1);
    if (total) GM_HIP(hipMemcpyAsync(pack.data(), d_pack, (size_t)total, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    mem.drop(d_pack);
    // the genome stretch of every alignment, each as a bitfield of its own
    std::vector<int> wcn, wlen, slot(m, -1); std::vector<uint8_t> wst; std::vector<int64_t> woff; int wstride = 0;
    for (size_t k = 0; k < m; k++) {
      const gm_sw_full_rec_t& R = C.recs[h0 + list[k]]; const gm_pass1_hit_t& h = b.h_hits[list[k]];
      int adv_g = 0; for (uint32_t t = 0; t < R.n_ops; t++) { const int type = pack[segs[k].dst + t] & 0x0f; if (!(type >= 2 && type <= 5)) adv_g++; }
      if (adv_g < 1) continue;
      slot[k] = (int)wcn.size(); wcn.push_back(h.cn); wst.push_back((uint8_t)h.gen_st); woff.push_back(R.genome_start); wlen.push_back(adv_g);
      wstride = std::max(wstride, (adv_g + 7) / 8);
    }
    std::vector<uint32_t> hw;
    if (!wcn.empty()) {
      hw.assign(wcn.size() * (size_t)wstride, 0);
      rc = gm_index_get_windows(ix, (int)wcn.size(), wcn.data(), wst.data(), woff.data(), wlen.data(), 0, hw.data(), wstride); if (rc) return rc;
    }
    const CsPostConsts K = cs_post_consts(s);
    std::vector<uint8_t> patch; std::vector<GmP2Seg> qa_segs, ql_segs;
    static const uint32_t no_genome[1] = {0};
    for (size_t k = 0; k < m; k++) {
      const uint32_t i = list[k]; const gm_sw_full_rec_t& R = C.recs[h0 + i]; const gm_pass1_hit_t& h = b.h_hits[i];
      const uint32_t* rw = C.reads_host + (size_t)h.read * C.read_words; const int ib = C.initbp_host[h.read];
      gm_sw_full_rec_t rloc = R; rloc.genome_start = 0; rloc.ops_off = segs[k].dst;      // the record against its own stretch and the packed operations
      const uint32_t* hg = slot[k] >= 0 ? hw.data() + (size_t)slot[k] * wstride : no_genome; const uint64_t hg_len = slot[k] >= 0 ? (uint64_t)wstride * 8 : 0;
      char *db = nullptr, *qr = nullptr;
      rc = gm_sw_full_batch_strings(1, &rloc, pack.data(), total, hg, hg_len, rw, C.read_len, ib, C.is_rna, &db, &qr);
      if (rc != GM_OK || !db || !qr) { free(db); free(qr); gm_set_error("%s: hit %llu: the strings of a record the device made cannot be built", C.who, (unsigned long long)(b.hits_before + i)); return GM_E_OVERFLOW; }
      FHit fh; fh.db = db; fh.qr = qr; free(db); free(qr);
      cs_post_sw(K, rw, ib, R.read_start, fh, C.use_q ? C.qptr[h.read] : nullptr, C.qual_delta, true);
      gm_post_rec_t& P = post[i];
      P.posterior = fh.posterior; P.matches = fh.cs_match; P.mismatches = fh.cs_mismatch; P.crossovers = fh.cs_xover; P.by_host = 1;
      posterior[i] = fh.posterior; dev_post[i] = 0;
      GmP2Seg a; a.pad = 0; a.src = patch.size(); a.dst = R.ops_off; a.len = (uint32_t)std::min<size_t>(fh.qr.size(), R.n_ops);
      patch.insert(patch.end(), fh.qr.begin(), fh.qr.begin() + a.len); qa_segs.push_back(a);
      a.src = patch.size(); a.dst = qoff[i]; a.len = (uint32_t)std::min<size_t>(fh.qual.size(), (size_t)P.qual_len);
      patch.insert(patch.end(), fh.qual.begin(), fh.qual.begin() + a.len); ql_segs.push_back(a);
    }
    uint8_t* d_patch = nullptr; GmP2Seg *d_qa_segs = nullptr, *d_ql_segs = nullptr;
    if (!patch.empty()) {
      GM_HIP(mem.up(&d_patch, patch.data(), patch.size(), q, 16)); GM_HIP(mem.up(&d_qa_segs, qa_segs.data(), m, q)); GM_HIP(mem.up(&d_ql_segs, ql_segs.data(), m, q));
      rc = gm_launch_p2_move((int)m, d_qa_segs, d_patch, d_qa, q); if (rc) return rc;
      rc = gm_launch_p2_move((int)m, d_ql_segs, d_patch, d_quals, q); if (rc) return rc;
      GM_HIP(hipStreamSynchronize(q));                                   // (the patch and its segments leave their scope)
    }
    C.post_redo += m;
    return GM_OK;
  }
};
}  // namespace

static int pass2_cs_batch(void* ctx, const Pass1Batch& b) {
  Pass2Call& C = *(Pass2Call*)ctx;
  gm_session_t* s = C.s; const gm_params_t& P = s->P; const gm_index* ix = s->ix;
  const int n = b.n; const uint64_t nh = b.nh;
  const uint64_t maps_before = C.maps.size();
  if (nh == 0) { for (int r = 0; r < n; r++) C.map_off.push_back(maps_before); return GM_OK; }
  hipStream_t q = s->stream;
  const int read_len = C.read_len, read_words = C.read_words, W = C.W, ops_cap = C.ops_cap, N = (int)nh;
  const size_t ops_bytes = (size_t)nh * (size_t)ops_cap;
  GmDevMem mem;
  GmFullItem* d_items = nullptr; GmFullOut* d_out = nullptr; gm_sw_full_rec_t* d_recs = nullptr; GmP2In* d_p2in = nullptr; uint32_t *d_len = nullptr, *d_back = nullptr; uint8_t* d_ops = nullptr;
  GM_HIP(mem.get(&d_items, (size_t)nh * sizeof(GmFullItem))); GM_HIP(mem.get(&d_out, (size_t)nh * sizeof(GmFullOut))); GM_HIP(mem.get(&d_recs, (size_t)nh * sizeof(gm_sw_full_rec_t)));
  GM_HIP(mem.get(&d_p2in, (size_t)nh * sizeof(GmP2In))); GM_HIP(mem.get(&d_len, (size_t)nh * 4 + 64)); GM_HIP(mem.get(&d_ops, ops_bytes + 16));
  // the items and the full alignment of every hit, by as many waves as the back-pointer budget allows (swf_plan's rule for one class; three words a cell)
  int rc = gm_launch_p2_items_cs(N, b.d_hits, b.base, read_len, ix->d_contig_off, ix->d_contig_rna, C.d_thresh_tab, P.tiebreak_rev ? 1 : 0, ops_cap, b.D->d_initbp, C.is_rna, d_items, q);
  if (rc) return rc;
  {
    const size_t stride = ((size_t)W * (size_t)read_len * 12 + 256 + 15) & ~(size_t)15;
    const int grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min<uint64_t>(nh, (uint64_t)GM_SWF_MAX_GRID), GM_SWF_BACK_BUDGET / stride));
    GM_HIP(mem.get(&d_back, (size_t)grid * stride));
    int cs9[9]; cs_setup_args(P, cs9);
    rc = gm_launch_sw_full_cs_batch(cs9, 0, N, grid, d_items, ix->d_genome, b.D->d_reads, read_words, W, read_len, C.use_q ? C.d_xrows + (size_t)b.base * C.xstride : nullptr, C.xstride,
                                    d_back, stride / 4, d_out, d_ops, P.local_alignment ? 1 : 0, q, 1, 1);
    if (rc) return rc;
  }
  rc = gm_launch_p2_records_cs(N, b.d_hits, d_out, ops_cap, d_recs, d_p2in, d_len, q); if (rc) return rc;
  std::vector<GmP2In> p2in((size_t)nh);
  const size_t h0 = C.recs.size();                                       // == b.hits_before
  C.recs.resize(h0 + (size_t)nh); C.sv.resize(h0 + (size_t)nh);
  GM_HIP(hipMemcpyAsync(p2in.data(), d_p2in, (size_t)nh * sizeof(GmP2In), hipMemcpyDeviceToHost, q));
  GM_HIP(hipMemcpyAsync(C.recs.data() + h0, d_recs, (size_t)nh * sizeof(gm_sw_full_rec_t), hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  // the records against their windows; ZV is pass 1's score (no second vector call, ref: mapping.c:375-379)
  Pass2CsBatch B(C, b, mem, h0);
  B.qoff.resize((size_t)nh + 1); B.post.resize((size_t)nh); B.posterior.assign((size_t)nh, 0.0); B.dev_post.assign((size_t)nh, 0);
  unsigned long long quals_total = 0;
  for (uint64_t i = 0; i < nh; i++) {
    const gm_pass1_hit_t& h = b.h_hits[i]; const gm_sw_full_rec_t& R = C.recs[h0 + i];
    C.sv[h0 + i] = h.score_vector;
    if (p2in[i].score_max < 1) { gm_set_error("%s: hit %llu: score_max %d", C.who, (unsigned long long)(b.hits_before + i), p2in[i].score_max); return GM_E_ARG; }
    gm_post_rec_t& Q = B.post[i]; memset(&Q, 0, sizeof Q);
    B.qoff[i] = quals_total;
    if (C.post_on) Q.qual_off = C.post_quals.size() + quals_total;      // (a hit without alignment: an empty slice at the running offset)
    if (R.score <= 0) continue;
    if (R.n_ops < 1 || (uint64_t)R.n_ops > (uint64_t)ops_cap || R.ops_off != (uint64_t)i * (uint64_t)ops_cap || R.read_start < 0 || R.rmapped < 0 || R.read_start + R.rmapped > read_len ||
        R.gmapped < 0 || R.genome_start < (int64_t)h.g_off || R.genome_start + R.gmapped > (int64_t)h.g_off + h.w_len) {
      gm_set_error("%s: hit %llu: a record that lies outside its window", C.who, (unsigned long long)(b.hits_before + i)); return GM_E_OVERFLOW; }
    if (C.post_on) { Q.qual_len = (uint32_t)R.rmapped; quals_total += (unsigned long long)R.rmapped; }
  }
  B.qoff[nh] = quals_total;
  // post_sw of every hit with an alignment, under the session's constants
  const bool mqv_on = gm_mqv_on(P);
  const double al = s->score_alpha, be = s->score_beta;
  std::vector<uint8_t> near_read((size_t)n, 0);
  B.d_ops = d_ops;
  if (C.post_on) {
    unsigned long long* d_qoff = nullptr; GmPostItem* d_pitems = nullptr; GmPostRes* d_pres = nullptr; double* d_fw = nullptr; uint32_t* d_info = nullptr;
    GM_HIP(mem.get(&d_qoff, ((size_t)nh + 1) * 8)); GM_HIP(mem.get(&d_pitems, (size_t)nh * sizeof(GmPostItem))); GM_HIP(mem.get(&d_pres, (size_t)nh * sizeof(GmPostRes)));
    GM_HIP(mem.get(&B.d_qa, ops_bytes + 16)); GM_HIP(mem.get(&B.d_quals, (size_t)quals_total + 16));
    GM_HIP(hipMemsetAsync(B.d_qa, 0, ops_bytes + 16, q)); GM_HIP(hipMemsetAsync(B.d_quals, 0, (size_t)quals_total + 16, q));
    rc = gm_launch_win_scan(d_len, N, INT_MAX, d_qoff, q); if (rc) return rc;
    rc = gm_launch_p2_post_items(N, b.d_hits, d_recs, d_qoff, b.base, read_len, ix->d_contig_off, ix->d_contig_rna, b.D->d_initbp, d_pitems, q); if (rc) return rc;
    // thread slots by post_plan's budget rule for one class of read_len columns
    const size_t want = std::min<size_t>(((size_t)nh + 63) & ~(size_t)63, (size_t)GM_POST_THREADS);
    const size_t fit = (GM_POST_BUDGET / ((size_t)read_len * GM_POST_COL_BYTES)) & ~(size_t)63;
    const int threads = (int)std::max<size_t>(64, std::min(want, fit));
    GM_HIP(mem.get(&d_fw, (size_t)threads * read_len * 17 * 8)); GM_HIP(mem.get(&d_info, (size_t)threads * read_len * 4));
    GmCsPostDev K; const CsPostConsts c = cs_post_consts(s);
    K.let_m = c.let_m; K.let_x = c.let_x; K.col_m[0] = c.col_m[0]; K.col_m[1] = c.col_m[1]; K.col_x[0] = c.col_x[0]; K.col_x[1] = c.col_x[1];
    K.pr_del_open = c.pr_del_open; K.pr_del_extend = c.pr_del_extend; K.pr_ins_open = c.pr_ins_open; K.pr_ins_extend = c.pr_ins_extend;
    K.qv = C.use_q ? C.d_qv + (size_t)b.base * C.xstride : nullptr; K.qtab = C.use_q ? C.d_qtab : nullptr; K.bq = nullptr;
    rc = gm_launch_post_sw_batch(K, 0, N, threads, d_pitems, d_ops, ix->d_genome, b.D->d_reads, read_words, C.xstride, C.is_rna, d_pres, B.d_qa, B.d_quals, d_fw, d_info, q, 1);
    if (rc != GM_OK) { gm_set_error("%s: the post_sw kernel's launch failed", C.who); return rc; }
    std::vector<GmPostRes> pres((size_t)nh); unsigned long long dev_total = 0;
    GM_HIP(hipMemcpyAsync(pres.data(), d_pres, (size_t)nh * sizeof(GmPostRes), hipMemcpyDeviceToHost, q));
    GM_HIP(hipMemcpyAsync(&dev_total, d_qoff + nh, 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    // B.qoff is the host's scan of the records that came down, d_qoff the device's of the same records: the re-dos patch d_quals by the host's offsets, so the two must agree
    if (dev_total != quals_total) { gm_set_error("%s: %llu base qualities on the device, %llu on the host", C.who, dev_total, quals_total); return GM_E_OVERFLOW; }
    std::vector<uint32_t> by_host;
    for (uint64_t i = 0; i < nh; i++) {
      if (C.recs[h0 + i].score <= 0) continue;
      if (pres[i].valid != 1) { by_host.push_back((uint32_t)i); continue; }
      gm_post_rec_t& Q = B.post[i];
      Q.posterior = pres[i].posterior; Q.matches = pres[i].cs_match; Q.mismatches = pres[i].cs_mismatch; Q.crossovers = pres[i].cs_xover;
      B.posterior[i] = pres[i].posterior; B.dev_post[i] = 1;
    }
    rc = B.redo(by_host); if (rc) return rc;
    for (int r = 0; r < n; r++) for (uint64_t i = b.hit_off[r]; i < b.hit_off[r + 1]; i++)      // AS at a rounding boundary
      if (B.dev_post[i] && gm_near_rint(gm_post_score_x(al, be, B.posterior[i], p2in[i].rmapped), C.guard_tol)) near_read[r] = 1;
  }
  // hit_run_post_sw's tail and the threshold compare, the selection, the guard
  std::vector<GmP2Host> ans((size_t)nh);
  for (uint64_t i = 0; i < nh; i++) ans[i] = pass2_answer(P, al, be, mqv_on, p2in[i], B.posterior[i]);
  Pass2SelDev sd; std::vector<int> flagged;
  rc = pass2_select(C, b, mem, sd, d_recs, p2in, ans, B.posterior, (size_t)maps_before, C.post_on ? B.dev_post.data() : nullptr, near_read.data(), &flagged); if (rc) return rc;
  if (!flagged.empty()) {
    std::vector<uint32_t> list;
    for (int r : flagged) for (uint64_t i = b.hit_off[r]; i < b.hit_off[r + 1]; i++) if (B.dev_post[i]) list.push_back((uint32_t)i);
    rc = B.redo(list); if (rc) return rc;
    for (uint32_t i : list) ans[i] = pass2_answer(P, al, be, mqv_on, p2in[i], B.posterior[i]);
    for (int r : flagged) near_read[r] = 0;                              // (no device posterior is left among their hits)
    rc = pass2_select(C, b, mem, sd, d_recs, p2in, ans, B.posterior, (size_t)maps_before, B.dev_post.data(), near_read.data(), &flagged); if (rc) return rc;
    if (!flagged.empty()) { gm_set_error("%s: read %d is flagged after its posteriors were redone on the host", C.who, b.base + flagged[0]); return GM_E_OVERFLOW; }
  }
  // the text of the mappings: clip 'H'; the read letters are post_sw's, or without post_sw those the text kernel rebuilds (its qralign is the result's)
  uint8_t *d_db = nullptr, *d_qr = nullptr;
  if (!C.post_on) {
    GM_HIP(mem.get(&d_db, ops_bytes + 16)); GM_HIP(mem.get(&d_qr, ops_bytes + 16));
    GM_HIP(hipMemsetAsync(d_db, 0, ops_bytes + 16, q)); GM_HIP(hipMemsetAsync(d_qr, 0, ops_bytes + 16, q));
  }
  std::vector<unsigned long long> toffs;
  rc = pass2_text(C, b, mem, (size_t)maps_before, h0, d_ops, C.post_on ? B.d_qa : nullptr, d_db, d_qr, 'H', toffs); if (rc) return rc;
  std::vector<uint8_t> loose, loose_qr(ops_bytes);
  if (C.want_ops) { loose.resize(ops_bytes); GM_HIP(hipMemcpyAsync(loose.data(), d_ops, ops_bytes, hipMemcpyDeviceToHost, q)); }
  GM_HIP(hipMemcpyAsync(loose_qr.data(), C.post_on ? B.d_qa : d_qr, ops_bytes, hipMemcpyDeviceToHost, q));
  const size_t pq0 = C.post_quals.size();
  if (C.post_on && quals_total) { C.post_quals.resize(pq0 + (size_t)quals_total); GM_HIP(hipMemcpyAsync(C.post_quals.data() + pq0, B.d_quals, (size_t)quals_total, hipMemcpyDeviceToHost, q)); }
  GM_HIP(hipStreamSynchronize(q));
  pass2_compact(C, b, h0, loose, &loose_qr);
  if (C.post_on) C.post.insert(C.post.end(), B.post.begin(), B.post.end());
  for (uint64_t i = 0; i < nh; i++) { C.full_calls++; C.full_cells += (uint64_t)b.h_hits[i].w_len * (uint64_t)read_len; }
  return GM_OK;
}

extern "C" int gm_read_mappings_cs(gm_session_t* s, int n_reads, int n_colours, const uint32_t* colours_packed, const uint8_t* initbp, const char* quals, int qual_delta,
                                   int want_ops, gm_read_mappings_cs_t* out, gm_map_stats_t* stats) {
  const char* who = "gm_read_mappings_cs";
  if (!s || !out) { gm_set_error("gm_read_mappings_cs: bad arguments (the session and the result struct are required)"); return GM_E_ARG; }
  memset(out, 0, sizeof *out);
  if (stats) memset(stats, 0, sizeof *stats);
  if (!s->P.colour_space) { gm_set_error("gm_read_mappings_cs: a letter-space session: use gm_read_mappings"); return GM_E_ARG; }
  Pass2Call C; C.who = who; C.s = s; C.want_ops = want_ops != 0; C.want_edit = s->P.extra_sam_fields != 0; C.colour = true; C.post_on = gm_mqv_on(s->P);
  C.map_off.push_back(0); C.cigar_off.push_back(0); if (C.want_edit) C.edit_off.push_back(0);
  const int nr = std::max(n_reads, 0);
  std::vector<uint64_t> hit_off((size_t)nr + 1, 0);
  gm_pass1_hit_t* hits = nullptr; uint64_t n_hits = 0;
  struct HitsGuard { gm_pass1_hit_t*& p; ~HitsGuard() { free(p); } } guard{hits};
  if (n_reads > 0) {
    const int read_len = n_colours;
    if (int rc = pass1_reads_check(who, s, n_reads, read_len, colours_packed, initbp)) return rc;
    if (int rc = pass1_k_check(who, s)) return rc;
    if (quals) {
      if (int rc = split_lines(quals, n_reads, C.qptr, nullptr, read_len, "gm_read_mappings_cs: read %d: QUAL string of %d characters for %d colours")) return rc;
      if (2 * s->P.crossover_score < -128) { gm_set_error("crossover score %d: per-position scores are kept in 8 bits", s->P.crossover_score); return GM_E_RANGE; }
    }
    C.use_q = quals != nullptr && !s->P.ignore_qvs; C.qual_delta = qual_delta;
    const int W = window_len_of(s->P, read_len);
    if (gm_score_windows_lds(1, read_len, W) > GM_SCORE_WIN_LDS_LIMIT) { gm_set_error("gm_read_mappings_cs: windows of %d positions beside reads of %d are beyond the scoring kernel's LDS", W, read_len); return GM_E_RANGE; }
    if (gm_sw_full_cs_batch_lds(W, read_len) > GM_SWF_LDS_LIMIT) { gm_set_error("gm_read_mappings_cs: windows of %d positions beside reads of %d are beyond the full-alignment kernel's LDS", W, read_len); return GM_E_RANGE; }
    if (pass2_front_prune_lds(s, read_len) > GM_SWF_LDS_LIMIT) { gm_set_error("gm_read_mappings_cs: reads of %d colours are beyond the LDS of the front's prune kernel on this index", read_len); return GM_E_RANGE; }
    // (defence only: the LDS tests above admit no read of more than a few thousand colours, a post_sw thread's column scratch holds 59 918)
    if ((uint64_t)read_len > GM_POST_BUDGET / (64 * GM_POST_COL_BYTES)) { gm_set_error("gm_read_mappings_cs: reads of %d colours are beyond the column scratch of one post_sw thread", read_len); return GM_E_RANGE; }
    C.read_len = read_len; C.read_words = (read_len + 7) / 8; C.W = W; C.ops_cap = W + read_len + 8;
    C.reads_host = colours_packed; C.initbp_host = initbp; C.is_rna = s->ix->genome_is_rna ? 1 : 0;
    if (const char* e = gm_tune("GM_POST_GUARD_TOL")) C.guard_tol = atof(e);
    // one crossover row and one QV row a read (ref: gmapper.c:532-544), made by the function the mapping entry uses, up once per call
    std::vector<int8_t> xrows; std::vector<uint8_t> qv;
    if (C.use_q) {
      C.xstride = (read_len + 15) & ~15;
      xrows.assign((size_t)n_reads * C.xstride, 0); qv.assign((size_t)n_reads * C.xstride, 0);
      for (int i = 0; i < n_reads; i++) xover_from_quals(s, &C.qptr[i], 1, read_len, qual_delta, xrows.data() + (size_t)i * C.xstride, qv.data() + (size_t)i * C.xstride);
    }
    GmDevMem mem;
    {
      GmDevTurn dev_turn(s);
      GM_HIP(hipSetDevice(s->ix->device));
      if (int rc = pass2_thresh_table(s, read_len, mem, &C.d_thresh_tab)) return rc;
      if (C.use_q) {
        GM_HIP(mem.up(&C.d_xrows, xrows.data(), xrows.size(), gm_sync, 64)); GM_HIP(mem.up(&C.d_qv, qv.data(), qv.size(), gm_sync, 64));
        C.d_qtab = s->d_qtab;
        if (!C.d_qtab) { const std::vector<double> qt = cs_qv_table(true); GM_HIP(mem.up(&C.d_qtab, qt.data(), qt.size(), gm_sync)); }
      }
    }
    const int rc = read_hits_impl(who, s, n_reads, read_len, colours_packed, initbp, &hits, &n_hits, hit_off.data(), nullptr, nullptr, nullptr, nullptr, stats, pass2_cs_batch, &C);
    if (rc) { if (stats) memset(stats, 0, sizeof *stats); return rc; }
    if (C.recs.size() != n_hits || C.map_off.size() != (size_t)n_reads + 1 || C.cigar_off.size() != (size_t)n_hits + 1 || (C.post_on && C.post.size() != n_hits) || C.qralign.size() != C.ops_len) {
      gm_set_error("gm_read_mappings_cs: %zu records of %llu hits, %zu map offsets of %d reads", C.recs.size(), (unsigned long long)n_hits, C.map_off.size(), n_reads); return GM_E_OVERFLOW; }
  }
  gm_read_mappings_cs_t R; memset(&R, 0, sizeof R);
  R.post_quals_len = C.post_quals.size();
  if (!(pass2_fill(C, nr, n_hits, hit_off, R) && pass2_give(C.post, &R.post) && pass2_give(C.post_quals, &R.post_quals) && pass2_give(C.qralign, &R.qralign))) {
    gm_read_mappings_cs_free(&R); gm_set_error("gm_read_mappings_cs: out of memory at %llu hits", (unsigned long long)n_hits); return GM_E_NOMEM; }
  R.hits = hits; hits = nullptr;
  if (stats) { stats->full_calls = C.full_calls; stats->full_cells = C.full_cells; stats->post_sw_host_redo = C.post_redo; }
  *out = R;
  return GM_OK;
}
