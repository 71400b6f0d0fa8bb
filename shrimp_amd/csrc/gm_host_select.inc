// gm_host_select.inc -- gm_select_pass1 / gm_select_pass2: the two selections of a read batch as public seams on caller arrays; part of gm_host.hip.
//
// Pass 1: the windows, their offsets and their scores go up whole (52 bytes a window), k_sel_pass1 leaves K slots a read, the slot counts are scanned by the scan of
// gm_read_windows (k_win_scan, the counts clamped to 64), k_sel_emit writes the tight records, and the offsets and the records come back.
// Pass 2: the host makes score_full, the posterior, the key and the threshold compare of every hit (doubles through libm: the functions the finalisation of the mapping
// entries uses), 24 bytes an item go up, k_sel_pass2 leaves the order of every read's final mappings, and the host adds z0 / z1 / mqv in that order.
// Every buffer is sized by the call's n: a fixed number of allocations, copies and launches.

extern "C" int gm_pass1_hit_size(void) { return (int)sizeof(gm_pass1_hit_t); }
extern "C" int gm_mapping_size(void) { return (int)sizeof(gm_mapping_t); }

extern "C" int gm_select_pass1(gm_session_t* s, int n_reads, int read_len, const gm_read_window_t* wins, uint64_t n_wins, const uint64_t* off, const int* scores,
                               gm_pass1_hit_t** hits, uint64_t* n_hits, uint64_t* hit_off) {
  if (!s || !hits || !n_hits || !hit_off) { gm_set_error("gm_select_pass1: bad arguments"); return GM_E_ARG; }
  *hits = nullptr; *n_hits = 0; hit_off[0] = 0;
  if (n_reads <= 0) return GM_OK;
  if (!off || read_len < 1 || (n_wins && (!wins || !scores))) { gm_set_error("gm_select_pass1: bad arguments"); return GM_E_ARG; }
  const int K = s->P.num_tmp_outputs;
  if (K > GM_SEL_MAX) { gm_set_error("gm_select_pass1: num_tmp_outputs %d is beyond the %d hits a read this entry selects", K, GM_SEL_MAX); return GM_E_RANGE; }
  if (K < 1) { gm_set_error("gm_select_pass1: num_tmp_outputs %d", K); return GM_E_ARG; }
  if (n_wins >= (1ull << 31)) { gm_set_error("gm_select_pass1: %llu windows (a hit names its window in 31 bits)", (unsigned long long)n_wins); return GM_E_RANGE; }
  const gm_index* ix = s->ix;
  if (off[0] != 0 || off[(size_t)2 * n_reads] != n_wins) { gm_set_error("gm_select_pass1: the offsets run from %llu to %llu, the windows from 0 to %llu", (unsigned long long)off[0], (unsigned long long)off[(size_t)2 * n_reads], (unsigned long long)n_wins); return GM_E_ARG; }
  for (size_t rs = 0; rs < (size_t)2 * n_reads; rs++)
    if (off[rs + 1] < off[rs] || off[rs + 1] > n_wins) { gm_set_error("gm_select_pass1: offsets not ascending at read %zu strand %zu", rs >> 1, rs & 1); return GM_E_ARG; }
  for (size_t rs = 0; rs < (size_t)2 * n_reads; rs++) {
    for (uint64_t i = off[rs]; i < off[rs + 1]; i++) {
      const gm_read_window_t& w = wins[i];
      if (w.read != (int32_t)(rs >> 1) || w.st != (int32_t)(rs & 1)) { gm_set_error("gm_select_pass1: window %llu says read %d strand %d in the list of read %zu strand %zu", (unsigned long long)i, w.read, w.st, rs >> 1, rs & 1); return GM_E_ARG; }
      if (w.cn < 0 || w.cn >= ix->n_contigs) { gm_set_error("gm_select_pass1: window %llu: contig %d of %d", (unsigned long long)i, w.cn, ix->n_contigs); return GM_E_ARG; }
      if (w.w_len < 1) { gm_set_error("gm_select_pass1: window %llu: w_len %d", (unsigned long long)i, w.w_len); return GM_E_ARG; }
      if ((uint64_t)w.g_off + (uint64_t)w.w_len > (uint64_t)(ix->contig_off[w.cn + 1] - ix->contig_off[w.cn])) { gm_set_error("gm_select_pass1: window %llu ends beyond contig %d", (unsigned long long)i, w.cn); return GM_E_ARG; }
    }
  }
  GmDevTurn dev_turn(s);     // (admitted like the mapping entries)
  GM_HIP(hipSetDevice(ix->device));
  hipStream_t q = s->stream;
  const int W = window_len_of(s->P, read_len);
  const int overlap_abs = (int)(unsigned int)(s->P.window_overlap < 0 ? -s->P.window_overlap : W * (s->P.window_overlap / 100.0));   // ref: mapping.c:1289
  GmDevMem mem;
  gm_read_window_t* d_wins = nullptr; unsigned long long *d_off = nullptr, *d_hit_off = nullptr; int* d_scores = nullptr; int32_t *d_sel_id = nullptr, *d_sel_score = nullptr;
  uint32_t* d_sel_cnt = nullptr; gm_pass1_hit_t *d_out = nullptr, *h_out = nullptr;
  const size_t nw = std::max<uint64_t>(n_wins, 1), slots = (size_t)n_reads * K;
  GM_HIP(mem.get(&d_wins, nw * sizeof(gm_read_window_t))); GM_HIP(mem.get(&d_off, ((size_t)2 * n_reads + 1) * 8)); GM_HIP(mem.get(&d_scores, nw * 4));
  GM_HIP(mem.get(&d_sel_id, slots * 4)); GM_HIP(mem.get(&d_sel_score, slots * 4));
  GM_HIP(mem.get(&d_sel_cnt, (size_t)n_reads * 4)); GM_HIP(mem.get(&d_hit_off, ((size_t)n_reads + 1) * 8));
  if (n_wins) {
    GM_HIP(hipMemcpyAsync(d_wins, wins, n_wins * sizeof(gm_read_window_t), hipMemcpyHostToDevice, q));
    GM_HIP(hipMemcpyAsync(d_scores, scores, n_wins * 4, hipMemcpyHostToDevice, q));
  }
  GM_HIP(hipMemcpyAsync(d_off, off, ((size_t)2 * n_reads + 1) * 8, hipMemcpyHostToDevice, q));
  int rc = gm_launch_sel_pass1(s->sc, n_reads, read_len, K, W, overlap_abs, d_wins, d_off, d_scores, d_sel_id, d_sel_score, d_sel_cnt, q);
  if (rc) return rc;
  rc = gm_launch_win_scan(d_sel_cnt, n_reads, GM_SEL_MAX, d_hit_off, q); if (rc) return rc;
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "offsets are copied as they are");
  GM_HIP(hipMemcpyAsync(hit_off, d_hit_off, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  const uint64_t total = hit_off[n_reads];
  if (total > (uint64_t)slots) { gm_set_error("gm_select_pass1: %llu hits in %zu slots", (unsigned long long)total, slots); hit_off[0] = 0; return GM_E_OVERFLOW; }
  if (total == 0) return GM_OK;
  GM_HIP(mem.get(&d_out, (size_t)total * sizeof(gm_pass1_hit_t)));
  h_out = mem.host<gm_pass1_hit_t>((size_t)total * sizeof(gm_pass1_hit_t));
  if (!h_out) { gm_set_error("gm_select_pass1: out of memory at %llu hits", (unsigned long long)total); return GM_E_NOMEM; }
  rc = gm_launch_sel_emit(s->sc, n_reads, read_len, K, d_wins, ix->d_contig_off, d_sel_id, d_sel_score, d_sel_cnt, d_hit_off, d_out, q);
  if (rc) return rc;
  GM_HIP(hipMemcpyAsync(h_out, d_out, (size_t)total * sizeof(gm_pass1_hit_t), hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  *hits = mem.give(h_out); *n_hits = total;
  return GM_OK;
}

extern "C" int gm_select_pass2(gm_session_t* s, int n_reads, const uint64_t* hit_off, const gm_pass1_hit_t* hits, const gm_sw_full_rec_t* recs, const gm_post_rec_t* post,
                               gm_mapping_t** maps, uint64_t* n_maps, uint64_t* map_off) {
  if (!s || !maps || !n_maps || !map_off) { gm_set_error("gm_select_pass2: bad arguments"); return GM_E_ARG; }
  *maps = nullptr; *n_maps = 0; map_off[0] = 0;
  if (n_reads <= 0) return GM_OK;
  if (!hit_off) { gm_set_error("gm_select_pass2: bad arguments"); return GM_E_ARG; }
  const gm_params_t& P = s->P; const gm_index* ix = s->ix;
  const bool mqv_on = gm_mqv_on(P), cs = P.colour_space != 0;
  if (hit_off[0] != 0) { gm_set_error("gm_select_pass2: the offsets start at %llu", (unsigned long long)hit_off[0]); return GM_E_ARG; }
  for (int r = 0; r < n_reads; r++) {
    if (hit_off[r + 1] < hit_off[r]) { gm_set_error("gm_select_pass2: offsets not ascending at read %d", r); return GM_E_ARG; }
    if (hit_off[r + 1] - hit_off[r] > GM_SEL_MAX) { gm_set_error("gm_select_pass2: read %d has %llu hits, beyond %d", r, (unsigned long long)(hit_off[r + 1] - hit_off[r]), GM_SEL_MAX); return GM_E_ARG; }
  }
  const uint64_t nh = hit_off[n_reads];
  if (nh && (!hits || !recs)) { gm_set_error("gm_select_pass2: bad arguments"); return GM_E_ARG; }
  if (nh && cs && mqv_on && !post) { gm_set_error("gm_select_pass2: a colour-space session with mapping qualities needs the answers of gm_post_sw_batch (post)"); return GM_E_ARG; }
  for (int r = 0; r < n_reads; r++) for (uint64_t i = hit_off[r]; i < hit_off[r + 1]; i++) {
    const gm_pass1_hit_t& h = hits[i];
    if (h.read != r) { gm_set_error("gm_select_pass2: hit %llu says read %d among the hits of read %d", (unsigned long long)i, h.read, r); return GM_E_ARG; }
    if (h.cn < 0 || h.cn >= ix->n_contigs || h.gen_st < 0 || h.gen_st > 1) { gm_set_error("gm_select_pass2: hit %llu: contig %d of %d, strand %d", (unsigned long long)i, h.cn, ix->n_contigs, h.gen_st); return GM_E_ARG; }
    if (h.score_max < 1) { gm_set_error("gm_select_pass2: hit %llu: score_max %d", (unsigned long long)i, h.score_max); return GM_E_ARG; }
  }
  for (int r = 0; r <= n_reads; r++) map_off[r] = 0;
  if (nh == 0) return GM_OK;
  // hit_run_post_sw per hit (ref: mapping.c:1609-1625), as HitScorer::post_sw (gm_host_finalize.inc)
  const double a = s->score_alpha, b = s->score_beta, tol = 1e-7;
  std::vector<GmSel2Item> items((size_t)nh);
  std::vector<double> posterior((size_t)nh, 0.0);
  std::vector<uint8_t> dev_post((size_t)nh, 0), near_read((size_t)n_reads, 0);
  for (int r = 0; r < n_reads; r++) for (uint64_t i = hit_off[r]; i < hit_off[r + 1]; i++) {
    const gm_pass1_hit_t& h = hits[i]; const gm_sw_full_rec_t& rec = recs[i];
    int sf = rec.status < 0 ? 0 : rec.score;
    if (sf > 0 && mqv_on) {
      if (cs) {
        if (post[i].status < 0) sf = 0;                                  // (a refused item counts as 0)
        else {
          posterior[i] = post[i].posterior; dev_post[i] = post[i].by_host ? 0 : 1;
          if (dev_post[i] && gm_near_rint(gm_post_score_x(a, b, posterior[i], rec.rmapped), tol)) near_read[r] = 1;      // AS at a rounding boundary
        }
      } else posterior[i] = gm_ls_posterior(a, b, rec.score, rec.rmapped);
      if (sf > 0) { int ps = gm_post_score(a, b, posterior[i], rec.rmapped); if (ps < 0) ps = 0; sf = ps; }
    }
    const int pct = (1000 * 100 * sf) / h.score_max;                     // ref: mapping.c:400-401
    GmSel2Item& it = items[i];
    it.grp = h.cn * 2 + h.gen_st; it.start = (int32_t)rec.genome_start;
    it.endkey = (int32_t)(-rec.genome_start - rec.rmapped + rec.deletions - rec.insertions);
    it.score_full = sf; it.key = P.sw_full_threshold < 0 ? sf : pct;
    it.keep = (double)sf >= gm_full_threshold(P, h.score_max) ? 1 : 0;  // ref: mapping.c:1661 (double compare)
  }
  std::vector<int32_t> order((size_t)nh); std::vector<uint32_t> cnt((size_t)n_reads);
  {
    GmDevTurn dev_turn(s);     // (admitted like the mapping entries)
    GM_HIP(hipSetDevice(ix->device));
    hipStream_t q = s->stream;
    GmDevMem mem;
    unsigned long long* d_off = nullptr; GmSel2Item* d_items = nullptr; int32_t* d_order = nullptr; uint32_t* d_cnt = nullptr;
    GM_HIP(mem.up(&d_off, hit_off, (size_t)n_reads + 1, q));
    GM_HIP(mem.up(&d_items, items.data(), (size_t)nh, q));
    GM_HIP(mem.get(&d_order, (size_t)nh * 4));
    GM_HIP(mem.get(&d_cnt, (size_t)n_reads * 4));
    int rc = gm_launch_sel_pass2(n_reads, P.num_outputs, P.strata ? 1 : 0, P.max_alignments, d_off, d_items, d_order, d_cnt, q);
    if (rc) return rc;
    GM_HIP(hipMemcpyAsync(order.data(), d_order, (size_t)nh * 4, hipMemcpyDeviceToHost, q));
    GM_HIP(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n_reads * 4, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
  }
  uint64_t total = 0;
  for (int r = 0; r < n_reads; r++) {
    if (cnt[r] > hit_off[r + 1] - hit_off[r]) { gm_set_error("gm_select_pass2: read %d: %u mappings of %llu hits", r, cnt[r], (unsigned long long)(hit_off[r + 1] - hit_off[r])); return GM_E_OVERFLOW; }
    total += cnt[r];
  }
  if (total == 0) return GM_OK;
  gm_mapping_t* out = (gm_mapping_t*)malloc((size_t)total * sizeof(gm_mapping_t));
  if (!out) { gm_set_error("gm_select_pass2: out of memory at %llu mappings", (unsigned long long)total); return GM_E_NOMEM; }
  uint64_t w = 0;
  for (int r = 0; r < n_reads; r++) {
    map_off[r] = w;
    const uint64_t base = hit_off[r]; const int m = (int)cnt[r];
    if (!m) continue;
    const uint64_t first = w;
    for (int k = 0; k < m; k++) {
      const uint64_t i = base + (uint64_t)order[base + k];
      gm_mapping_t& o = out[w++];
      o.read = r; o.hit = (int32_t)i; o.score_full = items[i].score_full; o.pct_score_full = (1000 * 100 * items[i].score_full) / hits[i].score_max;
      o.mqv = 255; o.flags = 0; o.posterior = posterior[i]; o.z0 = o.z1 = 0;
    }
    if (mqv_on) {                                                        // compute_unpaired_mqv, ref: output.c:777-793,975
      double z1 = 0.0;
      for (uint64_t k = first; k < w; k++) z1 += out[k].posterior;
      for (uint64_t k = first; k < w; k++) { out[k].z0 = out[k].posterior; out[k].z1 = z1; out[k].mqv = gm_unpaired_mqv(out[k].posterior, z1); }
      bool dev = false, near = near_read[r] != 0;
      for (uint64_t k = first; k < w; k++) dev = dev || dev_post[out[k].hit];
      if (dev) {                                                         // the rounding guard of the finalisation, made public
        near = near || gm_near_trunc(1000.0 * -log(z1), tol);
        for (uint64_t k = first; k < w; k++) near = near || gm_near_qv(out[k].posterior / z1, tol) || gm_near_trunc(1000.0 * -log(out[k].z0), tol);
      }
      if (near) for (uint64_t k = first; k < w; k++) if (dev_post[out[k].hit]) out[k].flags |= 1;
      if (P.single_best_mapping) {                                       // the first mapping with the highest quality, ref: output.c:977-984
        uint64_t mx = first;
        for (uint64_t k = first + 1; k < w; k++) if (out[k].mqv > out[mx].mqv) mx = k;
        out[first] = out[mx]; w = first + 1;
      }
    } else for (uint64_t k = first; k < w; k++) out[k].posterior = 0;
  }
  map_off[n_reads] = w;
  *maps = out; *n_maps = w;
  return GM_OK;
}
