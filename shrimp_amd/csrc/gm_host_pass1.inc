// gm_host_pass1.inc -- pass 1 as a seam: gm_score_windows (what f1_run computes for every window), gm_select_pass1_f1 (gm_select_pass1 with the f1 call cache) and
// gm_read_hits (reads to pass-1 hits in one call); part of gm_host.hip.
//
// gm_score_windows: the reads of the batch go up ONCE (packed, as the caller has them) beside the window records; k_score_windows fetches a window's read by its record.
// gm_select_pass1_f1: gm_select_pass1's copies plus the slots and an n_wins-word scratch for the computed (slot, score) pairs.
// gm_read_hits: per sub-batch gm_read_windows' front, heavy tier, counter read and capacity growth, the scan and the scatter, then k_score_windows on the set's own reads
// and the exported records, the selection and the emit: the hits and their offsets come down, the windows and their own scores only when asked for.
// The checks are made on the host before anything is uploaded.

// the read arguments, as gm_read_windows refuses them
static int pass1_reads_check(const char* who, const gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const uint8_t* initbp) {
  if (!reads_packed || read_len < 1) { gm_set_error("%s: bad arguments", who); return GM_E_ARG; }
  if ((s->P.colour_space != 0) != (initbp != nullptr)) {
    gm_set_error(s->P.colour_space ? "%s: a colour-space session needs the reads' primer letters (initbp)" : "%s: initbp given, but the session is not a colour-space one", who);
    return GM_E_ARG;
  }
  if (initbp) for (int i = 0; i < n_reads; i++) if (initbp[i] > 3) { gm_set_error("%s: read %d: primer letter code %d (the reference rejects such reads, fasta.c:636-645)", who, i, (int)initbp[i]); return GM_E_ARG; }
  if (read_len > s->P.longest_read_len || read_len >= 32768 / std::max(1, s->P.match_score)) { gm_set_error("%s: read length %d out of range (ref: sw-vector.c:393-398)", who, read_len); return GM_E_RANGE; }
  return GM_OK;
}

// the windows and their offsets, as gm_select_pass1 refuses them; *max_w: the longest window
static int pass1_windows_check(const char* who, const gm_session_t* s, int n_reads, const gm_read_window_t* wins, uint64_t n_wins, const uint64_t* off, int* max_w) {
  const gm_index* ix = s->ix;
  if (n_wins >= (1ull << 31)) { gm_set_error("%s: %llu windows (a hit names its window in 31 bits)", who, (unsigned long long)n_wins); return GM_E_RANGE; }
  if (off[0] != 0 || off[(size_t)2 * n_reads] != n_wins) { gm_set_error("%s: the offsets run from %llu to %llu, the windows from 0 to %llu", who, (unsigned long long)off[0], (unsigned long long)off[(size_t)2 * n_reads], (unsigned long long)n_wins); return GM_E_ARG; }
  for (size_t rs = 0; rs < (size_t)2 * n_reads; rs++)
    if (off[rs + 1] < off[rs] || off[rs + 1] > n_wins) { gm_set_error("%s: offsets not ascending at read %zu strand %zu", who, rs >> 1, rs & 1); return GM_E_ARG; }
  int mw = 1;
  for (size_t rs = 0; rs < (size_t)2 * n_reads; rs++) {
    for (uint64_t i = off[rs]; i < off[rs + 1]; i++) {
      const gm_read_window_t& w = wins[i];
      if (w.read != (int32_t)(rs >> 1) || w.st != (int32_t)(rs & 1)) { gm_set_error("%s: window %llu says read %d strand %d in the list of read %zu strand %zu", who, (unsigned long long)i, w.read, w.st, rs >> 1, rs & 1); return GM_E_ARG; }
      if (w.cn < 0 || w.cn >= ix->n_contigs) { gm_set_error("%s: window %llu: contig %d of %d", who, (unsigned long long)i, w.cn, ix->n_contigs); return GM_E_ARG; }
      if (w.w_len < 1) { gm_set_error("%s: window %llu: w_len %d", who, (unsigned long long)i, w.w_len); return GM_E_ARG; }
      if ((uint64_t)w.g_off + (uint64_t)w.w_len > (uint64_t)(ix->contig_off[w.cn + 1] - ix->contig_off[w.cn])) { gm_set_error("%s: window %llu ends beyond contig %d", who, (unsigned long long)i, w.cn); return GM_E_ARG; }
      mw = std::max(mw, (int)w.w_len);
    }
  }
  if (max_w) *max_w = mw;
  return GM_OK;
}

extern "C" int gm_score_windows(gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const uint8_t* initbp, const gm_read_window_t* wins, uint64_t n_wins,
                                const uint64_t* off, int* scores, uint32_t* slots) {
  if (!s) { gm_set_error("gm_score_windows: bad arguments"); return GM_E_ARG; }
  if (n_reads <= 0) return GM_OK;
  if (!off || (n_wins && (!wins || !scores))) { gm_set_error("gm_score_windows: bad arguments"); return GM_E_ARG; }
  if (int rc = pass1_reads_check("gm_score_windows", s, n_reads, read_len, reads_packed, initbp)) return rc;
  int max_w = 1;
  if (int rc = pass1_windows_check("gm_score_windows", s, n_reads, wins, n_wins, off, &max_w)) return rc;
  if (n_wins == 0) return GM_OK;
  const bool cs = s->P.colour_space != 0;
  if (gm_score_windows_lds(cs, read_len, max_w) > GM_SCORE_WIN_LDS_LIMIT) { gm_set_error("gm_score_windows: a window of %d positions beside reads of %d is beyond the kernel's LDS", max_w, read_len); return GM_E_RANGE; }
  GmDevTurn dev_turn(s);     // (admitted like the mapping entries)
  GM_HIP(hipSetDevice(s->ix->device));
  hipStream_t q = s->stream;
  const int read_words = (read_len + 7) / 8;
  GmDevMem mem;
  uint32_t *d_reads = nullptr, *d_slots = nullptr; uint8_t *d_initbp = nullptr, *d_rna = nullptr; gm_read_window_t* d_wins = nullptr; int* d_scores = nullptr;
  GM_HIP(mem.up(&d_reads, reads_packed, (size_t)n_reads * read_words, q, 256));
  if (cs) GM_HIP(mem.up(&d_initbp, initbp, (size_t)n_reads, q));
  GM_HIP(mem.up(&d_wins, wins, (size_t)n_wins, q));
  GM_HIP(mem.get(&d_scores, (size_t)n_wins * 4));
  if (slots) GM_HIP(mem.get(&d_slots, (size_t)n_wins * 4));
  GmIndexDev view = session_view(s);
  if (!cs) {                                                             // the reads' own RNA flags, as the pipeline makes them
    GM_HIP(mem.get(&d_rna, (size_t)n_reads + 64));
    if (int rc = gm_launch_read_rna_flags(d_reads, n_reads, read_len, read_words, d_rna, q)) return rc;
    view.read_rna = d_rna;
  }
  if (int rc = gm_launch_score_windows(view, s->sc, n_wins, d_wins, d_reads, read_len, read_words, 0, d_initbp, max_w, d_scores, d_slots, nullptr, q)) return rc;
  GM_HIP(hipMemcpyAsync(scores, d_scores, (size_t)n_wins * 4, hipMemcpyDeviceToHost, q));
  if (slots) GM_HIP(hipMemcpyAsync(slots, d_slots, (size_t)n_wins * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  return GM_OK;
}

// The selection on arrays that are on the device already: n_reads reads, their windows d_wins[0 .. n_wins) with the offsets d_off[2 n_reads + 1], the scores and (or
// null: no cache) the slots.  hit_off[n_reads + 1] (host) receives the offsets, *d_out the records (mem's; null when there are none), *bypassed the cache's count.
static int pass1_select_device(const char* who, gm_session_t* s, GmDevMem& mem, int n_reads, int read_len, const gm_read_window_t* d_wins, uint64_t n_wins,
                               const unsigned long long* d_off, const int* d_scores, const uint32_t* d_slots, uint64_t* hit_off, gm_pass1_hit_t** d_out, uint64_t* total,
                               uint64_t* bypassed) {
  const int K = s->P.num_tmp_outputs;
  hipStream_t q = s->stream;
  const int W = window_len_of(s->P, read_len);
  const int overlap_abs = (int)(unsigned int)(s->P.window_overlap < 0 ? -s->P.window_overlap : W * (s->P.window_overlap / 100.0));   // ref: mapping.c:1289
  int32_t *d_sel_id = nullptr, *d_sel_score = nullptr; uint32_t *d_sel_cnt = nullptr, *d_byp = nullptr; unsigned long long *d_hit_off = nullptr, *d_comp = nullptr;
  const size_t slots = (size_t)n_reads * K;
  *d_out = nullptr; *total = 0; *bypassed = 0;
  GM_HIP(mem.get(&d_sel_id, slots * 4)); GM_HIP(mem.get(&d_sel_score, slots * 4));
  GM_HIP(mem.get(&d_sel_cnt, (size_t)n_reads * 4)); GM_HIP(mem.get(&d_hit_off, ((size_t)n_reads + 1) * 8));
  std::vector<uint32_t> byp;
  int rc;
  if (d_slots) {
    GM_HIP(mem.get(&d_comp, std::max<uint64_t>(n_wins, 1) * 8)); GM_HIP(mem.get(&d_byp, (size_t)n_reads * 4));
    rc = gm_launch_sel_pass1_f1(s->sc, n_reads, read_len, K, W, overlap_abs, d_wins, d_off, d_scores, d_slots, d_comp, d_sel_id, d_sel_score, d_sel_cnt, d_byp, q);
  } else rc = gm_launch_sel_pass1(s->sc, n_reads, read_len, K, W, overlap_abs, d_wins, d_off, d_scores, d_sel_id, d_sel_score, d_sel_cnt, q);
  if (rc) return rc;
  rc = gm_launch_win_scan(d_sel_cnt, n_reads, GM_SEL_MAX, d_hit_off, q); if (rc) return rc;
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "offsets are copied as they are");
  GM_HIP(hipMemcpyAsync(hit_off, d_hit_off, ((size_t)n_reads + 1) * 8, hipMemcpyDeviceToHost, q));
  if (d_slots) { byp.resize((size_t)n_reads); GM_HIP(hipMemcpyAsync(byp.data(), d_byp, (size_t)n_reads * 4, hipMemcpyDeviceToHost, q)); }
  GM_HIP(hipStreamSynchronize(q));
  for (uint32_t b : byp) *bypassed += b;
  const uint64_t t = hit_off[n_reads];
  if (t > (uint64_t)slots) { gm_set_error("%s: %llu hits in %zu slots", who, (unsigned long long)t, slots); return GM_E_OVERFLOW; }
  if (t == 0) return GM_OK;
  GM_HIP(mem.get(d_out, (size_t)t * sizeof(gm_pass1_hit_t)));
  rc = gm_launch_sel_emit(s->sc, n_reads, read_len, K, d_wins, s->ix->d_contig_off, d_sel_id, d_sel_score, d_sel_cnt, d_hit_off, *d_out, q);
  if (rc) return rc;
  *total = t;
  return GM_OK;
}

// num_tmp_outputs as the selection entries refuse it
static int pass1_k_check(const char* who, const gm_session_t* s) {
  const int K = s->P.num_tmp_outputs;
  if (K > GM_SEL_MAX) { gm_set_error("%s: num_tmp_outputs %d is beyond the %d hits a read this entry selects", who, K, GM_SEL_MAX); return GM_E_RANGE; }
  if (K < 1) { gm_set_error("%s: num_tmp_outputs %d", who, K); return GM_E_ARG; }
  return GM_OK;
}

extern "C" int gm_select_pass1_f1(gm_session_t* s, int n_reads, int read_len, const gm_read_window_t* wins, uint64_t n_wins, const uint64_t* off, const int* scores,
                                  const uint32_t* slots, gm_pass1_hit_t** hits, uint64_t* n_hits, uint64_t* hit_off, uint64_t* bypassed) {
  if (bypassed) *bypassed = 0;
  if (!slots) return gm_select_pass1(s, n_reads, read_len, wins, n_wins, off, scores, hits, n_hits, hit_off);      // no cache: that entry, bit for bit
  if (!s || !hits || !n_hits || !hit_off) { gm_set_error("gm_select_pass1_f1: bad arguments"); return GM_E_ARG; }
  *hits = nullptr; *n_hits = 0; hit_off[0] = 0;
  if (n_reads <= 0) return GM_OK;
  if (!off || read_len < 1 || (n_wins && (!wins || !scores))) { gm_set_error("gm_select_pass1_f1: bad arguments"); return GM_E_ARG; }
  if (int rc = pass1_k_check("gm_select_pass1_f1", s)) return rc;
  if (int rc = pass1_windows_check("gm_select_pass1_f1", s, n_reads, wins, n_wins, off, nullptr)) return rc;
  GmDevTurn dev_turn(s);     // (admitted like the mapping entries)
  GM_HIP(hipSetDevice(s->ix->device));
  hipStream_t q = s->stream;
  GmDevMem mem;
  gm_read_window_t* d_wins = nullptr; unsigned long long* d_off = nullptr; int* d_scores = nullptr; uint32_t* d_slots = nullptr;
  const size_t nw = std::max<uint64_t>(n_wins, 1);
  GM_HIP(mem.get(&d_wins, nw * sizeof(gm_read_window_t))); GM_HIP(mem.get(&d_off, ((size_t)2 * n_reads + 1) * 8)); GM_HIP(mem.get(&d_scores, nw * 4)); GM_HIP(mem.get(&d_slots, nw * 4));
  if (n_wins) {
    GM_HIP(hipMemcpyAsync(d_wins, wins, n_wins * sizeof(gm_read_window_t), hipMemcpyHostToDevice, q));
    GM_HIP(hipMemcpyAsync(d_scores, scores, n_wins * 4, hipMemcpyHostToDevice, q));
    GM_HIP(hipMemcpyAsync(d_slots, slots, n_wins * 4, hipMemcpyHostToDevice, q));
  }
  GM_HIP(hipMemcpyAsync(d_off, off, ((size_t)2 * n_reads + 1) * 8, hipMemcpyHostToDevice, q));
  gm_pass1_hit_t* d_out = nullptr; uint64_t total = 0, byp = 0;
  const int rc = pass1_select_device("gm_select_pass1_f1", s, mem, n_reads, read_len, d_wins, n_wins, d_off, d_scores, d_slots, hit_off, &d_out, &total, &byp);
  if (rc) { hit_off[0] = 0; return rc; }
  if (bypassed) *bypassed = byp;
  if (total == 0) return GM_OK;
  gm_pass1_hit_t* h_out = mem.host<gm_pass1_hit_t>((size_t)total * sizeof(gm_pass1_hit_t));
  if (!h_out) { gm_set_error("gm_select_pass1_f1: out of memory at %llu hits", (unsigned long long)total); hit_off[0] = 0; return GM_E_NOMEM; }
  GM_HIP(hipMemcpyAsync(h_out, d_out, (size_t)total * sizeof(gm_pass1_hit_t), hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  *hits = mem.give(h_out); *n_hits = total;
  return GM_OK;
}

// One sub-batch of read_hits_impl while its hits are still on the device: reads [base, base + n) of the call are rows 0 .. n of D->d_reads, their nh hits d_hits (and
// h_hits, the same records on the host) with the offsets hit_off[n + 1], all counted within the sub-batch but for the records' own `read` (the call's); hits_before:
// the hits of the sub-batches before it.  gm_read_mappings runs pass 2 from here; a non-zero return ends the call with that code.
struct Pass1Batch { int base, n; DevSet* D; const gm_pass1_hit_t* d_hits; const gm_pass1_hit_t* h_hits; uint64_t nh, hits_before; const uint64_t* hit_off; };
typedef int (*pass1_batch_fn)(void* ctx, const Pass1Batch& b);

// gm_read_hits (who names the entry in messages; after: null there)
static int read_hits_impl(const char* who, gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const uint8_t* initbp, gm_pass1_hit_t** hits, uint64_t* n_hits,
                          uint64_t* hit_off, gm_read_window_t** wins, uint64_t* n_wins, uint64_t* off, int** scores, gm_map_stats_t* stats, pass1_batch_fn after, void* after_ctx) {
  if (!s || !hits || !n_hits || !hit_off) { gm_set_error("%s: bad arguments", who); return GM_E_ARG; }
  const int n_opt = (wins ? 1 : 0) + (n_wins ? 1 : 0) + (off ? 1 : 0) + (scores ? 1 : 0);
  if (n_opt != 0 && n_opt != 4) { gm_set_error("%s: wins, n_wins, off and scores are given together or not at all (%d of the four are)", who, n_opt); return GM_E_ARG; }
  const bool want = n_opt == 4;
  *hits = nullptr; *n_hits = 0; hit_off[0] = 0;
  if (want) { *wins = nullptr; *n_wins = 0; off[0] = 0; *scores = nullptr; }
  if (stats) memset(stats, 0, sizeof *stats);
  if (n_reads <= 0) return GM_OK;
  if (int rc = pass1_reads_check(who, s, n_reads, read_len, reads_packed, initbp)) return rc;
  if (int rc = pass1_k_check(who, s)) return rc;
  const int W = window_len_of(s->P, read_len);
  const bool cs = s->P.colour_space != 0, cache = s->P.hash_filter_calls != 0;
  if (gm_score_windows_lds(cs, read_len, W) > GM_SCORE_WIN_LDS_LIMIT) { gm_set_error("%s: windows of %d positions beside reads of %d are beyond the scoring kernel's LDS", who, W, read_len); return GM_E_RANGE; }
  GmDevTurn dev_turn(s);     // (admitted like the mapping entries)
  GM_HIP(hipSetDevice(s->ix->device));
  DevSet& D = s->set[0];
  if (int rc = prepare_unpaired_set(s, read_len)) return rc;
  const int read_words = (read_len + 7) / 8;
  hipStream_t q = s->stream;
  unsigned long long* d_stats = s->d_pstats[0];
  GmDevMem mem;                        // the offsets, the records and the scores on the device and the results of the call so far on the host, each grown on demand
  unsigned long long* d_off = nullptr; gm_read_window_t *d_out = nullptr, *h = nullptr; int *d_scores = nullptr, *h_sc = nullptr; uint32_t* d_slots = nullptr;
  gm_pass1_hit_t* h_hits = nullptr; size_t off_cap = 0, out_cap = 0, h_cap = 0, hits_cap = 0;
  std::vector<unsigned long long> hraw((size_t)GS_STRIPES * GS_STRIDE), hoff;
  std::vector<uint64_t> hho;
  uint64_t total = 0, total_hits = 0;
  int base = 0;
  while (base < n_reads) {
    const int n = std::min(n_reads - base, D.eff_batch);
    GM_HIP(hipMemcpyAsync(D.d_reads, reads_packed + (size_t)base * read_words, (size_t)n * read_words * 4, hipMemcpyHostToDevice, q));
    if (initbp) GM_HIP(hipMemcpyAsync(D.d_initbp, initbp + base, (size_t)n, hipMemcpyHostToDevice, q));
    int rc = pipeline_front(s, 0, n, read_len); if (rc) return rc;
    GM_HIP(hipEventSynchronize(s->pev[0][6]));
    const uint32_t n_heavy = s->h_pin[0];
    float ms[2];
    GM_HIP(hipEventElapsedTime(&ms[0], s->pev[0][0], s->pev[0][1]));
    GM_HIP(hipEventElapsedTime(&ms[1], s->pev[0][1], s->pev[0][2]));
    if (n_heavy) { rc = run_heavy_tier(s, D, session_view(s), n, read_len, read_words, W, (int)n_heavy, d_stats); if (rc) return rc; }
    // the stage counters first: d_hit_cnt of a row that overflowed is larger than the row
    unsigned long long hs[GS_N];
    GM_HIP(hipMemcpyAsync(hraw.data(), d_stats, hraw.size() * 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    fold_stats(hraw.data(), hs);
    if (hs[GS_OVERFLOW_SURV]) { gm_set_error("heavy list overflow"); return GM_E_OVERFLOW; }
    if (hs[GS_OVERFLOW_HITS]) {      // as gm_read_windows: a larger row, new buffers, the sub-batch again from the upload
      if (D.hcap >= 32768) { gm_set_error("window list overflow at capacity %d", D.hcap); return GM_E_OVERFLOW; }
      D.hcap *= 4;
      if (stats) stats->retries++;
      rc = alloc_buffers(s, D, read_len); if (rc) return rc;
      continue;
    }
    const int n_rs = 2 * n;
    if ((size_t)n_rs + 1 > off_cap) {
      mem.drop(d_off); off_cap = (size_t)2 * std::max(n, D.eff_batch) + 1;
      GM_HIP(mem.get(&d_off, off_cap * 8));
    }
    rc = gm_launch_win_scan(D.d_hit_cnt, n_rs, D.hcap, d_off, q); if (rc) return rc;
    unsigned long long t = 0;
    GM_HIP(hipMemcpyAsync(&t, d_off + n_rs, 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    if (total + t >= (1ull << 31)) { gm_set_error("%s: %llu windows (a hit names its window in 31 bits)", who, (unsigned long long)(total + t)); return GM_E_RANGE; }
    if (t > out_cap || !d_out) {
      mem.drop(d_out); mem.drop(d_scores); mem.drop(d_slots); out_cap = std::max<size_t>((size_t)t, 1);
      GM_HIP(mem.get(&d_out, out_cap * sizeof(gm_read_window_t))); GM_HIP(mem.get(&d_scores, out_cap * 4));
      if (cache) GM_HIP(mem.get(&d_slots, out_cap * 4));
    }
    rc = gm_launch_win_scatter(D.d_hits, D.d_perm, d_off, n_rs, D.hcap, t, base, d_out, q); if (rc) return rc;
    // the scores (and slots) of the exported records against the set's own reads: row `read - base` of D.d_reads, the RNA flags pipeline_front left for them
    rc = gm_launch_score_windows(session_view(s, &D), s->sc, t, d_out, D.d_reads, read_len, read_words, base, initbp ? D.d_initbp : nullptr, W, d_scores, d_slots, d_stats, q);
    if (rc) return rc;
    hho.resize((size_t)n + 1);
    gm_pass1_hit_t* d_hits = nullptr; uint64_t nh = 0, byp = 0;
    {
      GmDevMem sel;                    // the selection's scratch and records of this sub-batch
      rc = pass1_select_device(who, s, sel, n, read_len, d_out, t, d_off, d_scores, d_slots, hho.data(), &d_hits, &nh, &byp); if (rc) return rc;
      if (total_hits + nh > hits_cap) {
        const size_t cap = std::max<size_t>((size_t)(total_hits + nh), hits_cap + hits_cap / 2);
        gm_pass1_hit_t* p = mem.host(cap * sizeof(gm_pass1_hit_t), false, h_hits);
        if (!p) { gm_set_error("%s: out of memory at %zu hits", who, cap); return GM_E_NOMEM; }
        h_hits = p; hits_cap = cap;
      }
      if (nh) GM_HIP(hipMemcpyAsync(h_hits + total_hits, d_hits, (size_t)nh * sizeof(gm_pass1_hit_t), hipMemcpyDeviceToHost, q));
      if (want) {
        if (total + t > h_cap) {
          const size_t cap = std::max<size_t>((size_t)(total + t), h_cap + h_cap / 2);
          gm_read_window_t* p = mem.host(cap * sizeof(gm_read_window_t), false, h);
          if (!p) { gm_set_error("%s: out of memory at %zu windows", who, cap); return GM_E_NOMEM; }
          h = p;
          int* ps = mem.host(cap * sizeof(int), false, h_sc);
          if (!ps) { gm_set_error("%s: out of memory at %zu windows", who, cap); return GM_E_NOMEM; }
          h_sc = ps; h_cap = cap;
        }
        hoff.resize((size_t)n_rs + 1);
        if (t) {
          GM_HIP(hipMemcpyAsync(h + total, d_out, (size_t)t * sizeof(gm_read_window_t), hipMemcpyDeviceToHost, q));
          GM_HIP(hipMemcpyAsync(h_sc + total, d_scores, (size_t)t * 4, hipMemcpyDeviceToHost, q));
        }
        GM_HIP(hipMemcpyAsync(hoff.data(), d_off, hoff.size() * 8, hipMemcpyDeviceToHost, q));
      }
      if (stats) GM_HIP(hipMemcpyAsync(hraw.data(), d_stats, hraw.size() * 8, hipMemcpyDeviceToHost, q));      // again: the scoring kernel's counters
      GM_HIP(hipStreamSynchronize(q));
      if (after) {
        Pass1Batch pb; pb.base = base; pb.n = n; pb.D = &D; pb.d_hits = d_hits; pb.h_hits = h_hits + total_hits; pb.nh = nh; pb.hits_before = total_hits; pb.hit_off = hho.data();
        rc = after(after_ctx, pb); if (rc) return rc;
      }
    }
    for (uint64_t k = 0; k < nh; k++) h_hits[total_hits + k].win += (int32_t)total;      // window indices and offsets are the call's, not the sub-batch's
    for (int r = 0; r <= n; r++) hit_off[(size_t)base + r] = total_hits + hho[r];
    if (want) for (int i = 0; i <= n_rs; i++) off[(size_t)2 * base + i] = total + hoff[i];
    if (stats) {
      unsigned long long hv[GS_N]; fold_stats(hraw.data(), hv);
      stats->reads += (uint64_t)n;
      stats->lookups += hs[GS_LOOKUPS]; stats->list_entries += hs[GS_ENTRIES]; stats->list_bytes += 12ull * hs[GS_LOOKUPS] + 4ull * hs[GS_ENTRIES];
      stats->survivors += hs[GS_SURVIVORS]; stats->anchors += hs[GS_ANCHORS]; stats->windows += t;
      stats->exact_order_reads += hs[GS_EXACT_ORDER]; stats->survivors_pruned += hs[GS_PRUNED];
      stats->vec_calls += hv[GS_VEC_CALLS]; stats->vec_cells += hv[GS_VEC_CELLS]; stats->vec_bypassed += byp;
      stats->ms_lookup += ms[0]; stats->ms_anchors += ms[1];
    }
    total += t; total_hits += nh;
    base += n;
  }
  if (total_hits) *hits = mem.give(h_hits);
  *n_hits = total_hits;
  if (want) {
    if (total) { *wins = mem.give(h); *scores = mem.give(h_sc); }
    *n_wins = total;
  }
  return GM_OK;
}
extern "C" int gm_read_hits(gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const uint8_t* initbp, gm_pass1_hit_t** hits, uint64_t* n_hits,
                            uint64_t* hit_off, gm_read_window_t** wins, uint64_t* n_wins, uint64_t* off, int** scores, gm_map_stats_t* stats) {
  return read_hits_impl("gm_read_hits", s, n_reads, read_len, reads_packed, initbp, hits, n_hits, hit_off, wins, n_wins, off, scores, stats, nullptr, nullptr);
}
