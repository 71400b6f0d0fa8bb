// gm_host_windows.inc -- gm_read_windows: the front of the pipeline (K1, K1b, K2) as a public seam; part of gm_host.hip.
//
// Per sub-batch: the reads go up, pipeline_front runs on set 0, the heavy tier follows where K1 listed read-strands for it (as BackStages::wait_front does), the stage
// counters are read BEFORE anything looks at d_hits (a window list that overflowed grows hcap x4 and the sub-batch is redone from the upload), and only then the counts are
// scanned and the windows exported (gm_windows.hip).  What crosses the bus: the counters, the scan's total (8 bytes), the 2 n + 1 offsets and the tight records --
// nothing is sized by hcap.

extern "C" int gm_read_window_size(void) { return (int)sizeof(gm_read_window_t); }

extern "C" int gm_read_windows(gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const uint8_t* initbp,
                               gm_read_window_t** wins, uint64_t* n_wins, uint64_t* off, gm_map_stats_t* stats) {
  if (!s || !wins || !n_wins || !off) { gm_set_error("gm_read_windows: bad arguments"); return GM_E_ARG; }
  *wins = nullptr; *n_wins = 0; off[0] = 0;
  if (stats) memset(stats, 0, sizeof *stats);
  if (n_reads <= 0) return GM_OK;
  if (!reads_packed || read_len < 1) { gm_set_error("gm_read_windows: bad arguments"); return GM_E_ARG; }
  if ((s->P.colour_space != 0) != (initbp != nullptr)) {
    gm_set_error(s->P.colour_space ? "gm_read_windows: a colour-space session needs the reads' primer letters (initbp)" : "gm_read_windows: initbp given, but the session is not a colour-space one");
    return GM_E_ARG;
  }
  if (initbp) for (int i = 0; i < n_reads; i++) if (initbp[i] > 3) { gm_set_error("gm_read_windows: read %d: primer letter code %d (the reference rejects such reads, fasta.c:636-645)", i, (int)initbp[i]); return GM_E_ARG; }
  if (read_len > s->P.longest_read_len || read_len >= 32768 / std::max(1, s->P.match_score)) { gm_set_error("gm_read_windows: read length %d out of range (ref: sw-vector.c:393-398)", read_len); return GM_E_RANGE; }
  GmDevTurn dev_turn(s);     // (admitted like the mapping entries)
  GM_HIP(hipSetDevice(s->ix->device));
  DevSet& D = s->set[0];
  if (int rc = prepare_unpaired_set(s, read_len)) return rc;
  const int read_words = (read_len + 7) / 8;
  const int W = window_len_of(s->P, read_len);
  hipStream_t q = s->stream;
  unsigned long long* d_stats = s->d_pstats[0];
  GmDevMem mem;                        // the offsets, the records on the device and the records of the call so far on the host, each grown on demand
  unsigned long long* d_off = nullptr; gm_read_window_t *d_out = nullptr, *h = nullptr; size_t off_cap = 0, out_cap = 0, h_cap = 0;
  std::vector<unsigned long long> hraw((size_t)GS_STRIPES * GS_STRIDE), hoff;
  uint64_t total = 0;
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
    if (hs[GS_OVERFLOW_HITS]) {      // as BackStages::grow: a larger row, new buffers, the sub-batch again from the upload (fewer reads of it if the sub-batch size shrank)
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
    if (t > out_cap) {
      mem.drop(d_out); out_cap = (size_t)t;
      GM_HIP(mem.get(&d_out, out_cap * sizeof(gm_read_window_t)));
    }
    if (total + t > h_cap) {
      const size_t cap = std::max<size_t>((size_t)(total + t), h_cap + h_cap / 2);
      gm_read_window_t* p = mem.host(cap * sizeof(gm_read_window_t), false, h);
      if (!p) { gm_set_error("gm_read_windows: out of memory at %zu windows", cap); return GM_E_NOMEM; }
      h = p; h_cap = cap;
    }
    rc = gm_launch_win_scatter(D.d_hits, D.d_perm, d_off, n_rs, D.hcap, t, base, d_out, q); if (rc) return rc;
    hoff.resize((size_t)n_rs + 1);
    if (t) GM_HIP(hipMemcpyAsync(h + total, d_out, (size_t)t * sizeof(gm_read_window_t), hipMemcpyDeviceToHost, q));
    GM_HIP(hipMemcpyAsync(hoff.data(), d_off, hoff.size() * 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    for (int i = 0; i <= n_rs; i++) off[(size_t)2 * base + i] = total + hoff[i];
    total += t;
    if (stats) {
      stats->reads += (uint64_t)n;
      stats->lookups += hs[GS_LOOKUPS]; stats->list_entries += hs[GS_ENTRIES]; stats->list_bytes += 12ull * hs[GS_LOOKUPS] + 4ull * hs[GS_ENTRIES];
      stats->survivors += hs[GS_SURVIVORS]; stats->anchors += hs[GS_ANCHORS]; stats->windows += t;      // (t == K2's own GS_WINDOWS: both sum min(hit_cnt, hcap))
      stats->exact_order_reads += hs[GS_EXACT_ORDER]; stats->survivors_pruned += hs[GS_PRUNED];
      stats->ms_lookup += ms[0]; stats->ms_anchors += ms[1];
    }
    base += n;
  }
  if (total) *wins = mem.give(h);
  *n_wins = total;
  return GM_OK;
}
