// gm_host_pairs.inc -- host side of paired mode; included by gm_host.hip (same translation unit, after map_impl).
//   handle_readpair            ref: gmapper/mapping.c:2502-2636     readpair_pass2          ref: mapping.c:2181-2314
//   readpair_save_final_hits   ref: mapping.c:2446-2499             compute_paired_mqv      ref: output.c:811-942
//   readpair_output            ref: output.c:1070-1291              hit_output: sam_record with a mate (gm_host_records.inc)
// Device work per sub-batch of pairs: K1/K2 per mate set, pair-up, pass 1 over paired windows, pair top-K,
// pass 2 at half threshold; host: pair selection; device: the half-paired fall-back (pass 1 over all windows,
// top-K, pass 2); host: selection, paired mapping qualities, SAM text.

extern "C" void gm_pair_opts_default(gm_pair_opts_t* o) {
  if (!o) return;
  o->pair_mode = GM_PAIR_OPP_IN; o->min_insert_size = 0; o->max_insert_size = 1000;
  o->insert_size_mean = 200; o->insert_size_stddev = 100; o->half_paired = 1; o->match_mode = 4;
}

struct PPair {                    // struct read_hit_pair (ref: gmapper-definitions.h:162-173); h[] index the pair's per-mate window arrays
  int h[2]; int score_max, score, pct_score, key, insert_size;
};

struct PairCtx {
  const gm_session* s; gm_pair_opts_t O; int len[2], rwords[2]; double total_genome_size;
};

static int get_insert_size(const gm_index* ix, const FHit* rh, const FHit* rh_mp) {    // ref: mapping.c:405-456
  if (rh->r->cn != rh_mp->r->cn) return 0;
  int gs_mp, ge_mp, gs, ge; hit_ends(ix->contig_off, rh_mp, &gs_mp, &ge_mp); hit_ends(ix->contig_off, rh, &gs, &ge);
  const int fivep = (rh->r->gen_st == 1) ? ge : gs - 1;
  const int fivep_mp = (rh_mp->r->gen_st == 1) ? ge_mp : gs_mp - 1;
  return fivep_mp - fivep;
}
static void compute_paired_hit(const PairCtx& C, FHit* const H[2], PPair& d) {          // ref: mapping.c:2053-2080
  const FHit* a = &H[0][d.h[0]]; const FHit* b = &H[1][d.h[1]];
  d.score_max = a->r->score_max + b->r->score_max;
  d.score = a->score_full + b->score_full;
  d.pct_score = (1000 * 100 * d.score) / d.score_max;
  d.key = C.s->P.sw_full_threshold < 0 ? d.score : d.pct_score;
  const int ins = get_insert_size(C.s->ix, a, b);
  int sign;
  if (C.O.pair_mode == GM_PAIR_OPP_IN || C.O.pair_mode == GM_PAIR_COL_FW) sign = (a->r->gen_st == 0) ? +1 : -1;
  else sign = (a->r->gen_st == 1) ? +1 : -1;
  d.insert_size = sign * ins;
}
template <class Cmp>
static void push_dominant(const PairCtx& C, FHit* const H[2], std::vector<PPair>& v, int nip, Cmp cmp) {   // ref: mapping.c:2083-2110
  gm_small_stable_sort(v.begin(), v.end(), [&](const PPair& a, const PPair& b) { return cmp(&H[nip][a.h[nip]], &H[nip][b.h[nip]]) < 0; });
  size_t i = 0; const size_t n = v.size();
  while (i < n) {
    int mx = H[nip][v[i].h[nip]].score_full; size_t mi = i, j = i + 1;
    while (j < n && !cmp(&H[nip][v[i].h[nip]], &H[nip][v[j].h[nip]])) { if (H[nip][v[j].h[nip]].score_full > mx) { mx = H[nip][v[j].h[nip]].score_full; mi = j; } j++; }
    for (size_t k = i; k < j; k++) if (k != mi) { v[k].h[nip] = v[mi].h[nip]; compute_paired_hit(C, H, v[k]); }
    i = j;
  }
}

// readpair_pass2 after the device has aligned every window of the selected pairs (ref: mapping.c:2181-2314).
// plist[k] = (a << 8) | b in ext-heap array order; v = final pairs in output order.
static void pair_pass2(const PairCtx& C, FHit* const H[2], const uint32_t* plist, int np, std::vector<PPair>& v) {
  const gm_params_t& P = C.s->P;
  v.clear();
  for (int k = 0; k < np; k++) {
    PPair d; d.h[0] = (int)(plist[k] >> 8); d.h[1] = (int)(plist[k] & 0xff);
    const FHit& a = H[0][d.h[0]]; const FHit& b = H[1][d.h[1]];
    if (a.score_full == 0 || b.score_full == 0) continue;                                        // ref :2243-2245
    const int smax = a.r->score_max + b.r->score_max;
    const int thr = P.sw_full_threshold < 0 ? (int)(-P.sw_full_threshold) : (int)(smax * (P.sw_full_threshold / 100.0));
    if (a.score_full + b.score_full >= thr) { compute_paired_hit(C, H, d); v.push_back(d); }
  }
  // readpair_remove_duplicate_hits, ref: mapping.c:2113-2175
  push_dominant(C, H, v, 0, cmp_gen_start); push_dominant(C, H, v, 0, cmp_gen_end);
  push_dominant(C, H, v, 1, cmp_gen_start); push_dominant(C, H, v, 1, cmp_gen_end);
  auto pcmp = [&](const PPair& x, const PPair& y) {                                              // ref: mapping.c:2004-2050
    const int a0 = H[0][x.h[0]].r->sort_idx, b0 = H[0][y.h[0]].r->sort_idx;
    if (a0 != b0) return a0 - b0;
    return H[1][x.h[1]].r->sort_idx - H[1][y.h[1]].r->sort_idx;
  };
  gm_small_stable_sort(v.begin(), v.end(), [&](const PPair& x, const PPair& y) { return pcmp(x, y) < 0; });
  { size_t m = 0, i = 0; const size_t n = v.size();                                               // removedups, ref: common/util.c:1240-1255
    while (i < n) { size_t j = i + 1; while (j < n && !pcmp(v[i], v[j])) j++; if (m < i) v[m] = v[i]; m++; i = j; }
    v.resize(m); }
  gm_small_stable_sort(v.begin(), v.end(), [](const PPair& x, const PPair& y) { return (y.key - x.key) < 0; });
  if ((int)v.size() > P.num_outputs) v.resize(P.num_outputs);
  if (P.strata && !v.empty()) { size_t i = 1; while (i < v.size() && v[0].score == v[i].score) i++; v.resize(i); }      // ref: mapping.c:2268-2274
  if (P.max_alignments != 0 && (int)v.size() > P.max_alignments) v.clear();                                             // ref: mapping.c:2275-2284
}

static double normal_cdf(double x, double mean, double stddev) {                                 // ref: common/util.h:311-326
  double y = (x - mean) / stddev; if (y < 0) y = -y;
  const double b0 = 0.2316419, b1 = 0.319381530, b2 = -0.356563782, b3 = 1.781477937, b4 = -1.821255978, b5 = 1.330274429, pi = 3.141592653589;
  const double t = 1.0 / (1.0 + b0 * y);
  double res = (exp(-y * y / 2) / sqrt(2.0 * pi)) * ((((b5 * t + b4) * t + b3) * t + b2) * t + b1) * t;
  if (x > mean) res = 1 - res;
  return res;
}
static double pr_insert_size(const PairCtx& C, double ins) {                                     // ref: output.c:795-808
  double res = normal_cdf(ins + 10, C.O.insert_size_mean, C.O.insert_size_stddev) - normal_cdf(ins - 10, C.O.insert_size_mean, C.O.insert_size_stddev);
  if (res < 1e-200) res = 1e-200;
  return res;
}
static double pr_missed(int read_len) { return read_len < 40 ? 1e-10 : (read_len < 60 ? 1e-14 : 1e-16); }   // ref: mapping.h:28-37
static double pr_random_mapping_given_score(const PairCtx& C, int read_len, int score) {         // ref: mapping.h:39-61
  const gm_params_t& P = C.s->P;
  if (score > read_len * P.match_score) return 1e-200;
  const unsigned a = (unsigned)(read_len * P.match_score - score), b = (unsigned)abs(P.colour_space ? P.crossover_score : P.mismatch_score - P.match_score);   // colour space: crossovers
  const int n_mismatches = (a == 0) ? 0 : (int)((a - 1) / b + 1);                                // ceil_div, ref: util.h:213-219
  double lnck = 0.0; for (int i = 0; i < n_mismatches; i++) lnck += log(read_len - i) - log(i + 1);   // ref: util.c:1306-1313
  const double tmp = -lnck - n_mismatches * log(3) + read_len * log(4);
  return exp(-tmp);
}

// compute_paired_mqv (ref: output.c:811-942).  fp = final pairs (h[] index HP[nip]), U[nip] = final unpaired hits.
static void compute_paired_mqv(const PairCtx& C, FHit* const HP[2], const PPair* fp, int nfp, std::vector<FHit*> U[2]) {
  double z1[2], z3, pr_top_random[3] = {1.0, 1.0, 1.0}, pr_missed_mp[2], class_select_denom;
  for (int nip = 0; nip < 2; nip++) {
    z1[nip] = 0;
    for (auto* h : U[nip]) z1[nip] += h->posterior;
    for (auto* h : U[nip]) { h->z0 = h->posterior; h->z1 = z1[nip]; }
  }
  double insert_size_denom = 0.0;
  for (int j = 0; j < nfp; j++) insert_size_denom += pr_insert_size(C, fp[j].insert_size);
  // pools: windows of the final pairs in order of first appearance (readpair_save_final_hits, ref: mapping.c:2446-2499)
  int pool[2][GM_SEL_MAX]; int npool[2] = {0, 0};
  for (int j = 0; j < nfp; j++)
    for (int nip = 0; nip < 2; nip++) {
      int k = 0; while (k < npool[nip] && pool[nip][k] != fp[j].h[nip]) k++;
      if (k == npool[nip]) pool[nip][npool[nip]++] = fp[j].h[nip];
    }
  z3 = 0.0;
  for (int nip = 0; nip < 2; nip++)
    for (int k = 0; k < npool[nip]; k++) {
      FHit& rh = HP[nip][pool[nip][k]];
      rh.insert_size_denom = insert_size_denom;
      double tmp = 0.0;
      for (int j = 0; j < nfp; j++) if (fp[j].h[nip] == pool[nip][k]) tmp += pr_insert_size(C, fp[j].insert_size) * HP[1 - nip][fp[j].h[1 - nip]].posterior;
      tmp *= rh.posterior;
      if (tmp < 1e-200) tmp = 1e-200;
      rh.z2 = tmp;
      if (nip == 0) z3 += tmp;
    }
  for (int nip = 0; nip < 2; nip++) for (int k = 0; k < npool[nip]; k++) HP[nip][pool[nip][k]].z3 = z3;
  for (int nip = 0; nip < 2; nip++) {
    if (U[nip].empty()) continue;
    size_t mx = 0;
    for (size_t i = 1; i < U[nip].size(); i++) if (U[nip][i]->z0 > U[nip][mx]->z0) mx = i;
    pr_top_random[nip] = pr_random_mapping_given_score(C, C.len[nip], U[nip][mx]->score_full);
    for (auto* h : U[nip]) h->pr_top_random = pr_top_random[nip];
    pr_top_random[nip] *= C.total_genome_size;
    if (pr_top_random[nip] > 1) pr_top_random[nip] = 1.0;
  }
  for (int j = 0; j < nfp; j++) {
    double tmp = pr_random_mapping_given_score(C, C.len[0], HP[0][fp[j].h[0]].score_full);
    tmp *= pr_random_mapping_given_score(C, C.len[1], HP[1][fp[j].h[1]].score_full);
    tmp *= 1000;
    if (tmp < pr_top_random[2]) pr_top_random[2] = tmp;
  }
  for (int j = 0; j < nfp; j++) { HP[0][fp[j].h[0]].pr_top_random = pr_top_random[2]; HP[1][fp[j].h[1]].pr_top_random = pr_top_random[2]; }
  pr_top_random[2] *= C.total_genome_size;
  if (pr_top_random[2] > 1) pr_top_random[2] = 1.0;
  for (int nip = 0; nip < 2; nip++) {
    pr_missed_mp[nip] = pr_missed(C.len[1 - nip]);
    for (auto* h : U[nip]) h->pr_missed_mp = pr_missed_mp[nip];
  }
  class_select_denom = 0.0;
  if (!U[0].empty()) class_select_denom += pr_top_random[1] * pr_top_random[2] * pr_missed_mp[0];
  if (!U[1].empty()) class_select_denom += pr_top_random[0] * pr_top_random[2] * pr_missed_mp[1];
  if (nfp > 0) class_select_denom += pr_top_random[0] * pr_top_random[1];
  for (int nip = 0; nip < 2; nip++)
    for (auto* rh : U[nip]) {
      const double p_corr = (pr_top_random[1 - nip] * pr_top_random[2] * pr_missed_mp[nip] / class_select_denom) * (rh->z0 / rh->z1);
      rh->mqv = qv_from_pr_corr(p_corr); if (rh->mqv < 4) rh->mqv = 0;
    }
  for (int j = 0; j < nfp; j++)
    for (int nip = 0; nip < 2; nip++) {
      FHit& rh = HP[nip][fp[j].h[nip]];
      const double p_corr = (pr_top_random[0] * pr_top_random[1] / class_select_denom) * (rh.z2 / rh.z3);
      rh.mqv = qv_from_pr_corr(p_corr); if (rh.mqv < 4) rh.mqv = 0;
    }
}

// K1 + K1b + K2 for one read set, nothing waits on the host: the heavy count goes to the pinned word *pin (the caller looks at it after the
// front's event and runs the heavy tier then)
static int stage_windows_async(gm_session* s, DevSet& D, const GmIndexDev& dv, int n, int read_len, unsigned long long* d_stats, uint32_t* pin,
                               hipEvent_t k1_begin = nullptr, hipEvent_t k1_end = nullptr) {
  const int read_words = (read_len + 7) / 8, W = window_len_of(s->P, read_len);
  hipStream_t q = s->stream;
  int fused = 0;
  if (k1_begin) GM_HIP(hipEventRecord(k1_begin, q));
  int rc = launch_lookup(s, D, dv, n, read_len, read_words, W, d_stats, &fused);
  if (rc) return rc;
  if (k1_end) GM_HIP(hipEventRecord(k1_end, q));
  rc = launch_prune_anchors(s, D, dv, n, read_len, W, d_stats, fused);
  if (rc) return rc;
  GM_HIP(hipMemcpyAsync(pin, D.d_heavy_cnt, 4, hipMemcpyDeviceToHost, q));
  return GM_OK;
}

namespace {                                                    // (the call's own types: nothing of them is exported)
// -C / -F do not apply in paired mode (ref: gmapper.c:2448-2451)
struct BothStrands { gm_session* s; int v; explicit BothStrands(gm_session* s_) : s(s_), v(s_->sc.skip_strands) { s->sc.skip_strands = 0; } ~BothStrands() { s->sc.skip_strands = v; } };
// One gm_map_pairs call: what init() settles before the first sub-batch and nothing changes after it (the output thread reads it beside the calling thread).
struct PairCall {
  gm_session* s = nullptr; const gm_index* ix = nullptr; gm_pair_opts_t O; int pmode = 4, n_pairs = 0; bool mp_counts = false, cs = false, timing = false;
  std::optional<BothStrands> both_strands;
  int len[2], rwords[2], W[2], ovl[2], in_st[2]; const uint32_t* mates[2]; const uint8_t* initbp_in[2];
  GmIndexDev dv, dvm[2];                                       // dvm: the view each mate's kernels get (see init)
  hipStream_t qa = nullptr, q = nullptr;                       // the front's stream; the stream of everything after the front
  int dmin[2], dmax[2], dmin2[2], dmax2[2];                    // insert ranges as window-offset deltas, from the first mate and from the second
  GmScoreDev scp, scr, sc_half; int cs9[9];                    // score sets: the paired pass 1, the rescue's pass 1, the paired pass 2; sw_full_cs_setup's arguments
  PairCtx C;
  std::vector<const char*> nptr[2], qptr[2]; std::vector<int> nlen[2]; bool named = false, quals = false; int qual_delta = 33;   // name and QUAL line of every mate
  int nthreads = 1; DevSet* PS[2][2]; bool overlap = false; uint32_t* per_pair_bytes = nullptr; gm_map_stats_t* stats = nullptr;
  void parallel_chunks(int nchunks, const std::function<void(int)>& fn) const {
    std::atomic<int> next(0);
    auto worker = [&]() { for (;;) { int c = next.fetch_add(1); if (c >= nchunks) break; fn(c); } };
    gm_run_on_threads(std::min(nthreads, nchunks), worker);
  }
  // validation, then the set-up (map_pairs_impl has checked s, n_pairs, the lengths and the read pointers)
  int init(gm_session* s_, int n_pairs_, int len1, const uint32_t* m1, int len2, const uint32_t* m2, const char* names1, const char* names2, const gm_pair_opts_t* opts,
           gm_map_stats_t* stats_, const char* quals1, const char* quals2, int qual_delta_, const uint8_t* initbp1, const uint8_t* initbp2, uint32_t* per_pair_bytes_) {
    s = s_; n_pairs = n_pairs_; stats = stats_; qual_delta = qual_delta_; per_pair_bytes = per_pair_bytes_;
    GM_HIP(hipSetDevice(s->ix->device));
    int rc = ensure_host_genome(s); if (rc) return rc;
    cs = s->P.colour_space != 0;
    initbp_in[0] = initbp1; initbp_in[1] = initbp2;
    if (cs && n_pairs > 0 && (!initbp1 || !initbp2)) { gm_set_error("gm_map_pairs_cs: no primer letters"); return GM_E_ARG; }
    if (opts) O = *opts; else gm_pair_opts_default(&O);
    if (O.pair_mode < GM_PAIR_OPP_IN || O.pair_mode > GM_PAIR_COL_BW) { gm_set_error("gm_map_pairs: pair_mode %d", O.pair_mode); return GM_E_ARG; }
    // half_paired = 0 (--no-half-paired): each mate's list entries are filtered by the other mate's region counts (k_mp_filter, ref: mapping.c:545-608,
    // gmapper.c:2657-2662 use_mp_region_counts = 1) and no unpaired rescue runs afterwards (gmapper.c:2678-2683)
    // match_mode (the reference's -n in paired mode, gmapper.c:2652-2673): 4 as above; 3: the lookup also keeps the entries of regions marked once that the mate reaches
    // with a region it marked twice (GmMpDev; without half-paired the filter then applies rule 3), the window kernel runs hit-list mode 3; 2: no region counts, a window
    // per anchor.  pass 1 asks for two matches only in mode 4 (:2673); the unpaired rescue always does (:2708).
    pmode = O.match_mode == 0 ? 4 : O.match_mode;
    if (pmode < 2 || pmode > 4) { gm_set_error("gm_map_pairs: match_mode %d (2, 3 or 4 in paired mode, ref: gmapper.c:2495-2498)", O.match_mode); return GM_E_ARG; }
    mp_counts = !O.half_paired && pmode == 4;
    both_strands.emplace(s);
    scp = s->sc; scp.match_mode = pmode == 4 ? 2 : (pmode == 3 ? 3 : 1); scp.min_matches = pmode == 4 ? 2 : 1;      // hit_list.match_mode, pass1.min_matches of the paired set
    scr = s->sc; scr.min_matches = 2;                                                                                // the half-paired rescue's pass 1
    len[0] = len1; len[1] = len2; mates[0] = m1; mates[1] = m2;
    for (int m = 0; m < 2; m++) { rc = check_read_len(s, len[m], pmode); if (rc) return rc; }
    GM_HIP(hipSetDevice(s->ix->device));
    if (stats) memset(stats, 0, sizeof *stats);
    s->last_lookup_ms = 0; s->last_lookup_bytes = 0; s->last_lookup_launches = 0;
    ix = s->ix; dv = ix->dev_view();
    // colour space: a mate the pair mode reverses (read_reverse, ref: gmapper.c:174-185,561-570) keeps its colours and swaps its strand labels (GmIndexDev::cs_flip);
    // letter space: it is stored reverse-complemented (k_revcomp_reads)
    dvm[0] = dvm[1] = dv;
    qa = s->stream; q = s->stream_b;
    static const bool pair_reverse[5][2] = {{0, 0}, {0, 0}, {1, 1}, {0, 1}, {1, 0}};   // ref: gmapper-defaults.h:184-191
    for (int m = 0; m < 2; m++) {
      rwords[m] = (len[m] + 7) / 8; W[m] = window_len_of(s->P, len[m]);
      ovl[m] = (int)(unsigned int)(s->P.window_overlap < 0 ? -s->P.window_overlap : W[m] * (s->P.window_overlap / 100.0));
      in_st[m] = pair_reverse[O.pair_mode][m] ? 1 : 0;
      if (cs) dvm[m].cs_flip = in_st[m];
      DevSet& D = s->set[m];
      if (D.cur_len != len[m] || D.d_pmin == nullptr || (D.caps_pair_mode != pmode && (pmode != 4 || D.caps_pair_mode != 0))) { choose_caps(s, D, len[m], pmode); D.caps_pair_mode = pmode; rc = alloc_buffers(s, D, len[m], true); if (rc) return rc; }
    }
    // Two pairs of buffer sets: the front (K1, K1b, K2 of both mates; stream A) of sub-batch i + 1 is queued before the host turns to the rest of
    // sub-batch i (stream B), as in map_impl.  GM_OVERLAP=0: one pair, in order.
    PS[0][0] = &s->set[0]; PS[0][1] = &s->set[1]; PS[1][0] = &s->set2[0]; PS[1][1] = &s->set2[1];
    overlap = n_pairs > std::min(s->set[0].eff_batch, s->set[1].eff_batch);
    if (const char* e = getenv("GM_OVERLAP")) overlap = overlap && atoi(e) != 0;
    if (overlap)
      for (int m = 0; m < 2; m++) {
        DevSet& D = s->set2[m]; const DevSet& R = s->set[m];
        if (D.cur_len != len[m] || D.d_pmin == nullptr || D.scap != R.scap || D.scap2 != R.scap2 || D.hcap < R.hcap || D.rcap_per_read < R.rcap_per_read) {
          D.scap = R.scap; D.scap2 = R.scap2; D.hcap = std::max(D.hcap, R.hcap); D.rcap_per_read = std::max(D.rcap_per_read, R.rcap_per_read);
          rc = alloc_buffers(s, D, len[m], true); if (rc) return rc;
        }
      }
    // readpair_compute_mp_ranges, ref: mapping.c:2317-2442 (only the delta_g_off part is used without mate-pair region counts)
    const int mn = O.min_insert_size, mx = O.max_insert_size;
    int a = mn - W[1], b = mx + (W[0] - len[0]) - len[1], c = -mx + len[0] + (len[1] - W[1]), d = -mn + W[0];
    switch (O.pair_mode) {
      case GM_PAIR_OPP_IN: break;
      case GM_PAIR_OPP_OUT: a += len[0] + len[1]; b += len[0] + len[1]; c -= len[0] + len[1]; d -= len[0] + len[1]; break;
      case GM_PAIR_COL_FW: a += len[1]; b += len[1]; c -= len[1]; d -= len[1]; break;
      default: a += len[0]; b += len[0]; c -= len[0]; d -= len[0]; break;
    }
    dmin[0] = a; dmax[0] = b; dmin[1] = c; dmax[1] = d;
    // the second mate's ranges (ref: mapping.c:2340-2343,2366-2369,2381-2384,2407-2410)
    if (O.pair_mode == GM_PAIR_OPP_IN || O.pair_mode == GM_PAIR_OPP_OUT) { dmin2[0] = -dmax[1]; dmax2[0] = -dmin[1]; dmin2[1] = -dmax[0]; dmax2[1] = -dmin[0]; }
    else { dmin2[0] = -dmax[0]; dmax2[0] = -dmin[0]; dmin2[1] = -dmax[1]; dmax2[1] = -dmin[1]; }
    C.s = s; C.O = O; C.len[0] = len1; C.len[1] = len2; C.rwords[0] = rwords[0]; C.rwords[1] = rwords[1]; C.total_genome_size = (double)ix->total_len;
    const char* names[2] = {names1, names2}; const char* qualsv[2] = {quals1, quals2};
    for (int m = 0; m < 2; m++) if (names[m]) split_lines(names[m], n_pairs, nptr[m], &nlen[m]);
    named = names1 && names2;
    if ((quals1 != nullptr) != (quals2 != nullptr)) { gm_set_error("gm_map_pairs_fastq: QUAL strings for both mates or for none"); return GM_E_ARG; }
    quals = quals1 != nullptr;                                 // FASTQ input: QUAL string of every mate
    for (int m = 0; m < 2; m++)
      if (qualsv[m]) {
        char fmt[96]; snprintf(fmt, sizeof fmt, "pair %%d, mate %d: QUAL string of %%d characters for %%d bases", m + 1);
        rc = split_lines(qualsv[m], n_pairs, qptr[m], nullptr, len[m], fmt); if (rc) return rc;
      }
    nthreads = gm_host_threads(16);
    sc_half = s->sc;                                                                    // per-mate threshold of the paired pass 2, ref: gmapper.c:2677
    if (s->P.sw_full_threshold < 0) { sc_half.full_thr_frac = -1.0; sc_half.full_abs = (int)(-(s->P.sw_full_threshold * 0.5)); }
    else sc_half.full_thr_frac = (s->P.sw_full_threshold * 0.5) / 100.0;
    cs_setup_args(s->P, cs9);
    timing = gm_tune("GM_TIMING") != nullptr;
    return GM_OK;
  }
};
// One sub-batch from the paired pass 2 on: the calling thread fills it stage by stage, then the output thread owns it.  resP / opsP, resU / opsU: the paired and
// the unpaired results in one of the session's two pinned sets (pinned: the copies run at link rate beside the kernels)
struct PairOut {
  int base = 0, n = 0, chunk = 2048, nchunks = 0, NO = 1, ops_stride[2] = {0, 0};
  HitScorer F[2];                                                // the mates' post_sw and unpaired selection
  GmPinVec<GmFullRes>* resP = nullptr; GmPinVec<uint8_t>* opsP = nullptr; GmPinVec<GmFullRes>* resU = nullptr; GmPinVec<uint8_t>* opsU = nullptr;
  std::vector<FHit> fhP[2]; std::vector<PPair> fpairs; std::vector<int> fcnt; std::vector<uint32_t> offP[2], cntU[2], offU[2];
};
struct PairScratch { std::vector<FHit> fhU[2]; std::vector<FHit*> U[2]; };      // a worker's unpaired mappings of the pair in hand, reused from pair to pair
// What is printed for a pair: paired records [first2, last2) of fp, unpaired ones [firstU[m], lastU[m]) of each mate; --single-best-mapping narrows them by the mapping
// qualities (set by now) and may add one improper pair of two unpaired mappings, imp[] (ref: output.c:1086-1235)
struct PairPlan { int first2, last2, firstU[2], lastU[2]; const FHit* imp[2]; };
static PairPlan plan_pair_output(const gm_params_t& P, FHit* const HP[2], const PPair* fp, int nfp, const std::vector<FHit*> U[2]) {
  PairPlan p = {0, nfp, {0, 0}, {(int)U[0].size(), (int)U[1].size()}, {nullptr, nullptr}};
  if (!gm_mqv_on(P) || !P.single_best_mapping || !(nfp > 0 || !U[0].empty() || !U[1].empty())) return p;
  int max_idx_unpaired[2] = {-1, -1}, max_mqv_unpaired[2] = {-1, -1}, max_mqv_paired[2] = {-1, -1}; const FHit* max_hit_paired[2] = {nullptr, nullptr};
  for (int nip = 0; nip < 2; nip++) {
    for (int i = 0; i < (int)U[nip].size(); i++) if (U[nip][i]->mqv > max_mqv_unpaired[nip]) { max_mqv_unpaired[nip] = U[nip][i]->mqv; max_idx_unpaired[nip] = i; }
    // the pool of paired hits in the order readpair_save_final_hits builds it: first appearance over the pairs (a repeated hit compares equal: strict >)
    for (int j = 0; j < nfp; j++) { const FHit* h = &HP[nip][fp[j].h[nip]]; if (h->mqv > max_mqv_paired[nip]) { max_mqv_paired[nip] = h->mqv; max_hit_paired[nip] = h; } }
  }
  // get_idx_mp_max_mqv (ref: output.c:1049-1067): of the pairs that hold hit h of mate nip, the first whose other mate has the best quality
  auto pair_of = [&](int nip, const FHit* h) { int best = -1, idx = -1; for (int j = 0; j < nfp; j++) if (&HP[nip][fp[j].h[nip]] == h) { const int q = HP[1 - nip][fp[j].h[1 - nip]].mqv; if (q > best) { best = q; idx = j; } } return idx; };
  if (!P.all_contigs) {
    for (int nip = 0; nip < 2; nip++) if (max_idx_unpaired[nip] >= 0) { p.firstU[nip] = max_idx_unpaired[nip]; p.lastU[nip] = p.firstU[nip] + 1; }
    const int best_nip = max_mqv_paired[0] > max_mqv_paired[1] ? 0 : 1;
    if (max_mqv_paired[best_nip] >= 0) { p.first2 = pair_of(best_nip, max_hit_paired[best_nip]); p.last2 = p.first2 + 1; }
    return p;
  }
  int max_mqv[2]; bool max_is_paired[2];
  for (int nip = 0; nip < 2; nip++) {
    if (max_mqv_unpaired[nip] > max_mqv_paired[nip]) { max_mqv[nip] = max_mqv_unpaired[nip]; max_is_paired[nip] = false; }
    else { max_mqv[nip] = max_mqv_paired[nip]; max_is_paired[nip] = true; }
  }
  const int best_nip = max_mqv[0] >= max_mqv[1] ? 0 : 1;
  if (max_is_paired[best_nip]) { p.lastU[0] = p.lastU[1] = 0; p.first2 = pair_of(best_nip, max_hit_paired[best_nip]); p.last2 = p.first2 + 1; return p; }
  int idx_best_other = -1; double max_other_z0 = 0.0;
  const auto& OU = U[1 - best_nip];
  for (int i = 0; i < (int)OU.size(); i++) if (OU[i]->z0 > max_other_z0) { max_other_z0 = OU[i]->z0; idx_best_other = i; }
  int best_other_mqv = -1;
  if (idx_best_other >= 0) best_other_mqv = qv_from_pr_corr(max_other_z0 / OU[idx_best_other]->z1);
  if (P.no_improper_mappings || max_mqv_unpaired[best_nip] < 10 || best_other_mqv < 10) {
    p.last2 = 0; p.lastU[1 - best_nip] = 0; p.firstU[best_nip] = max_idx_unpaired[best_nip]; p.lastU[best_nip] = p.firstU[best_nip] + 1;
  } else {                                                            // both good: one improper pair, possibly across contigs
    p.imp[best_nip] = U[best_nip][max_idx_unpaired[best_nip]]; p.imp[1 - best_nip] = OU[idx_best_other];
    p.last2 = 0; p.lastU[0] = p.lastU[1] = 0;
  }
  return p;
}

// What readpair_output settles for pair pr before it prints (ref: output.c:1070-1235): the mates' unpaired selection (t.U afterwards), the paired mapping qualities, the
// plan.  emit_pair prints from it; gm_pair_mappings (gm_host_pair_mappings.inc) hands the same out as arrays.
static PairPlan settle_pair(const PairCall& c, PairOut& b, int pr, PairScratch& t) {
  const gm_params_t& P = c.s->P;
  FHit* HP[2] = {b.fhP[0].data() + b.offP[0][pr], b.fhP[1].data() + b.offP[1][pr]};
  std::vector<FHit*>* const U = t.U;
  for (int m = 0; m < 2; m++) b.F[m].select_hits(b.cntU[m][pr] ? &b.resU[m][b.offU[m][pr]] : nullptr, b.opsU[m].data(), (int)b.cntU[m][pr], t.fhU[m], U[m]);
  const PPair* fp = &b.fpairs[(size_t)pr * b.NO]; const int nfp = b.fcnt[pr];
  if (gm_mqv_on(P)) compute_paired_mqv(c.C, HP, fp, nfp, U);                  // --local / --no-mapping-qualities: none (ref: gmapper.c:2258,2325-2328, output.c:1092)
  return plan_pair_output(P, HP, fp, nfp, U);
}
// readpair_output for pair pr of the sub-batch (ref: output.c:1070-1291): the mates' unpaired selection, the paired mapping qualities, the text.  Returns the number of
// records; t.U holds the unpaired mappings afterwards.
static uint64_t emit_pair(const PairCall& c, PairOut& b, int pr, std::string& o, PairScratch& t) {
  const gm_params_t& P = c.s->P;
  const long gp = (long)b.base + pr;
  FHit* HP[2] = {b.fhP[0].data() + b.offP[0][pr], b.fhP[1].data() + b.offP[1][pr]};
  std::vector<FHit*>* const U = t.U;
  const PPair* fp = &b.fpairs[(size_t)pr * b.NO]; const int nfp = b.fcnt[pr];
  const PairPlan p = settle_pair(c, b, pr, t);
  // QNAME = common prefix of the two names, minus a trailing ':' or '/' (ref: output.c:365-378)
  const char* qn; size_t qnl; char qbuf[40];
  if (c.named) {
    const char* a = c.nptr[0][gp]; const char* z = c.nptr[1][gp]; const size_t na = (size_t)c.nlen[0][gp], nb = (size_t)c.nlen[1][gp];
    size_t i = 0; while (i < std::min(na, nb) && a[i] == z[i]) i++;
    if (i > 0 && (a[i - 1] == ':' || a[i - 1] == '/')) i--;
    qn = a; qnl = i;
  } else { qnl = (size_t)snprintf(qbuf, sizeof qbuf, "p%ld", gp); qn = qbuf; }
  const RecCtx C{P, c.s->ix->names, c.s->ix->contig_off, c.s->h_genome.data()};
  auto mate_view = [&](int m) { return RecRead{qn, qnl, c.mates[m] + (size_t)gp * c.rwords[m], c.len[m], c.cs ? (int)c.initbp_in[m][gp] : -1,
                                               c.quals ? c.qptr[m][gp] : nullptr, c.qual_delta, nullptr, b.ops_stride[m]}; };
  const RecRead R[2] = {mate_view(0), mate_view(1)};
  uint64_t k = 0;
  if (P.output_format) {
    // --shrimp-format / -P: one line (block) per mapped mate under the mate's own name, ">name" for the unmapped mate of a half-paired
    // mapping (ref: gmapper/output.c:270-296, hit_output called per mate by readpair_output :1070-1291)
    auto one = [&](int m, const FHit* rh) {
      RecRead rd = R[m];
      if (c.named) { rd.name = c.nptr[m][gp]; rd.name_len = (size_t)c.nlen[m][gp]; }
      if (!rh) { o += '>'; o.append(rd.name, rd.name_len); o += '\n'; return; }
      shrimp_record(C, rd, *rh, o);
    };
    for (int j = p.first2; j < p.last2; j++) { one(0, &HP[0][fp[j].h[0]]); one(1, &HP[1][fp[j].h[1]]); k += 2; }
    if (p.imp[0]) { one(0, p.imp[0]); one(1, p.imp[1]); k += 2; }
    for (int i = p.firstU[0]; i < p.lastU[0]; i++) { one(0, U[0][i]); one(1, nullptr); k += 2; }
    for (int i = p.firstU[1]; i < p.lastU[1]; i++) { one(0, nullptr); one(1, U[1][i]); k += 2; }
    return k;
  }
  // --sam-r2: every record carries the MATE's sequence as given (re_mp->seq: letters, or primer + colours; ref: output.c:452-460,729-737)
  std::string mseq[2]; const std::string* ms[2] = {nullptr, nullptr};
  if (P.sam_r2) {
    for (int m = 0; m < 2; m++) {
      const int L = c.len[m]; const uint32_t* rw = R[m].words;
      if (c.cs) { mseq[m] += "ACGT"[R[m].primer & 3]; for (int i = 0; i < L; i++) { const int cc = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; mseq[m] += (cc < 4) ? (char)('0' + cc) : '.'; } }
      else for (int i = 0; i < L; i++) { const int cc = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; mseq[m] += (cc < 4) ? "ACGT"[cc] : (cc == 4 ? 'U' : 'N'); }
    }
    ms[0] = &mseq[1]; ms[1] = &mseq[0];                                        // (mate 1's records carry mate 2's sequence and the other way round)
  }
  // the two records of one line of the output: mate 0's mapping h0 and mate 1's h1 (null: that mate is unmapped)
  auto two = [&](const FHit* h0, const FHit* h1, bool improper) {
    const RecMate of0{true, improper, h1, ms[0]}, of1{false, improper, h0, ms[1]};      // what mate 0's record says of mate 1, and the other way round
    sam_record(C, R[0], h0, &of0, o); sam_record(C, R[1], h1, &of1, o);
    k += 2;
  };
  for (int j = p.first2; j < p.last2; j++) two(&HP[0][fp[j].h[0]], &HP[1][fp[j].h[1]], false);
  if (p.imp[0]) two(p.imp[0], p.imp[1], true);
  for (int ui = p.firstU[0]; ui < p.lastU[0]; ui++) two(U[0][ui], nullptr, false);
  for (int ui = p.firstU[1]; ui < p.lastU[1]; ui++) two(nullptr, U[1][ui], false);
  if (nfp == 0 && U[0].empty() && U[1].empty() && P.sam_unaligned) two(nullptr, nullptr, false);      // ref: mapping.c:2627-2633
  return k;
}

// The output stage of a sub-batch (unpaired selection, mapping qualities, text: ~6 of a sub-batch's ~70 ms, all host) runs on a thread of its own beside the device work of
// the next sub-batch; at most one is outstanding, and its text is appended -- in order -- before the next one starts.
struct OutJob { std::thread th; std::vector<std::string> outs; std::vector<uint64_t> cm, cr; double ms = 0; bool failed = false; ~OutJob() { if (th.joinable()) th.join(); } };
static void pair_output(const PairCall& c, PairOut& b, OutJob& J) {
  const auto t0 = std::chrono::steady_clock::now();
  c.parallel_chunks(b.nchunks, [&](int ch) {
    PairScratch t; std::string& o = J.outs[ch]; o.reserve((size_t)b.chunk * (c.len[0] + c.len[1] + 300));
    for (int pr = ch * b.chunk; pr < std::min(b.n, (ch + 1) * b.chunk); pr++) {
      const size_t o_before = o.size();
      J.cr[ch] += emit_pair(c, b, pr, o, t);
      if (b.fcnt[pr] > 0 || !t.U[0].empty() || !t.U[1].empty()) J.cm[ch]++;
      if (c.per_pair_bytes) c.per_pair_bytes[(long)b.base + pr] = (uint32_t)(o.size() - o_before);
    }
  });
  J.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
// what the paired pass hands from stage to stage on the calling thread
struct PairSel { uint32_t n_work[2] = {0, 0}; std::vector<uint32_t> cntP[2], plist, pcnt; std::vector<std::vector<uint32_t>> saved_chunks[2]; };
// The call's state that changes from sub-batch to sub-batch, and the stages of a sub-batch in the order map_pairs_impl calls them.  Each stage queues its HIP calls on
// qa (front) or q (the rest) and returns GM_OK, GM_REDO or an error.
struct PairRun : PairCall {
  // -n 4 without half-paired: k_mp_filter works on the survivor lists in LDS; a sub-batch in which some pair did not fit its tiers (or a read-strand went to the heavy
  // tier, which re-emits without the mate's counts) is redone through the generic kernel's mate-pair modes (rows of regions marked twice, then rule 1: GmMpDev mode 5),
  // and so is the rest of the call
  bool mp_exact = gm_tune("GM_MP_EXACT") != nullptr;
  GmIndexDev dkm[2][2];           // match modes 3 / 2: each mate's view with its mate-pair fields, per buffer pair (the heavy tier reads it again)
  std::vector<unsigned long long> hraw = std::vector<unsigned long long>((size_t)GS_STRIPES * GS_STRIDE); unsigned long long hs[GS_N];
  std::vector<std::string> pieces_all; uint64_t matched = 0, records = 0;
  bool out_failed = false;         // (an allocation failed on the output thread: no exception leaves a thread; the call ends with GM_E_NOMEM)
  int cur = 0; DevSet* S[2] = {nullptr, nullptr}; unsigned long long* dst = nullptr;      // the buffer pair of the sub-batch in hand, its counters
  std::chrono::steady_clock::time_point tw;
  std::unique_ptr<OutJob> pending; // (last: its thread reads the PairCall part, and is joined before anything here goes away)
  int lap(const char* what) { if (timing) { GM_HIP(hipStreamSynchronize(q)); auto n2 = std::chrono::steady_clock::now(); fprintf(stderr, "  pairs %-18s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(n2 - tw).count()); tw = n2; } return 0; }
  // stage times of the back part (gm_map_stats_t, as the unpaired path fills them): events on the back stream, read behind the synchronisation points that exist anyway
  int stage_ms(int e0, int e1, double gm_map_stats_t::* field) { float ms = 0; GM_HIP(hipEventElapsedTime(&ms, s->ev[e0], s->ev[e1])); if (stats) stats->*field += ms; return GM_OK; }
  // the stages after the front work on buffer pair k from here on; B: the pairs a sub-batch on it can hold
  int use_pair(int k, int B) {
    cur = k; S[0] = PS[k][0]; S[1] = PS[k][1]; dst = s->d_pstats[k]; tw = std::chrono::steady_clock::now();
    if (s->pairs_cap >= B) return GM_OK;
    if (s->d_pairs) (void)hipFree(s->d_pairs);
    if (s->d_pair_cnt) (void)hipFree(s->d_pair_cnt);
    s->d_pairs = nullptr; s->d_pair_cnt = nullptr; s->pairs_cap = 0;
    GM_HIP(hipMalloc(&s->d_pairs, (size_t)B * GM_SEL_MAX * 4)); GM_HIP(hipMalloc(&s->d_pair_cnt, (size_t)B * 4)); s->pairs_cap = B;
    return GM_OK;
  }
  // a mate's reads: RNA flags (before the mate is turned: its complement of U is A), then read_reverse in letter space (ref: gmapper.c:174-185,567-570)
  int prep_mate(DevSet& D, int m, int n) {
    int rc;
    if (D.d_read_rna) { rc = gm_launch_read_rna_flags(D.d_reads, n, len[m], rwords[m], D.d_read_rna, qa); if (rc) return rc; }
    if (in_st[m] && !cs) { rc = gm_launch_revcomp_reads(D.d_reads, n, len[m], rwords[m], qa, D.d_read_rna); if (rc) return rc; }
    return GM_OK;
  }
  // K1 of mate m through the generic entry with the view given; timed: the launch whose survivors K2 takes (slab segments out, K1 events around it)
  int lookup(int k, int m, int n, const GmIndexDev& view, bool timed) {
    DevSet& D = *PS[k][m];
    if (timed) GM_HIP(hipEventRecord(s->pkev[k][2 * m], qa));
    int rc = gm_launch_lookup(gm_view_of(view, D), D.d_reads, n, len[m], rwords[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_heavy_list, D.d_heavy_cnt, 2 * D.eff_batch, s->d_pstats[k], qa, &s->k1, timed ? D.d_surv_seg : nullptr, nullptr);
    if (rc) return rc;
    if (timed) GM_HIP(hipEventRecord(s->pkev[k][2 * m + 1], qa));
    return GM_OK;
  }
  // Anchors of mate m's survivors, then the heavy count to its pinned word.  rows (match modes 3 / 2): K2 takes the lookup's rows as they are, with the paired score set.
  // Otherwise the prune rules hold: K2 straight on the survivors when its LDS tier can take a whole row (small and medium genomes), else K1b + K2 -- K1b's overflow goes to
  // the heavy tier, which re-emits a read-strand's survivors from the index without the mate's counts: a heavy read-strand then has the anchors of the half-paired run
  // (a superset: the filter only removes list entries that cannot pair up), or, on the exact path, runs mode 5 too.
  int anchors(int k, int m, int n, const GmIndexDev* rows = nullptr) {
    DevSet& D = *PS[k][m]; unsigned long long* const dst = s->d_pstats[k];
    int rc;
    if (rows) rc = gm_launch_anchors(*rows, scp, n, len[m], W[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, dst, qa);
    else if (D.scap <= 4096) rc = gm_launch_anchors(dv, s->sc, n, len[m], W[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, dst, qa);
    else rc = launch_prune_anchors(s, D, dv, n, len[m], W[m], dst, 0);
    if (rc) return rc;
    GM_HIP(hipMemcpyAsync(&s->h_pin[2 + 2 * k + m], D.d_heavy_cnt, 4, hipMemcpyDeviceToHost, qa));
    return GM_OK;
  }
  // -n 2: the lookup keeps every list entry.  -n 3: a first lookup pass lists, per read-strand, the regions it marked twice; the second keeps the entries of such
  // regions and of regions within reach of one the mate (other strand) marked twice -- count_main >= 2 || count_mp >= 2, use_mp_region_counts == 2; without
  // half-paired a pass in between flags, in each row, the regions the mate reaches at all, and the rule is count_mp >= 1 && count_main + count_mp >= 3
  // (GmMpDev modes 1, 2 / 3 + 4).  No prune rules in either mode: K2 takes the rows as they are.  Also the exact path of -n 4 without half-paired (mode 5).
  int front_rows(int k, int n) {
    const MpDelta dl = gm_mp_region_deltas(ix->params.region_bits, dmin, dmax, dmin2, dmax2);
    int rc;
    for (int m = 0; m < 2; m++) {
      DevSet& D = *PS[k][m];
      rc = prep_mate(D, m, n); if (rc) return rc;
      dkm[k][m] = dvm[m];
      if (pmode == 2) dkm[k][m].no_region_counts = 1;
      else if (D.mp_rows_for < 2 * D.eff_batch) {      // (-n 3, and the exact path of -n 4 without half-paired)
        if (D.d_mp_rows) (void)hipFree(D.d_mp_rows);
        if (D.d_mp_cnt) (void)hipFree(D.d_mp_cnt);
        D.d_mp_rows = nullptr; D.d_mp_cnt = nullptr; D.mp_rows_for = 0;
        GM_HIP(hipMalloc(&D.d_mp_rows, (size_t)2 * D.eff_batch * GM_MP_CAP * 4)); GM_HIP(hipMalloc(&D.d_mp_cnt, (size_t)2 * D.eff_batch * 4));
        D.mp_rows_for = 2 * D.eff_batch;
      }
    }
    if (pmode != 2) {
      for (int m = 0; m < 2; m++) {
        DevSet& D = *PS[k][m];
        GM_HIP(hipMemsetAsync(D.d_mp_cnt, 0, (size_t)2 * n * 4, qa));
        GmIndexDev d1 = dvm[m]; d1.mp.mode = 1; d1.mp.out_rows = D.d_mp_rows; d1.mp.out_cnt = D.d_mp_cnt;
        rc = lookup(k, m, n, d1, false); if (rc) return rc;
      }
      for (int m = 0; m < 2; m++) {
        GmMpDev& M = dkm[k][m].mp; const DevSet& Mate = *PS[k][1 - m];
        M.mode = pmode == 4 ? 5 : (O.half_paired ? 2 : 4); M.rows = Mate.d_mp_rows; M.cnt = Mate.d_mp_cnt; M.out_rows = PS[k][m]->d_mp_rows; M.out_cnt = PS[k][m]->d_mp_cnt;
        for (int st = 0; st < 2; st++) {
          M.dmin[st] = m ? dl.bmin[st] : dl.amin[st]; M.dmax[st] = m ? dl.bmax[st] : dl.amax[st];
          M.mate_dmin[st] = m ? dl.amin[st] : dl.bmin[st]; M.mate_dmax[st] = m ? dl.amax[st] : dl.bmax[st];
        }
      }
      if (pmode == 3 && !O.half_paired)      // rule 3 asks count_mp >= 1 of a region marked twice: both mates flag each other's rows first
        for (int m = 0; m < 2; m++) { GmIndexDev d3 = dkm[k][m]; d3.mp.mode = 3; rc = lookup(k, m, n, d3, false); if (rc) return rc; }
    }
    for (int m = 0; m < 2; m++) { rc = lookup(k, m, n, dkm[k][m], true); if (rc) return rc; }
    for (int m = 0; m < 2; m++) {
      GmIndexDev dk2 = dv; dk2.mp = dkm[k][m].mp;
      rc = anchors(k, m, n, pmode != 4 ? &dk2 : nullptr); if (rc) return rc;      // (-n 4: the prune rules hold)
    }
    return GM_OK;
  }
  // The front of one sub-batch on buffer pair k: reads in (stream C, so that the call never queues behind kernels), K1 + K1b + K2 for both mates
  int front(int k, int base, int n) {
    GM_HIP(hipMemsetAsync(s->d_pstats[k], 0, (size_t)GS_STRIPES * GS_STRIDE * 8, qa));
    for (int m = 0; m < 2; m++)
      GM_HIP(hipMemcpyAsync(PS[k][m]->d_reads, mates[m] + (size_t)base * rwords[m], (size_t)n * rwords[m] * 4, hipMemcpyHostToDevice, s->stream_c));
    if (cs) for (int m = 0; m < 2; m++) GM_HIP(hipMemcpyAsync(PS[k][m]->d_initbp, initbp_in[m] + base, (size_t)n, hipMemcpyHostToDevice, s->stream_c));
    for (int m = 0; m < 2; m++) PS[k][m]->xover_on = false;
    if (cs && quals) for (int m = 0; m < 2; m++) {               // per-position crossover scores from the QVs (as in map_impl)
      std::vector<int8_t> xbuf((size_t)n * len[m]);
      xover_from_quals(s, qptr[m].data() + base, n, len[m], qual_delta, xbuf.data(), nullptr);
      GM_HIP(hipMemcpyAsync(PS[k][m]->d_xover, xbuf.data(), xbuf.size(), hipMemcpyHostToDevice, s->stream_c));
      GM_HIP(hipStreamSynchronize(s->stream_c));                // xbuf goes out of scope
      PS[k][m]->xover_on = true;
    }
    GM_HIP(hipEventRecord(s->pev[k][8], s->stream_c));
    GM_HIP(hipStreamWaitEvent(qa, s->pev[k][8], 0));
    int rc = GM_OK;
    if (pmode != 4 || (mp_counts && mp_exact)) rc = front_rows(k, n);
    else if (mp_counts) {   // K1 of both mates (never fused with the prune: the filter needs every survivor), the mate-pair filter, then K1b + K2 of both
      for (int m = 0; m < 2; m++) { rc = prep_mate(*PS[k][m], m, n); if (rc) return rc; rc = lookup(k, m, n, dvm[m], true); if (rc) return rc; }
      rc = gm_launch_mp_filter(n, ix->params.region_bits, ix->params.region_overlap, PS[k][0]->d_surv, PS[k][0]->d_surv_cnt, PS[k][0]->scap,
                               PS[k][1]->d_surv, PS[k][1]->d_surv_cnt, PS[k][1]->scap, dmin, dmax, dmin2, dmax2, PS[k][0]->d_surv_seg, PS[k][1]->d_surv_seg, ix->n_slabs, s->d_pstats[k], qa);
      for (int m = 0; m < 2 && !rc; m++) rc = anchors(k, m, n);
    } else for (int m = 0; m < 2 && !rc; m++) {
      rc = prep_mate(*PS[k][m], m, n);
      if (!rc) rc = stage_windows_async(s, *PS[k][m], dvm[m], n, len[m], s->d_pstats[k], &s->h_pin[2 + 2 * k + m], s->pkev[k][2 * m], s->pkev[k][2 * m + 1]);
    }
    if (rc) return rc;
    GM_HIP(hipEventRecord(s->pev[k][6], qa));
    return GM_OK;
  }

  // a capacity of this pair grew, or the exact mate-pair path is needed: the sub-batch is redone from its front, and the front queued for the next one is dropped
  int redo() { GM_HIP(hipStreamSynchronize(qa)); GM_HIP(hipStreamSynchronize(q)); if (stats) stats->retries++; return GM_OK; }
  int grow(bool hits_ovf, const uint32_t n_work[2]) {
    bool retry = false;
    for (int m = 0; m < 2; m++) {
      DevSet& D = *S[m];
      bool g = false;
      if (hits_ovf) { if (D.hcap >= 32768) { gm_set_error("window list overflow at capacity %d", D.hcap); return GM_E_OVERFLOW; } D.hcap *= 4; g = true; }
      if (n_work[m] > (size_t)D.eff_batch * D.rcap_per_read) {
        if (D.rcap_per_read >= GM_SEL_MAX) { gm_set_error("pass-2 work overflow"); return GM_E_OVERFLOW; }
        D.rcap_per_read = std::min(GM_SEL_MAX, D.rcap_per_read * 2); g = true;
      }
      if (g) { retry = true; int rc = alloc_buffers(s, D, len[m], true); if (rc) return rc; }
    }
    return retry ? GM_REDO : GM_OK;
  }
  // The front's end: K1's times, the heavy tier of each mate (then the front's end event again), the back stream behind it
  int finish_front(int n) {
    GM_HIP(hipEventSynchronize(s->pev[cur][6]));
    float k1 = 0;
    for (int m = 0; m < 2; m++) {                              // K1's own time for both mate sets of this sub-batch (bench.py's roofline leg)
      float ms = 0; GM_HIP(hipEventElapsedTime(&ms, s->pkev[cur][2 * m], s->pkev[cur][2 * m + 1]));
      if (stats) stats->ms_lookup += ms;
      s->last_lookup_ms += ms; s->last_lookup_launches++; k1 += ms;
    }
    // the rest of the front (K1b, K2, the mate-pair filter of --no-half-paired): from the first K1's begin to the front's end, minus the two K1s
    float span = 0; GM_HIP(hipEventElapsedTime(&span, s->pkev[cur][0], s->pev[cur][6]));
    if (stats) stats->ms_anchors += std::max(0.0f, span - k1);
    if (mp_counts && !mp_exact && (s->h_pin[2 + 2 * cur] || s->h_pin[2 + 2 * cur + 1])) { mp_exact = true; return GM_REDO; }   // (see mp_exact)
    bool heavy = false;
    for (int m = 0; m < 2; m++) {
      const uint32_t n_heavy = s->h_pin[2 + 2 * cur + m];
      if (n_heavy) {
        int rc = (pmode == 4 && !mp_exact) ? run_heavy_tier(s, *S[m], dvm[m], n, len[m], rwords[m], W[m], (int)n_heavy, dst)
                        : run_heavy_tier(s, *S[m], dkm[cur][m], n, len[m], rwords[m], W[m], (int)n_heavy, dst, pmode == 4 ? nullptr : &scp);
        if (rc) return rc; heavy = true;
      }
    }
    if (heavy) GM_HIP(hipEventRecord(s->pev[cur][6], qa));
    GM_HIP(hipStreamWaitEvent(q, s->pev[cur][6], 0));
    lap("K1+K1b+K2 x2");
    return GM_OK;
  }
  // pair-up, pass 1 of both mates over the paired windows, the pair top-K, the pass-2 work lists; then the counters, and what they ask to be redone
  int pass1_select(int n, uint32_t n_work[2]) {
    DevSet& A = *S[0]; DevSet& Bs = *S[1];
    GM_HIP(hipEventRecord(s->ev[0], q));
    int rc = gm_launch_pair_up(n, A.d_hits, A.d_perm, A.d_hit_cnt, A.hcap, Bs.d_hits, Bs.d_perm, Bs.d_hit_cnt, Bs.hcap,
                               A.d_pmin, A.d_pmax, Bs.d_pmin, Bs.d_pmax, dmin, dmax, q);
    if (rc) return rc;
    for (int m = 0; m < 2; m++) {
      DevSet& D = *S[m];
      rc = gm_launch_pass1(gm_view_of(dvm[m], D), scp, D.d_reads, n, len[m], rwords[m], W[m], ovl[m], D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, D.d_slots, dst, q, D.d_pmin, nullptr, cs ? D.d_initbp : nullptr);
      if (rc) return rc;
    }
    GM_HIP(hipEventRecord(s->ev[1], q));
    lap("pair_up+pass1 x2");
    rc = gm_launch_pair_select(s->sc, n, len[0], len[1], A.d_hits, A.d_perm, A.d_hit_cnt, A.hcap, A.d_pmin, A.d_pmax,
                               Bs.d_hits, Bs.d_perm, Bs.d_hit_cnt, Bs.hcap, A.d_sel, A.d_sel_sidx, A.d_sel_cnt, Bs.d_sel, Bs.d_sel_sidx, Bs.d_sel_cnt,
                               s->d_pairs, s->d_pair_cnt, q);
    if (rc) return rc;
    for (int m = 0; m < 2; m++) {
      DevSet& D = *S[m];
      rc = gm_launch_build_work(n, D.d_sel_cnt, D.d_sel_off, D.d_work, D.d_n_work, q); if (rc) return rc;
      GM_HIP(hipMemcpyAsync(&n_work[m], D.d_n_work, 4, hipMemcpyDeviceToHost, q));
    }
    GM_HIP(hipEventRecord(s->ev[2], q));
    GM_HIP(hipMemcpyAsync(hraw.data(), dst, hraw.size() * 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    fold_stats(hraw.data(), hs);
    rc = stage_ms(0, 1, &gm_map_stats_t::ms_pass1); if (rc) return rc;        // (pair_up + the mates' own pass 1)
    rc = stage_ms(1, 2, &gm_map_stats_t::ms_select); if (rc) return rc;
    if (hs[GS_OVERFLOW_SURV]) { gm_set_error("heavy list overflow"); return GM_E_OVERFLOW; }
    if ((pmode == 3 || (mp_counts && mp_exact)) && hs[GS_MP_UNFILTERED]) {   // a row of regions marked twice beyond GM_MP_CAP: no exact answer
      gm_set_error("gm_map_pairs: mate-pair region counts: %llu read-strands beyond the row capacity (%d regions marked twice)", hs[GS_MP_UNFILTERED], GM_MP_CAP); return GM_E_OVERFLOW;
    }
    if (mp_counts && !mp_exact && hs[GS_MP_UNFILTERED]) { mp_exact = true; return GM_REDO; }   // (see mp_exact)
    rc = grow(hs[GS_OVERFLOW_HITS] != 0, n_work); if (rc) return rc;
    lap("pair_select");
    return GM_OK;
  }
  // Pass 2 of both mates, letter or colour, and each mate's four result copies.  paired: the windows of the selected pairs (sel_sidx, the pair flag) -- with sc_half --
  // or the rescue's own selection with the session's score set.  Events ev[e0] before mate 0, ev[e0 + 1] between the mates (the first one's copies are queued behind
  // it), ev[e0 + 2] behind mate 1's kernel.
  int pass2_both(int n, const GmScoreDev& sc, bool paired, int e0, const uint32_t n_work[2], GmPinVec<GmFullRes>* res, GmPinVec<uint8_t>* ops, std::vector<uint32_t> cnt[2], std::vector<uint32_t> off[2]) {
    GM_HIP(hipEventRecord(s->ev[e0], q));
    for (int m = 0; m < 2; m++) {
      DevSet& D = *S[m]; int rc;
      if (m == 1) GM_HIP(hipEventRecord(s->ev[e0 + 1], q));
      if (cs) rc = gm_launch_pass2_cs(dvm[m], sc, cs9, D.d_reads, D.d_initbp, n, len[m], rwords[m], W[m], D.d_hits, D.hcap, D.d_sel, D.d_work, D.d_n_work,
                                      D.d_res, D.d_ops, D.ops_stride, (uint32_t*)D.d_back, D.back_stride / 4, D.p2_grid, dst, q, D.xover_on ? D.d_xover : nullptr, paired ? D.d_sel_sidx : nullptr, D.d_p2_order, D.d_p2_cls);
      else rc = gm_launch_pass2(gm_view_of(dv, D), sc, D.d_reads, n, len[m], rwords[m], W[m], D.d_hits, D.d_perm, D.hcap, D.d_sel, D.d_sel_cnt, D.d_work, D.d_n_work,
                                D.d_res, D.d_ops, D.ops_stride, D.d_back, D.back_stride, D.p2_grid, dst, q, paired ? D.d_sel_sidx : nullptr, in_st[m], paired ? 1 : 0, D.d_p2_order, D.d_p2_cls);
      if (rc) return rc;
      if (m == 1) GM_HIP(hipEventRecord(s->ev[e0 + 2], q));
      rc = res[m].resize(n_work[m]); if (rc) return rc; rc = ops[m].resize((size_t)n_work[m] * D.ops_stride); if (rc) return rc; cnt[m].resize(n); off[m].resize(n);
      if (n_work[m]) {
        GM_HIP(hipMemcpyAsync(res[m].data(), D.d_res, (size_t)n_work[m] * sizeof(GmFullRes), hipMemcpyDeviceToHost, q));
        GM_HIP(hipMemcpyAsync(ops[m].data(), D.d_ops, (size_t)n_work[m] * D.ops_stride, hipMemcpyDeviceToHost, q));
      }
      GM_HIP(hipMemcpyAsync(cnt[m].data(), D.d_sel_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, q));
      GM_HIP(hipMemcpyAsync(off[m].data(), D.d_sel_off, (size_t)n * 4, hipMemcpyDeviceToHost, q));
    }
    return GM_OK;
  }
  // paired pass 2 on the unique windows of the selected pairs, at half the threshold per mate; the pair lists with it
  int paired_pass2(PairOut& b, PairSel& t) {
    t.plist.resize((size_t)b.n * GM_SEL_MAX); t.pcnt.resize(b.n);
    int rc = pass2_both(b.n, sc_half, true, 3, t.n_work, b.resP, b.opsP, t.cntP, b.offP); if (rc) return rc;
    GM_HIP(hipMemcpyAsync(t.plist.data(), s->d_pairs, t.plist.size() * 4, hipMemcpyDeviceToHost, q));
    GM_HIP(hipMemcpyAsync(t.pcnt.data(), s->d_pair_cnt, (size_t)b.n * 4, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    rc = stage_ms(3, 4, &gm_map_stats_t::ms_pass2); if (rc) return rc;        // (mate 0's pass 2 with its result copies, then mate 1's kernel)
    rc = stage_ms(4, 5, &gm_map_stats_t::ms_pass2); if (rc) return rc;
    lap("pass2 (pairs)+copy");
    return GM_OK;
  }
  // host: pair selection (readpair_pass2 per pair) on the host threads; the windows of the final pairs are saved from the rescue
  void select_pairs_host(PairOut& b, PairSel& t) {
    select_setup(b, t);
    parallel_chunks(b.nchunks, [&](int c) {
      std::vector<PPair> v;
      for (int pr = c * b.chunk; pr < std::min(b.n, (c + 1) * b.chunk); pr++) {
        FHit* H[2] = {b.fhP[0].data() + b.offP[0][pr], b.fhP[1].data() + b.offP[1][pr]};
        for (int m = 0; m < 2; m++) for (uint32_t a = 0; a < t.cntP[m][pr]; a++) b.F[m].post_sw(H[m][a], &b.resP[m][b.offP[m][pr] + a], b.opsP[m].data());
        pair_pass2(C, H, t.plist.data() + (size_t)pr * GM_SEL_MAX, (int)t.pcnt[pr], v);
        b.fcnt[pr] = (int)v.size();
        for (size_t j = 0; j < v.size(); j++) {
          b.fpairs[(size_t)pr * b.NO + j] = v[j];
          for (int m = 0; m < 2; m++) t.saved_chunks[m][c].push_back(H[m][v[j].h[m]].r->hit_slot);   // ref: mapping.c:2304-2310
        }
      }
    });
    lap("host pair select");
  }
  // the sizes of the selection's results and the mates' scorers (shared with gm_pair_mappings, whose selection runs on the device)
  void select_setup(PairOut& b, PairSel& t) {
    b.nchunks = (b.n + b.chunk - 1) / b.chunk;
    b.fhP[0].resize(t.n_work[0]); b.fhP[1].resize(t.n_work[1]);
    b.NO = std::max(1, s->P.num_outputs);
    b.fpairs.resize((size_t)b.n * b.NO); b.fcnt.assign(b.n, 0);
    t.saved_chunks[0].resize(b.nchunks); t.saved_chunks[1].resize(b.nchunks);
    for (int m = 0; m < 2; m++) { b.F[m] = HitScorer(); b.F[m].s = s; b.F[m].read_len = len[m]; b.F[m].read_words = rwords[m]; }
    if (cs) {   // post_sw needs the colours and the primer letter of each read (ref: sw-post.c:448-528)
      for (int m = 0; m < 2; m++) {
        HitScorer& F = b.F[m];
        F.reads = mates[m] + (size_t)b.base * rwords[m]; F.initbp = initbp_in[m] + b.base; F.ops_half = S[m]->ops_stride / 2; F.csk = cs_post_consts(s);
        if (quals) { F.qual_ptr = qptr[m].data() + b.base; F.qual_delta = qual_delta; }      // post_sw with the reads' QVs (ref: sw-post.c:486-491)
      }
    }
  }
  // device: half-paired fall-back -- handle_read per mate with the windows already there (ref: mapping.c:2598-2625, gmapper.c:2700-2714)
  int rescue(PairOut& b, PairSel& t) {
    const int n = b.n;
    if (!O.half_paired) { for (int m = 0; m < 2; m++) { b.cntU[m].assign(n, 0); b.offU[m].assign(n, 0); } return GM_OK; }
    uint32_t n_work2[2] = {0, 0}; int rc;
    for (int m = 0; m < 2; m++) {
      DevSet& D = *S[m];
      std::vector<uint32_t> sl; for (auto& v : t.saved_chunks[m]) sl.insert(sl.end(), v.begin(), v.end());
      GM_HIP(hipMemsetAsync(D.d_saved, 0, (size_t)n * 2 * D.hcap, q));
      if (!sl.empty()) {
        GM_HIP(hipMemcpyAsync(D.d_saved_list, sl.data(), sl.size() * 4, hipMemcpyHostToDevice, q));
        rc = gm_launch_mark_saved(D.d_saved, D.d_saved_list, (int)sl.size(), q); if (rc) return rc;
        GM_HIP(hipStreamSynchronize(q));   // sl goes out of scope
      }
      GM_HIP(hipEventRecord(s->ev[6 + 3 * m], q));
      rc = gm_launch_pass1(gm_view_of(dvm[m], D), scr, D.d_reads, n, len[m], rwords[m], W[m], ovl[m], D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, D.d_slots, dst, q, nullptr, D.d_saved, cs ? D.d_initbp : nullptr,
                           true);      // (handle_read per mate: a score below the unpaired threshold is never read again -- the pair sums were formed before)
      if (rc) return rc;
      GM_HIP(hipEventRecord(s->ev[7 + 3 * m], q));
      rc = gm_launch_select(s->sc, n, len[m], D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, D.d_sel, D.d_sel_cnt, D.d_sel_off, D.d_work, D.d_n_work, q, D.d_saved);
      if (rc) return rc;
      GM_HIP(hipEventRecord(s->ev[8 + 3 * m], q));
      GM_HIP(hipMemcpyAsync(&n_work2[m], D.d_n_work, 4, hipMemcpyDeviceToHost, q));
    }
    GM_HIP(hipStreamSynchronize(q));
    for (int m = 0; m < 2; m++) {                            // the rescue's pass 1 and selection, per mate
      rc = stage_ms(6 + 3 * m, 7 + 3 * m, &gm_map_stats_t::ms_pass1); if (rc) return rc;
      rc = stage_ms(7 + 3 * m, 8 + 3 * m, &gm_map_stats_t::ms_select); if (rc) return rc;
    }
    rc = grow(false, n_work2); if (rc) return rc;
    return pass2_both(n, s->sc, false, 0, n_work2, b.resU, b.opsU, b.cntU, b.offU);
  }
  int collect_stats() {
    GM_HIP(hipMemcpyAsync(hraw.data(), dst, hraw.size() * 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    fold_stats(hraw.data(), hs);
    if (O.half_paired) { int rc = stage_ms(0, 1, &gm_map_stats_t::ms_pass2); if (rc) return rc; rc = stage_ms(1, 2, &gm_map_stats_t::ms_pass2); if (rc) return rc; }      // the rescue's pass 2
    if (stats) { add_device_stats(stats, hs); stats->mp_unfiltered += hs[GS_MP_UNFILTERED]; }
    lap("rescue p1+sel+p2");
    return GM_OK;
  }
  void finish_pending() {
    if (!pending) return;
    if (pending->th.joinable()) pending->th.join();
    out_failed = out_failed || pending->failed;
    if (stats) stats->ms_host += pending->ms;
    for (size_t c = 0; c < pending->outs.size(); c++) { matched += pending->cm[c]; records += pending->cr[c]; pieces_all.push_back(std::move(pending->outs[c])); }
    pending.reset();
  }
  void start_output(std::shared_ptr<PairOut> b) {
    finish_pending();                                            // (the sub-batch before this one: its text comes first, and its pinned result set is free again after this)
    std::unique_ptr<OutJob> J(new OutJob());
    J->outs.assign(b->nchunks, std::string()); J->cm.assign(b->nchunks, 0); J->cr.assign(b->nchunks, 0);
    OutJob* const jp = J.get(); const PairCall& call = *this;
    jp->th = std::thread([&call, b, jp]() { try { pair_output(call, *b, *jp); } catch (...) { jp->failed = true; } });
    pending = std::move(J);
    lap("host output");
  }
};
}  // namespace

static int map_pairs_impl(gm_session* s, int n_pairs, int len1, const uint32_t* m1, int len2, const uint32_t* m2,
                          const char* names1, const char* names2, const gm_pair_opts_t* opts, char** sam, size_t* sam_len, gm_map_stats_t* stats,
                          const char* quals1 = nullptr, const char* quals2 = nullptr, int qual_delta = 33,
                          const uint8_t* initbp1 = nullptr, const uint8_t* initbp2 = nullptr, uint32_t* per_pair_bytes = nullptr) {
  if (!s || n_pairs < 0 || len1 < 1 || len2 < 1 || (n_pairs > 0 && (!m1 || !m2))) { gm_set_error("gm_map_pairs: bad arguments"); return GM_E_ARG; }
  GmDevTurn dev_turn(s);
  PairRun R;
  int rc = R.init(s, n_pairs, len1, m1, len2, m2, names1, names2, opts, stats, quals1, quals2, qual_delta, initbp1, initbp2, per_pair_bytes); if (rc) return rc;
  for (int k = 0; k < 2; k++) for (int m = 0; m < 2; m++) R.dkm[k][m] = R.dvm[m];
  int cur = 0, front_n = 0, out_idx = 0; bool have_front = false;
  for (int base = 0; base < n_pairs;) {
    const int B = std::min(R.PS[cur][0]->eff_batch, R.PS[cur][1]->eff_batch);
    const int n = have_front ? front_n : std::min(B, n_pairs - base);
    rc = R.use_pair(cur, B); if (rc) return rc;
    if (!have_front) { rc = R.front(cur, base, n); if (rc) return rc; }
    bool have_next = false; int next_n = 0;
    if (R.overlap && base + n < n_pairs) {
      next_n = std::min(std::min(R.PS[cur ^ 1][0]->eff_batch, R.PS[cur ^ 1][1]->eff_batch), n_pairs - (base + n));
      rc = R.front(cur ^ 1, base + n, next_n); if (rc) return rc;
      have_next = true;
    }
    auto b = std::make_shared<PairOut>(); PairSel t;
    const int pinset = (out_idx & 1) * 4;
    b->base = base; b->n = n; b->resP = &s->pin_res[pinset]; b->opsP = &s->pin_ops[pinset]; b->resU = &s->pin_res[pinset + 2]; b->opsU = &s->pin_ops[pinset + 2];
    for (int m = 0; m < 2; m++) b->ops_stride[m] = R.S[m]->ops_stride;
    rc = R.finish_front(n);
    if (!rc) rc = R.pass1_select(n, t.n_work);
    if (!rc) rc = R.paired_pass2(*b, t);
    if (!rc) { R.select_pairs_host(*b, t); rc = R.rescue(*b, t); }
    if (rc == GM_REDO) { rc = R.redo(); if (rc) return rc; have_front = false; continue; }
    if (!rc) rc = R.collect_stats();
    if (rc) return rc;
    R.start_output(b); out_idx++;
    base += n;
    if (R.overlap) cur ^= 1;
    have_front = have_next; front_n = next_n;
  }
  R.finish_pending();
  if (R.out_failed) { gm_set_error("gm_map_pairs: out of memory in the output stage"); return GM_E_NOMEM; }
  if (stats) { stats->reads = 2ull * (uint64_t)n_pairs; stats->reads_matched = R.matched; stats->sam_records = R.records; }
  size_t total = 0; for (auto& p : R.pieces_all) total += p.size();
  if (sam) {
    size_t cap = 0; char* r = g_outcache.take(total + 1, &cap);      // the text buffer of the last call, if it was given back (gm_free parks large ones)
    if (!r) { cap = total + 1 + total / 16; r = (char*)malloc(cap); }      // (some room: the next call's text is a little longer half of the time, and a parked buffer that is too small is a fresh one's page faults)
    if (!r) return GM_E_NOMEM;
    g_outcache.track(r, cap);
    size_t o = 0; for (auto& p : R.pieces_all) { memcpy(r + o, p.data(), p.size()); o += p.size(); }
    r[total] = 0; *sam = r; if (sam_len) *sam_len = total;
  }
  return GM_OK;
}

extern "C" int gm_map_pairs_fastq(gm_session_t* s, int n_pairs, int len1, const uint32_t* mates1_packed, int len2, const uint32_t* mates2_packed,
                                  const char* names1, const char* names2, const char* quals1, const char* quals2, int qual_delta,
                                  const gm_pair_opts_t* opts, char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (!quals1 || !quals2) { gm_set_error("gm_map_pairs_fastq: no QUAL strings"); return GM_E_ARG; }
  if (s && s->P.colour_space) { gm_set_error("gm_map_pairs_fastq: quality values are not implemented for colour-space pairs"); return GM_E_ARG; }
  return map_pairs_impl(s, n_pairs, len1, mates1_packed, len2, mates2_packed, names1, names2, opts, sam, sam_len, stats, quals1, quals2, qual_delta);
}
// Colour-space pairs (the gmapper-cs binary with -p opp-in): mates as packed colours plus one primer-letter byte per read, as gm_map_reads_cs takes them
extern "C" int gm_map_pairs_cs(gm_session_t* s, int n_pairs, int len1, const uint32_t* mates1_packed, const uint8_t* initbp1, int len2, const uint32_t* mates2_packed,
                               const uint8_t* initbp2, const char* names1, const char* names2, const gm_pair_opts_t* opts, char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (s && !s->P.colour_space) { gm_set_error("gm_map_pairs_cs: the session is in letter space"); return GM_E_ARG; }
  return map_pairs_impl(s, n_pairs, len1, mates1_packed, len2, mates2_packed, names1, names2, opts, sam, sam_len, stats, nullptr, nullptr, 33, initbp1, initbp2);
}
extern "C" int gm_map_pairs_cs_fastq(gm_session_t* s, int n_pairs, int len1, const uint32_t* mates1_packed, const uint8_t* initbp1, int len2, const uint32_t* mates2_packed,
                                     const uint8_t* initbp2, const char* names1, const char* names2, const char* quals1, const char* quals2, int qual_delta,
                                     const gm_pair_opts_t* opts, char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (s && !s->P.colour_space) { gm_set_error("gm_map_pairs_cs_fastq: the session is in letter space"); return GM_E_ARG; }
  if (!quals1 || !quals2) { gm_set_error("gm_map_pairs_cs_fastq: no QUAL strings"); return GM_E_ARG; }
  return map_pairs_impl(s, n_pairs, len1, mates1_packed, len2, mates2_packed, names1, names2, opts, sam, sam_len, stats, quals1, quals2, qual_delta, initbp1, initbp2);
}
// (gm_map_pairs_file / gm_map_pairs_file_cb: gm_host_files.inc)
extern "C" int gm_map_pairs(gm_session_t* s, int n_pairs, int len1, const uint32_t* mates1_packed, int len2, const uint32_t* mates2_packed,
                            const char* names1, const char* names2, const gm_pair_opts_t* opts, char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (s && s->P.colour_space) { gm_set_error("gm_map_pairs: a colour-space session takes its pairs through gm_map_pairs_cs (primer letters)"); return GM_E_ARG; }
  return map_pairs_impl(s, n_pairs, len1, mates1_packed, len2, mates2_packed, names1, names2, opts, sam, sam_len, stats);
}
