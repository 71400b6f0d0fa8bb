// gm_host_seams.inc -- the seams on caller bitfields: S1 (sw_vector*, sw_gapless*), S2 (sw_full_ls / sw_full_cs, gm_sw_full_batch_strings), S3 (post_sw) with their
// per-thread states, the launch planners (swf_plan, post_plan) and swf_rec_check; part of gm_host.hip.  The batch forms of S2 / S3 share their bodies with the _ix
// entries and stand beside them in gm_host_seams_ix.inc.

// ---- S1: vector SW on caller bitfields ----------------------------------------------------------
struct SwVecState { bool init = false, colours = false; GmScoreDev sc; int dblen = 0, qrlen = 0; uint64_t invocs = 0, cells = 0; double secs = 0; };
static thread_local SwVecState g_sv;

extern "C" int sw_vector_setup(int dblen, int qrlen, int a_gap_open, int a_gap_ext, int b_gap_open, int b_gap_ext,
                               int match, int mismatch, int use_colours, bool reset_stats) {
  if (match * qrlen >= 32768) { gm_set_error("match * qrlen >= 32768 (ref: sw-vector.c:393-398)"); return GM_E_RANGE; }
  if (gm_device_count() < 1) { gm_set_error("no HIP device"); return GM_E_NODEVICE; }
  gm_params_t P; gm_params_default(&P);
  P.match_score = match; P.mismatch_score = mismatch; P.a_gap_open_score = a_gap_open; P.a_gap_extend_score = a_gap_ext;
  P.b_gap_open_score = b_gap_open; P.b_gap_extend_score = b_gap_ext;
  g_sv.sc = make_score(P); g_sv.dblen = dblen; g_sv.qrlen = qrlen; g_sv.init = true; g_sv.colours = use_colours != 0;
  if (reset_stats) { g_sv.invocs = g_sv.cells = 0; g_sv.secs = 0; }
  return 0;
}
extern "C" int sw_vector_cleanup(void) { g_sv.init = false; return 0; }
extern "C" void sw_vector_stats(uint64_t* invocs, uint64_t* cells, double* secs) {
  if (invocs) *invocs = g_sv.invocs; if (cells) *cells = g_sv.cells; if (secs) *secs = g_sv.secs;
}

static int sw_vector_batch_impl(int n, const uint32_t* genome, uint64_t genome_words, const int64_t* g_off, const int* glen,
                                const uint32_t* reads, int read_words, const int* rlen, int* scores, int early_thr, uint8_t* stopped) {
  if (!g_sv.init) { gm_set_error("sw_vector called before sw_vector_setup"); return GM_E_NOTSETUP; }
  if (n <= 0) return GM_OK;
  int max_g = 0, max_r = 0;
  for (int i = 0; i < n; i++) { max_g = std::max(max_g, glen[i]); max_r = std::max(max_r, rlen[i]); if (glen[i] < 1 || rlen[i] < 1) return GM_E_ARG; }
  if (max_g > g_sv.dblen || max_r > g_sv.qrlen) { gm_set_error("window/read longer than sw_vector_setup sizes"); return GM_E_ARG; }
  GmDevMem mem; uint32_t *dg = nullptr, *dr = nullptr; long long* dgo = nullptr; int *dgl = nullptr, *drl = nullptr, *ds = nullptr; uint8_t* dst = nullptr;
  GM_HIP(mem.get(&dg, (genome_words + 8) * 4)); GM_HIP(hipMemset(dg, 0, (genome_words + 8) * 4)); GM_HIP(hipMemcpy(dg, genome, genome_words * 4, hipMemcpyHostToDevice));
  GM_HIP(mem.up(&dr, reads, (size_t)n * read_words, gm_sync, 32)); GM_HIP(mem.up(&dgo, g_off, n, gm_sync)); GM_HIP(mem.up(&dgl, glen, n, gm_sync)); GM_HIP(mem.up(&drl, rlen, n, gm_sync));
  GM_HIP(mem.get(&ds, (size_t)n * 4)); if (stopped) GM_HIP(mem.get(&dst, (size_t)n));
  // (the early stop needs a scheme in which a cell gains at most `match` and gaps cost: otherwise every window runs to its end)
  const GmScoreDev& sv = g_sv.sc;
  if (!(sv.match > 0 && sv.mismatch <= sv.match && sv.a_go >= 0 && sv.a_ge >= 0 && sv.b_go >= 0 && sv.b_ge >= 0 && sv.match * (2 * 128 + 2) < 32000)) early_thr = 0;
  int rc = gm_launch_sw_vector_batch(g_sv.sc, n, dg, dgo, dgl, dr, read_words, drl, max_g, max_r, ds, 0, early_thr, dst);
  if (rc == GM_OK) {
    GM_HIP(hipDeviceSynchronize()); GM_HIP(hipMemcpy(scores, ds, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (stopped) GM_HIP(hipMemcpy(stopped, dst, (size_t)n, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < n; i++) { g_sv.invocs++; g_sv.cells += (uint64_t)glen[i] * rlen[i]; }
  return rc;
}
extern "C" int gm_sw_vector_batch(int n, const uint32_t* genome, uint64_t genome_words, const int64_t* g_off, const int* glen,
                                  const uint32_t* reads, int read_words, const int* rlen, int* scores) {
  return sw_vector_batch_impl(n, genome, genome_words, g_off, glen, reads, read_words, rlen, scores, 0, nullptr);
}
extern "C" int gm_sw_vector_batch_bounded(int n, const uint32_t* genome, uint64_t genome_words, const int64_t* g_off, const int* glen,
                                          const uint32_t* reads, int read_words, const int* rlen, int threshold, int* scores, uint8_t* stopped) {
  if (threshold <= 0 || !stopped) { gm_set_error("gm_sw_vector_batch_bounded: threshold > 0 and a stopped[] array are required"); return GM_E_ARG; }
  return sw_vector_batch_impl(n, genome, genome_words, g_off, glen, reads, read_words, rlen, scores, threshold, stopped);
}

extern "C" int sw_vector(uint32_t* genome, int goff, int glen, uint32_t* read, int rlen, uint32_t* genome_ls, int initbp, bool is_rna) {
  if (!g_sv.init) abort();   // ref: sw-vector.c:462-463
  // is_rna only matters to the colour-space first-colour row (lstocs(genome_ls[j], initbp, is_rna), ref: sw-vector.c:129,289): it rides in bit 8 of the primer word
  if (is_rna && genome_ls) initbp |= GM_SEAM_RNA;
  int64_t go = goff; int score = 0;
  const uint64_t gw = ((uint64_t)goff + glen + 7) / 8;
  if (g_sv.colours) {        // colour space: genome = colours, genome_ls = letters of the same contig (ref: sw-vector.c:476-479)
    if (!genome_ls) { gm_set_error("sw_vector: colour space needs genome_ls"); return GM_E_ARG; }
    int rc = gm_sw_vector_batch_cs(1, genome, genome_ls, gw, &go, &glen, read, (rlen + 7) / 8, &rlen, &initbp, &score);
    return rc == GM_OK ? score : rc;
  }
  int rc = gm_sw_vector_batch(1, genome, gw, &go, &glen, read, (rlen + 7) / 8, &rlen, &score);
  return rc == GM_OK ? score : rc;
}

// ---- S1, ungapped: sw_gapless on caller bitfields (ref: common/sw-gapless.h:11-14, sw-gapless.c:29-117) -----------------------------
// What f1_setup / f1_run call when gapless_sw is set (ref: f1-wrapper.h:66-68,122-125).  State per calling thread, like the reference's threadprivate statics.
struct SwGaplessState { bool init = false; int match = 0, mismatch = 0; uint64_t invocs = 0, cells = 0, ticks = 0; };
static thread_local SwGaplessState g_sg;
extern "C" int sw_gapless_setup(int match, int mismatch, bool reset_stats) {
  if (gm_device_count() < 1) { gm_set_error("no HIP device"); return GM_E_NODEVICE; }
  g_sg.match = match; g_sg.mismatch = mismatch; g_sg.init = true;
  if (reset_stats) g_sg.invocs = g_sg.cells = g_sg.ticks = 0;
  return 0;
}
extern "C" void sw_gapless_stats(uint64_t* invocs, uint64_t* cells, uint64_t* ticks) {      // (ticks: nanoseconds spent inside sw_gapless on this thread; the reference counts rdtsc ticks)
  if (invocs) *invocs = g_sg.invocs; if (cells) *cells = g_sg.cells; if (ticks) *ticks = g_sg.ticks;
}
// n independent calls; call i's genome bitfield starts at word genome_woff[i] of `genome` (and of `genome_ls`, colour space only: then `genome` holds colours,
// `genome_ls` the letters of the same contig and initbp[i] the read's primer letter) and holds glen[i] positions
extern "C" int gm_sw_gapless_batch(int n, const uint32_t* genome, const uint32_t* genome_ls, uint64_t genome_words, const int64_t* genome_woff, const int* glen,
                                   const uint32_t* reads, int read_words, const int* rlen, const int* g_idx, const int* r_idx, const int* initbp, int* scores) {
  if (!g_sg.init) { gm_set_error("sw_gapless called before sw_gapless_setup"); return GM_E_NOTSETUP; }
  if (n <= 0) return GM_OK;
  if (genome_ls && !initbp) { gm_set_error("gm_sw_gapless_batch: colour space needs initbp"); return GM_E_ARG; }
  int max_r = 0;
  for (int i = 0; i < n; i++) {
    if (glen[i] < 1 || rlen[i] < 1 || g_idx[i] < 0 || r_idx[i] < 0 || g_idx[i] >= glen[i] || r_idx[i] >= rlen[i] || genome_woff[i] < 0 ||
        (uint64_t)genome_woff[i] + ((uint64_t)glen[i] + 7) / 8 > genome_words || (rlen[i] + 7) / 8 > read_words) { gm_set_error("gm_sw_gapless_batch: call %d out of range", i); return GM_E_ARG; }
    max_r = std::max(max_r, rlen[i]);
  }
  const auto t0 = std::chrono::steady_clock::now();
  GmDevMem mem;
  uint32_t *dg = nullptr, *dgl = nullptr, *dr = nullptr; long long* dwo = nullptr; int *dn = nullptr, *drl = nullptr, *dgi = nullptr, *dri = nullptr, *dib = nullptr, *ds = nullptr;
  GM_HIP(mem.get(&dg, (genome_words + 8) * 4)); GM_HIP(hipMemset(dg, 0, (genome_words + 8) * 4)); GM_HIP(hipMemcpy(dg, genome, genome_words * 4, hipMemcpyHostToDevice));
  if (genome_ls) { GM_HIP(mem.get(&dgl, (genome_words + 8) * 4)); GM_HIP(hipMemset(dgl, 0, (genome_words + 8) * 4)); GM_HIP(hipMemcpy(dgl, genome_ls, genome_words * 4, hipMemcpyHostToDevice)); }
  GM_HIP(mem.up(&dr, reads, (size_t)n * read_words, gm_sync, 32)); GM_HIP(mem.up(&dwo, genome_woff, n, gm_sync));
  int** const dst[5] = {&dn, &drl, &dgi, &dri, &dib}; const int* const src[5] = {glen, rlen, g_idx, r_idx, initbp};
  for (int k = 0; k < 5; k++) GM_HIP(mem.up(dst[k], src[k], n, gm_sync));      // (initbp is absent in letter space)
  GM_HIP(mem.get(&ds, (size_t)n * 4));
  int rc = gm_launch_sw_gapless_batch(n, g_sg.match, g_sg.mismatch, dg, dgl, dwo, dn, dr, read_words, drl, dgi, dri, dib, max_r, ds, 0);
  if (rc == GM_OK) { GM_HIP(hipDeviceSynchronize()); GM_HIP(hipMemcpy(scores, ds, (size_t)n * 4, hipMemcpyDeviceToHost)); }
  if (rc == GM_OK) {                                                                             // (a failed launch scored nothing: it does not count)
    for (int i = 0; i < n; i++) { g_sg.invocs++; g_sg.cells += (uint64_t)rlen[i]; }              // ref: sw-gapless.c:111 (cells += rlen)
    g_sg.ticks += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  }
  return rc;
}
extern "C" int sw_gapless(uint32_t* genome, int glen, uint32_t* read, int rlen, int g_idx, int r_idx, uint32_t* genome_ls, int init_bp, bool is_rna) {
  if (!g_sg.init) abort();   // ref: sw-gapless.c:66-67
  if (is_rna && genome_ls) init_bp |= GM_SEAM_RNA;      // lstocs(letter, init_bp, is_rna), ref: sw-gapless.c:84
  int64_t wo = 0; int score = 0;
  int rc = gm_sw_gapless_batch(1, genome, genome_ls, ((uint64_t)glen + 7) / 8, &wo, &glen, read, (rlen + 7) / 8, &rlen, &g_idx, &r_idx, genome_ls ? &init_bp : nullptr, &score);
  return rc == GM_OK ? score : rc;
}

// ---- S2: full SW on caller bitfields ------------------------------------------------------------
struct SwFullState { bool init = false; GmScoreDev sc; int dblen = 0, qrlen = 0; uint64_t invocs = 0, cells = 0; double secs = 0; };
static thread_local SwFullState g_sf;
static const char LSTRANS[17] = "ACGTUMRWSYKVHDBN";   // base_translate, ref: common/fasta.c:689-690

extern "C" int sw_full_ls_setup(int dblen, int qrlen, int a_gap_open, int a_gap_ext, int b_gap_open, int b_gap_ext,
                                int match, int mismatch, bool reset_stats, int anchor_width) {
  if (gm_device_count() < 1) { gm_set_error("no HIP device"); return GM_E_NODEVICE; }
  if (const int rc = gm_check_anchor_width("sw_full_ls_setup", anchor_width)) return rc;
  gm_params_t P; gm_params_default(&P);
  P.match_score = match; P.mismatch_score = mismatch; P.a_gap_open_score = a_gap_open; P.a_gap_extend_score = a_gap_ext;
  P.b_gap_open_score = b_gap_open; P.b_gap_extend_score = b_gap_ext; P.anchor_width = anchor_width;
  g_sf.sc = make_score(P); g_sf.dblen = dblen; g_sf.qrlen = qrlen; g_sf.init = true;
  if (reset_stats) { g_sf.invocs = g_sf.cells = 0; g_sf.secs = 0; }
  return 0;
}
extern "C" int sw_full_ls_cleanup(void) { g_sf.init = false; return 0; }
// invocations, cells (window x read, the upper bound of the band the reference counts, ref: sw-full-ls.c:237) and seconds spent inside sw_full_ls on this thread
extern "C" void sw_full_ls_stats(uint64_t* invocs, uint64_t* cells, double* secs) {
  if (invocs) *invocs = g_sf.invocs; if (cells) *cells = g_sf.cells; if (secs) *secs = g_sf.secs;
}
struct SeamTimer { double* acc; std::chrono::steady_clock::time_point t0; explicit SeamTimer(double* a) : acc(a), t0(std::chrono::steady_clock::now()) {}
                   ~SeamTimer() { *acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } };

// sw_full_ls / sw_full_cs are calls of one item of the batch body (sw_full_batch_impl, gm_host_seams_ix.inc) and take their strings from gm_sw_full_batch_strings.  `seam`:
// the seam counts and times the call itself (one invocation, window x read cells, also when it refuses), and an anchor box is taken as given, whatever its length.
static int sw_full_batch_impl(bool colour, int n, const uint32_t* genome, uint64_t genome_words, const int64_t* g_off, const int* glen, const uint32_t* reads, int read_words,
                              const int* rlen, const uint8_t* initbp, const struct gm_anchor* anchors, const uint8_t* revcmpl, const int* threshscore, const int* maxscore,
                              const int* xover, int xover_stride, int is_rna, int local, gm_sw_full_rec_t* recs, uint8_t** ops, uint64_t* ops_len,
                              const gm_index_t* ix = nullptr, const int* cn = nullptr, const uint8_t* gen_st = nullptr, bool seam = false);

extern "C" void sw_full_ls(uint32_t* genome, int goff, int glen, uint32_t* read, int rlen, int threshscore, int maxscore,
                           struct gm_sw_full_results* sfr, bool revcmpl, struct gm_anchor* anchors, int anchors_cnt, int local_alignment) {
  if (!g_sf.init) abort();   // ref: sw-full-ls.c:649-650
  SeamTimer tm(&g_sf.secs); g_sf.invocs++; g_sf.cells += (uint64_t)std::max(glen, 0) * (uint64_t)std::max(rlen, 0);
  if ((anchors != nullptr && anchors_cnt != 1) || glen > g_sf.dblen || rlen > g_sf.qrlen || glen < 1 || rlen < 1) {
    gm_set_error("sw_full_ls: one anchor box (gmapper's call, ref: mapping.c:391-394) or none (the threshold band) is implemented");
    sfr->score = 0; sfr->dbalign = strdup(""); sfr->qralign = strdup(""); return;
  }
  const int64_t go = goff; const uint8_t rv = revcmpl ? 1 : 0;
  gm_sw_full_rec_t R; uint8_t* ops = nullptr; uint64_t ops_len = 0;
  // (the genome bitfield ends with the window's last word; any failure below: score 0, empty strings, the reason in gm_last_error())
  const bool ok = sw_full_batch_impl(false, 1, genome, ((uint64_t)goff + glen + 7) / 8, &go, &glen, read, (rlen + 7) / 8, &rlen, nullptr, anchors, &rv, &threshscore, &maxscore,
                                     nullptr, 0, 0, local_alignment, &R, &ops, &ops_len, nullptr, nullptr, nullptr, true) == GM_OK && R.status == 0 &&
                  gm_sw_full_batch_strings(0, &R, ops, ops_len, genome, (uint64_t)goff + glen, read, rlen, 0, 0, &sfr->dbalign, &sfr->qralign) == GM_OK;
  free(ops);
  if (!ok) { sfr->score = 0; sfr->dbalign = strdup(""); sfr->qralign = strdup(""); return; }
  sfr->score = R.score;
  if (R.score > 0) {
    sfr->read_start = R.read_start; sfr->rmapped = R.rmapped; sfr->genome_start = (int)R.genome_start; sfr->gmapped = R.gmapped;      // (genome_start includes goff)
    sfr->matches += R.matches; sfr->mismatches += R.mismatches; sfr->insertions += R.insertions; sfr->deletions += R.deletions;
  } else {   // the reference backtraces stale scratch here; every caller discards it (score 0 < threshold)
    sfr->rmapped = 1; sfr->gmapped = 1; sfr->genome_start = goff;
  }
}

extern "C" int gm_sw_vector_batch_cs(int n, const uint32_t* genome_cs, const uint32_t* genome_ls, uint64_t genome_words, const int64_t* g_off,
                                     const int* glen, const uint32_t* reads, int read_words, const int* rlen, const int* initbp, int* scores) {
  if (!g_sv.init) { gm_set_error("sw_vector called before sw_vector_setup"); return GM_E_NOTSETUP; }
  if (n <= 0) return GM_OK;
  int max_g = 0, max_r = 0;
  for (int i = 0; i < n; i++) { max_g = std::max(max_g, glen[i]); max_r = std::max(max_r, rlen[i]); if (glen[i] < 1 || rlen[i] < 1 || initbp[i] < 0 || (initbp[i] & ~GM_SEAM_RNA) > 3) return GM_E_ARG; }
  if (max_g > g_sv.dblen || max_r > g_sv.qrlen) { gm_set_error("window/read longer than sw_vector_setup sizes"); return GM_E_ARG; }
  uint32_t *dgc = nullptr, *dgl = nullptr, *dr = nullptr; long long* dgo = nullptr; int *dgn = nullptr, *drl = nullptr, *dib = nullptr, *ds = nullptr;
  GmDevMem mem; GM_HIP(mem.get(&dgc, (genome_words + 8) * 4)); GM_HIP(mem.get(&dgl, (genome_words + 8) * 4));
  GM_HIP(hipMemset(dgc, 0, (genome_words + 8) * 4)); GM_HIP(hipMemset(dgl, 0, (genome_words + 8) * 4));
  GM_HIP(hipMemcpy(dgc, genome_cs, genome_words * 4, hipMemcpyHostToDevice)); GM_HIP(hipMemcpy(dgl, genome_ls, genome_words * 4, hipMemcpyHostToDevice));
  GM_HIP(mem.up(&dr, reads, (size_t)n * read_words, gm_sync, 32)); GM_HIP(mem.up(&dgo, g_off, n, gm_sync)); GM_HIP(mem.up(&dgn, glen, n, gm_sync));
  GM_HIP(mem.up(&drl, rlen, n, gm_sync)); GM_HIP(mem.up(&dib, initbp, n, gm_sync)); GM_HIP(mem.get(&ds, (size_t)n * 4));
  int rc = gm_launch_sw_vector_batch_cs(g_sv.sc, n, dgc, dgl, dgo, dgn, dr, read_words, drl, dib, max_g, max_r, ds, 0);
  if (rc == GM_OK) { GM_HIP(hipDeviceSynchronize()); GM_HIP(hipMemcpy(scores, ds, (size_t)n * 4, hipMemcpyDeviceToHost)); }
  for (int i = 0; i < n; i++) { g_sv.invocs++; g_sv.cells += (uint64_t)glen[i] * rlen[i]; }
  return rc;
}

// ---- S2 in colour space: sw_full_cs on caller bitfields (ref: common/sw-full-cs.c:1084-1236) --------------
struct SwFullCsState { bool init = false; int p[9]; int dblen = 0, qrlen = 0; uint64_t invocs = 0, cells = 0; double secs = 0; };
static thread_local SwFullCsState g_sc;
extern "C" int sw_full_cs_setup(int dblen, int qrlen, int a_gap_open, int a_gap_ext, int b_gap_open, int b_gap_ext,
                                int match, int mismatch, int global_xover_penalty, bool reset_stats, int anchor_width, int indel_taboo_len) {
  if (reset_stats) { g_sc.invocs = g_sc.cells = 0; g_sc.secs = 0; }
  if (gm_device_count() < 1) { gm_set_error("no HIP device"); return GM_E_NODEVICE; }
  if (const int rc = gm_check_anchor_width("sw_full_cs_setup", anchor_width)) return rc;
  const int p[9] = {match, mismatch, global_xover_penalty, -a_gap_open, -a_gap_ext, -b_gap_open, -b_gap_ext, anchor_width, indel_taboo_len};
  memcpy(g_sc.p, p, sizeof p); g_sc.dblen = dblen; g_sc.qrlen = qrlen; g_sc.init = true;
  return 0;
}
extern "C" int sw_full_cs_cleanup(void) { g_sc.init = false; return 0; }
extern "C" void sw_full_cs_stats(uint64_t* invocs, uint64_t* cells, double* secs) {   // ref: sw-full-cs.c:1127-1140 (cells: window x read x 4 layers here)
  if (invocs) *invocs = g_sc.invocs; if (cells) *cells = g_sc.cells; if (secs) *secs = g_sc.secs;
}

extern "C" void sw_full_cs(uint32_t* genome_ls, int goff, int glen, uint32_t* read, int rlen, int initbp, int threshscore,
                           struct gm_sw_full_results* sfr, bool revcmpl, bool is_rna, struct gm_anchor* anchors, int anchors_cnt,
                           int local_alignment, int* crossover_score) {
  if (!g_sc.init) abort();   // ref: sw-full-cs.c:1155-1156
  SeamTimer tm(&g_sc.secs); g_sc.invocs++; g_sc.cells += 4ull * (uint64_t)std::max(glen, 0) * (uint64_t)std::max(rlen, 0);
  // A refusal must not read as "no alignment" (score 0 is what a window below the threshold returns): the reason goes to stderr as well as to gm_last_error().
  auto fail = [&](const char* why) { gm_set_error("sw_full_cs: %s", why); fprintf(stderr, "gmapper_hip: sw_full_cs refused: %s\n", why); sfr->score = 0; sfr->dbalign = nullptr; sfr->qralign = nullptr; };
  // ... and where the batch body or a launcher has refused, its reason stands as it is ("sw_full_cs: item 0 refused: ...", or what the failing call left)
  auto refused = [&] { fprintf(stderr, "gmapper_hip: %s\n", gm_last_error()); sfr->score = 0; sfr->dbalign = nullptr; sfr->qralign = nullptr; };
  if ((anchors == nullptr ? g_sc.p[7] >= 0 : anchors_cnt != 1) || glen > g_sc.dblen || rlen > g_sc.qrlen || glen < 1 || rlen < 1 ||
      initbp < 0 || initbp > 3) {
    fail("only one anchor box (gmapper's call, ref: mapping.c:375-379) is implemented -- or none under anchor_width -1, the threshold band"); return;
  }
  // crossover_score: one score per read position (from the QVs, ref: gmapper.c:532-544 -- clamped there to [2 * global, -1]); the kernels keep a row of them in 8 bits,
  // and the batch body refuses a score outside them as this seam always has (a window that does not fit LDS likewise: same formula, same limit)
  const int64_t go = goff; const uint8_t rv = revcmpl ? 1 : 0, ib = (uint8_t)initbp;
  gm_sw_full_rec_t R; uint8_t* ops = nullptr; uint64_t ops_len = 0;
  const int rc = sw_full_batch_impl(true, 1, genome_ls, ((uint64_t)goff + glen + 7) / 8, &go, &glen, read, (rlen + 7) / 8, &rlen, &ib, anchors, &rv, &threshscore, nullptr,
                                    crossover_score, rlen, is_rna ? 1 : 0, local_alignment, &R, &ops, &ops_len, nullptr, nullptr, nullptr, true);
  if (rc == GM_OK && R.status == 0 && R.score > 0 &&
      gm_sw_full_batch_strings(1, &R, ops, ops_len, genome_ls, (uint64_t)goff + glen, read, rlen, initbp, is_rna ? 1 : 0, &sfr->dbalign, &sfr->qralign) == GM_OK) {
    sfr->score = R.score; sfr->read_start = R.read_start; sfr->rmapped = R.rmapped; sfr->genome_start = (int)R.genome_start; sfr->gmapped = R.gmapped;
    sfr->matches += R.matches; sfr->mismatches += R.mismatches; sfr->insertions += R.insertions; sfr->deletions += R.deletions; sfr->crossovers += R.crossovers;
  } else if (rc == GM_OK && R.status == 0 && R.score <= 0) { sfr->score = 0; sfr->dbalign = nullptr; sfr->qralign = nullptr; }      // below threshold: no strings (ref :1224-1226)
  else refused();
  free(ops);
}

// ---- S2 batch: gm_sw_full_ls_batch / gm_sw_full_cs_batch -----------------------------------------------------------------------------
// One call = a fixed number of device buffers (genome, reads, items, results, ops, back-pointer scratch, crossover rows), copies and launches.  The scratch is
// grid x (largest glen x rlen of the launch), never the sum over the items; when that passes GM_SWF_BACK_BUDGET with the grid the items would fill, the items are
// sorted into at most three launches by matrix size (so that a few large windows do not starve the many small ones of waves) that share the one scratch.
static const size_t GM_SWF_BACK_BUDGET = (size_t)512 << 20;
static const int GM_SWF_MAX_GRID = 2048;
struct SwfLaunch { int first = 0, count = 0, grid = 0, max_g = 0, max_r = 0; size_t stride = 0; };
// items (accepted ones only) are reordered by class; unit = scratch bytes a cell; *pool = bytes of the shared scratch
static void swf_plan(std::vector<GmFullItem>& items, size_t unit, std::vector<SwfLaunch>& launches, size_t* pool) {
  launches.clear(); *pool = 0;
  if (items.empty()) return;
  auto cells = [](const GmFullItem& it) { return (size_t)it.glen * (size_t)it.rlen; };
  size_t M = 0; for (const GmFullItem& it : items) M = std::max(M, cells(it));
  int want = (int)std::min<size_t>(items.size(), (size_t)GM_SWF_MAX_GRID);
  if (gm_tune("GM_SWF_SLOTS") && atoi(gm_tune("GM_SWF_SLOTS")) > 0) want = std::min(want, atoi(gm_tune("GM_SWF_SLOTS")));      // (tuning build: few slots, i.e. many items of all shapes through each)
  std::vector<size_t> bound;                                  // a class takes the items of at most this many cells that no earlier class took
  if ((size_t)want * (M * unit + 256) > GM_SWF_BACK_BUDGET) { bound = {M / 64, M / 8, M}; } else bound = {M};
  std::vector<GmFullItem> sorted; sorted.reserve(items.size());
  size_t lo = 0;
  for (size_t b : bound) {
    SwfLaunch L; L.first = (int)sorted.size(); size_t mc = 0;
    for (const GmFullItem& it : items) { const size_t c = cells(it); if (c > lo && c <= b) { sorted.push_back(it); mc = std::max(mc, c); L.max_g = std::max(L.max_g, it.glen); L.max_r = std::max(L.max_r, it.rlen); } }
    lo = b;
    L.count = (int)sorted.size() - L.first;
    if (!L.count) continue;
    L.stride = (mc * unit + 256 + 15) & ~(size_t)15;
    L.grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(want, L.count), GM_SWF_BACK_BUDGET / L.stride));
    *pool = std::max(*pool, (size_t)L.grid * L.stride);
    launches.push_back(L);
  }
  items.swap(sorted);
}
static inline int swf_nib(const uint32_t* b, long long i) { return (int)((b[i / 8] >> (4 * (i % 8))) & 0xf); }

// What gm_sw_full_batch_strings and gm_post_sw_batch check of a batch record before anything is read through it: its operations lie inside the ops buffer, the
// alignment inside the genome (genome_len positions) and the read (rlen positions), and in colour space every operation byte is of the encoding (low nibble 1..9).
// Returns the reason, or null; *read_positions = the columns that hold a read position.
static const char* swf_rec_check(bool colour_space, const gm_sw_full_rec_t* rec, const uint8_t* ops, uint64_t ops_len, uint64_t genome_len, int rlen, uint64_t* read_positions) {
  if (rec->ops_off > ops_len || rec->n_ops > ops_len - rec->ops_off || rec->genome_start < 0 || rec->read_start < 0 || rlen < 0)
    return "the record points outside the ops buffer or the bitfields";
  const uint8_t* o = ops + rec->ops_off;
  uint64_t adv_g = 0, adv_r = 0; bool coded = true;
  for (uint32_t k = 0; k < rec->n_ops; k++) {
    const int type = o[k] & 0x0f;
    const bool ins = colour_space ? type == 1 : o[k] == 'I', del = colour_space ? (type >= 2 && type <= 5) : o[k] == 'D';
    if (!del) adv_g++; if (!ins) adv_r++;
    if (colour_space && (type < 1 || type > 9)) coded = false;
  }
  if ((uint64_t)rec->genome_start + adv_g > genome_len || (uint64_t)rec->read_start + adv_r > (uint64_t)rlen) return "the record's alignment runs past the genome or the read";
  if (!coded) return "an operation byte that is none of the encoding";
  if (read_positions) *read_positions = adv_r;
  return nullptr;
}
// pretty_print of one batch item (ref: sw-full-ls.c:524-560, sw-full-cs.c:945-1060), as sw_full_ls / sw_full_cs above build their strings.  Host only.
extern "C" int gm_sw_full_batch_strings(int colour_space, const gm_sw_full_rec_t* rec, const uint8_t* ops, uint64_t ops_len, const uint32_t* genome, uint64_t genome_len,
                                        const uint32_t* read, int rlen_in, int initbp, int is_rna, char** dbalign, char** qralign) {
  if (!rec || !dbalign || !qralign) { gm_set_error("gm_sw_full_batch_strings: a required argument is missing"); return GM_E_ARG; }
  *dbalign = *qralign = nullptr;
  const bool aligned = rec->status == 0 && rec->score > 0;
  if (!aligned) { if (!colour_space) { *dbalign = strdup(""); *qralign = strdup(""); } return GM_OK; }
  if (!ops || !genome || !read || (colour_space && (initbp < 0 || initbp > 3))) { gm_set_error("gm_sw_full_batch_strings: a required argument is missing"); return GM_E_ARG; }
  if (const char* why = swf_rec_check(colour_space != 0, rec, ops, ops_len, genome_len, rlen_in, nullptr)) { gm_set_error("gm_sw_full_batch_strings: %s", why); return GM_E_ARG; }
  const uint8_t* o = ops + rec->ops_off;
  std::string db, q;
  long long pj = rec->genome_start; int pi = rec->read_start;
  if (!colour_space) {
    for (uint32_t k = 0; k < rec->n_ops; k++) {
      if (o[k] == 'D') { db.push_back('-'); q.push_back(LSTRANS[swf_nib(read, pi++)]); }
      else if (o[k] == 'I') { db.push_back(LSTRANS[swf_nib(genome, pj++)]); q.push_back('-'); }
      else { db.push_back(LSTRANS[swf_nib(genome, pj++)]); q.push_back(LSTRANS[swf_nib(read, pi++)]); }
    }
  } else {
    const int rlen = rlen_in;
    std::vector<uint8_t> qr[4];
    for (int k = 0; k < 4; k++) {
      qr[k].resize(rlen); int letter = (k + initbp) % 4;
      for (int j = 0; j < rlen; j++) {
        const int base = swf_nib(read, j);
        if (base == 15) { qr[k][j] = 15; letter = (k + initbp) % 4; }
        else {                                                   // cstols(letter, base, is_rna), ref: util.h:157-180
          const int lt = (is_rna && letter == 4) ? 3 : letter;
          int l2 = (lt % 2 == 0) ? ((4 + lt + base) % 4) : ((4 + lt - base) % 4); if (is_rna && l2 == 3) l2 = 4;
          qr[k][j] = (uint8_t)((letter == 15 || base > 3) ? 15 : l2); letter = qr[k][j];
        }
      }
    }
    for (uint32_t t = 0; t < rec->n_ops; t++) {
      const int type = o[t] & 0x0f; const bool xov = (o[t] & 0x80) != 0;
      if (type == 1) { db.push_back(LSTRANS[swf_nib(genome, pj++)]); q.push_back('-'); continue; }
      const bool del = type >= 2 && type <= 5;
      const int lay = del ? type - 2 : type - 6;
      char c = LSTRANS[qr[lay][pi++]];
      if (xov) c = (char)tolower((int)c);
      if (del) { db.push_back('-'); q.push_back(c); }
      else { const char d = LSTRANS[swf_nib(genome, pj++)]; if (c == 'n' || c == 'N') c = xov ? (char)tolower((int)d) : d; db.push_back(d); q.push_back(c); }
    }
  }
  *dbalign = strdup(db.c_str()); *qralign = strdup(q.c_str());
  return GM_OK;
}

// ---- S3: post_sw on a caller's sw_full_results (ref: common/sw-post.c:364-758, sw-post.h:6-9) ------------------------------------------
// The colour-space posterior of one alignment, host doubles through libm in the reference's operation order (cs_post_sw above, the routine the
// read pipeline uses).  State per calling thread, like the reference's threadprivate statics.
struct PostSwState { bool init = false; CsPostConsts K; bool use_read_qvs = false; int qual_delta = 33, max_len = 0; uint64_t invocs = 0, cells = 0; double secs = 0; };
static thread_local PostSwState g_ps;
extern "C" int post_sw_setup(int max_len, double pr_snp, double pr_xover, double pr_del_open, double pr_del_extend, double pr_ins_open, double pr_ins_extend,
                             bool use_read_qvs, bool use_sanger_qvs, int qual_vector_offset, int qual_delta, bool reset_stats) {
  g_ps.K = cs_post_consts_from(pr_snp, pr_xover, pr_del_open, pr_del_extend, pr_ins_open, pr_ins_extend, use_sanger_qvs, use_read_qvs ? qual_vector_offset : 0);
  g_ps.use_read_qvs = use_read_qvs; g_ps.qual_delta = qual_delta; g_ps.max_len = max_len; g_ps.init = true;
  if (reset_stats) { g_ps.invocs = g_ps.cells = 0; g_ps.secs = 0; }
  return 1;                                                  // the reference returns 1 (sw-post.c:441)
}
extern "C" int post_sw_cleanup(void) { g_ps.init = false; return 1; }
extern "C" int post_sw_stats(uint64_t* invocs, uint64_t* cells, double* secs) {
  if (invocs) *invocs = g_ps.invocs; if (cells) *cells = g_ps.cells; if (secs) *secs = g_ps.secs;
  return 1;
}
// read: the colour read as the reference's 4-bit bitfield; qual: its QV string (used when post_sw_setup got use_read_qvs); sfr: the result of
// sw_full_cs -- qralign is re-called in place, matches / mismatches / crossovers are recounted, qual (malloc) and posterior are filled.
extern "C" void post_sw(uint32_t* read, int initbp, char* qual, struct gm_sw_full_results* sfr) {
  if (!g_ps.init) abort();                                   // ref: sw-post.c:657-658
  if (!sfr || !sfr->dbalign || !sfr->qralign) abort();
  SeamTimer tm(&g_ps.secs); g_ps.invocs++;
  FHit h; h.db = sfr->dbalign; h.qr = sfr->qralign;
  cs_post_sw(g_ps.K, read, initbp, sfr->read_start, h, g_ps.use_read_qvs ? qual : nullptr, g_ps.qual_delta, true);
  size_t len = 0; for (char c : h.qr) len += c != '-';
  g_ps.cells += 16 * (uint64_t)len;
  memcpy(sfr->qralign, h.qr.data(), h.qr.size());
  sfr->matches = h.cs_match; sfr->mismatches = h.cs_mismatch; sfr->crossovers = h.cs_xover;
  sfr->qual = (char*)malloc(h.qr.size() + 1);
  if (sfr->qual) { memcpy(sfr->qual, h.qual.data(), h.qual.size()); sfr->qual[h.qual.size()] = 0; }
  sfr->posterior = h.posterior;
}

// ---- S3 batch: gm_post_sw_batch -- post_sw of n records of a gm_sw_full_cs_batch call in one go (k_post_sw_batch, gm_post.hip) --------------------------------
// A fixed number of device buffers, copies and launches whatever n is.  The column scratch (GM_POST_COL_BYTES a column) belongs to the thread slots of a launch and is
// sized by the launch's longest alignment; when the slots the items would fill pass GM_POST_BUDGET the thread count is lowered to fit, and the items are sorted into at
// most three launches by length (as swf_plan does by matrix size) so that one long alignment does not starve many short ones of threads.  A result the kernel flags
// (a letter call or a base quality the last bits of exp / log could decide) is redone by cs_post_sw on the strings rebuilt from the record: by_host = 1.
static const size_t GM_POST_BUDGET = (size_t)512 << 20;
struct PostLaunch { int first = 0, count = 0, threads = 0, max_len = 0; };
struct PostPlan { int n = 0; PostLaunch l[3]; };
static thread_local PostPlan g_post_plan;
static void post_plan(std::vector<GmPostItem>& items, std::vector<PostLaunch>& launches) {
  launches.clear();
  if (items.empty()) return;
  int M = 0; for (const GmPostItem& it : items) M = std::max(M, it.len);
  const size_t want = std::min<size_t>((items.size() + 63) & ~(size_t)63, (size_t)GM_POST_THREADS);
  std::vector<int> bound;                                       // a class takes the items of at most this many columns that no earlier class took
  if (want * (size_t)M * GM_POST_COL_BYTES > GM_POST_BUDGET) bound = {M / 64, M / 8, M}; else bound = {M};
  std::vector<GmPostItem> sorted; sorted.reserve(items.size());
  int lo = 0;
  for (int b : bound) {
    PostLaunch L; L.first = (int)sorted.size();
    for (const GmPostItem& it : items) if (it.len > lo && it.len <= b) { sorted.push_back(it); L.max_len = std::max(L.max_len, it.len); }
    lo = b;
    L.count = (int)sorted.size() - L.first;
    if (!L.count) continue;
    const size_t fit = (GM_POST_BUDGET / ((size_t)L.max_len * GM_POST_COL_BYTES)) & ~(size_t)63;          // (>= 64: longer alignments were refused)
    L.threads = (int)std::max<size_t>(64, std::min(std::min(want, ((size_t)L.count + 63) & ~(size_t)63), fit));
    launches.push_back(L);
  }
  items.swap(sorted);
}
extern "C" int gm_post_sw_batch_last_plan(int launch, int* items, int* threads, int* columns) {
  const PostPlan& P = g_post_plan;
  if (launch >= 0 && launch < P.n) { if (items) *items = P.l[launch].count; if (threads) *threads = P.l[launch].threads; if (columns) *columns = P.l[launch].max_len; }
  return P.n;
}
