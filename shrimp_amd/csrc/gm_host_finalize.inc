// gm_host_finalize.inc -- the host's share of a read after pass 2: score every result, select the read's mappings, give them mapping qualities; included by
// gm_host.hip (same translation unit, in front of gm_host_records.inc, which turns the outcome into text).
//   HitScorer::post_sw         hit_run_post_sw          ref: gmapper/mapping.c:1609-1625      cs_post_sw    ref: common/sw-post.c:111-758
//   HitScorer::select_hits     read_pass2               ref: mapping.c:1628-1750              dedup_pass    ref: mapping.c:1552-1600
//   HitScorer::unpaired_mqv    compute_unpaired_mqv     ref: gmapper/output.c:777-793,975-984
struct FHit {            // one pass-2 candidate on the host (read_hit + sw_full_results subset)
  const GmFullRes* r; const uint8_t* ops;
  int score_full, pass2_key; double pct_score_full; double posterior; int mqv; double z0, z1;
  bool dev_post = false;          // colour space: posterior and re-called letters came from k_post_sw_cs (the host routine can still redo them)
  double z2, z3, pr_top_random, insert_size_denom, pr_missed_mp;   // paired mode (ref: sw-full-common.h:30-44)
  std::string db, qr, qual; int cs_match = 0, cs_mismatch = 0, cs_xover = 0;   // colour space: dbalign / qralign and the counts post_sw leaves (ref: sw-post.c:531-565)
};
// what the scorer below calls of gm_host_records.inc
struct RecCtx; struct RecRead; struct RecMate;
static void cs_alignment_strings(const uint8_t* bt, const uint8_t* codes, int n, std::string& db, std::string& qr, bool recalled = false);
static void sam_record(const RecCtx& C, const RecRead& rd, const FHit* h, const RecMate* mate, std::string& out);
static void shrimp_record(const RecCtx& C, const RecRead& rd, const FHit& h, std::string& out);

static int qv_from_pr_corr(double pr_corr) {   // ref: common/util.h:267-283
  double pr_err = 1 - pr_corr;
  if (pr_err > .99999999) return 0; else if (pr_err < 1E-25) return 250;
  return (int)(-10.0 * log(pr_err) / log(10.0));
}
static int double_to_neglog(double x) { return (int)((double)1000 * -log(x)); }   // ref: common/util.h:297-301

// The double expressions of hit_run_post_sw and compute_unpaired_mqv (ref: mapping.c:1609-1625, output.c:777-793), shared by the finalisation of the mapping entries
// and by gm_select_pass2: one text, so both round through the host's libm alike.
static inline double gm_ls_posterior(double a, double b, int score, int rmapped) { return pow(2.0, ((double)score - (double)rmapped * (2.0 * a + b)) / a); }
static inline double gm_post_score_x(double a, double b, double posterior, int rmapped) { return a * log(posterior) / log(2.0) + (double)rmapped * (2.0 * a + b); }   // what rint() turns into AS
static inline int gm_post_score(double a, double b, double posterior, int rmapped) { return (int)rint(gm_post_score_x(a, b, posterior, rmapped)); }
static inline double gm_full_threshold(const gm_params_t& P, int score_max) { return P.sw_full_threshold < 0 ? -P.sw_full_threshold : score_max * (P.sw_full_threshold / 100.0); }   // ref: mapping.c:1661
static inline int gm_unpaired_mqv(double posterior, double z1) { const int q = qv_from_pr_corr(posterior / z1); return q < 4 ? 0 : q; }
// the rounding guard's distance tests (see HitScorer::guard_tol)
static inline bool gm_near_rint(double x, double tol) { const double f = x - floor(x); return fabs(f - 0.5) < tol; }              // rint(): boundary at the half integers
static inline bool gm_near_trunc(double x, double tol) { return fabs(x - rint(x)) < tol; }                                          // (int): boundary at the integers
static inline bool gm_near_qv(double pr_corr, double tol) {                                                                         // qv_from_pr_corr, ref: common/util.h:267-283
  const double pr_err = 1 - pr_corr;
  if (fabs(pr_err - .99999999) < tol * 1e-2 || (pr_err > 0 && fabs(pr_err / 1E-25 - 1.0) < tol)) return true;
  if (pr_err > .99999999 || pr_err < 1E-25) return false;
  return gm_near_trunc(-10.0 * log(pr_err) / log(10.0), tol);
}

static int cmp_gen_start(const FHit* a, const FHit* b) {   // ref: mapping.c:1485-1494
  if (a->r->cn != b->r->cn) return (int)a->r->cn - (int)b->r->cn;
  if (a->r->gen_st != b->r->gen_st) return a->r->gen_st - b->r->gen_st;
  return a->r->genome_start - b->r->genome_start;
}
static int cmp_gen_end(const FHit* a, const FHit* b) {     // ref: mapping.c:1496-1506
  if (a->r->cn != b->r->cn) return (int)a->r->cn - (int)b->r->cn;
  if (a->r->gen_st != b->r->gen_st) return a->r->gen_st - b->r->gen_st;
  return (-a->r->genome_start - a->r->rmapped + a->r->n_del - a->r->n_ins) - (-b->r->genome_start - b->r->rmapped + b->r->n_del - b->r->n_ins);
}
// A stable sort of the handful of mappings a read has: insertion sort below 24 elements (the same order as any stable sort; std::stable_sort asks the allocator for a merge
// buffer at every call -- three calls a read were a third of the finalisation's cycles), the library's merge sort above.
template <class It, class Less> static inline void gm_small_stable_sort(It b, It e, Less less) {
  const auto n = e - b;
  if (n < 2) return;
  if (n > 24) { std::stable_sort(b, e, less); return; }
  for (It i = b + 1; i != e; ++i) {
    auto x = *i; It j = i;
    while (j != b && less(x, *(j - 1))) { *j = *(j - 1); --j; }
    *j = x;
  }
}
template <class Cmp>
static void dedup_pass(std::vector<FHit*>& v, Cmp cmp) {     // ref: mapping.c:1552-1600 (glibc qsort == stable merge sort here)
  if (v.size() < 2) return;
  gm_small_stable_sort(v.begin(), v.end(), [&](const FHit* a, const FHit* b) { return cmp(a, b) < 0; });
  size_t i = 0, k = 0, n = v.size();
  while (i < n) {
    int mx = v[i]->pass2_key; size_t mi = i, j = i + 1;
    while (j < n && !cmp(v[i], v[j])) { if (v[j]->pass2_key > mx) { mx = v[j]->pass2_key; mi = j; } j++; }
    if (mi != k) v[k] = v[mi];
    k++; i = j;
  }
  v.resize(k);
}

// ---- colour space: post_sw (ref: common/sw-post.c:639-758) for reads without quality values -----------------------------------
// A 16-state forward-backward over the aligned columns; state j = previous letter << 2 | letter.  The sums run in the reference's
// order in doubles through the same libm calls, so posterior (-> Z0/Z1, MAPQ, AS) carries the same bits; what is hoisted out of
// the reference's inner loops (node priors, exp() of the previous column, log() of a sum shared by four states) is computed from
// identical operands, once instead of four or sixteen times.
struct CsPostConsts {
  double let_m, let_x, col_m[2], col_x[2];            // log(1 - e), log(e / 3) for the letter and the two colour error rates
  double pr_del_open, pr_del_extend, pr_ins_open, pr_ins_extend;
  bool sanger = true; int qoff = 0;                   // read QVs: PHRED (Sanger) or Solexa-style odds (ref: sw-post.c:489-491); offset of the first colour's QV in the string
};
static CsPostConsts cs_post_consts_from(double pr_snp, double pr_xover, double pr_del_open, double pr_del_extend, double pr_ins_open, double pr_ins_extend,
                                        bool sanger, int qoff) {
  CsPostConsts c; const double ce[2] = {pr_xover, .75};
  c.let_m = log(1 - pr_snp); c.let_x = log(pr_snp / 3.0);
  for (int k = 0; k < 2; k++) { c.col_m[k] = log(1 - ce[k]); c.col_x[k] = log(ce[k] / 3.0); }
  c.pr_del_open = pr_del_open; c.pr_del_extend = pr_del_extend; c.pr_ins_open = pr_ins_open; c.pr_ins_extend = pr_ins_extend; c.sanger = sanger; c.qoff = qoff;
  return c;
}
static CsPostConsts cs_post_consts(const gm_session* s) {
  return cs_post_consts_from(s->pr_mismatch, s->P.pr_xover, s->pr_del_open, s->pr_del_extend, s->pr_ins_open, s->pr_ins_extend, true, 0);
}
// exp() of 16 state values of one column.  The 16 arguments take few distinct values (a state's prior has four possible values, the
// transition terms depend on one letter only), and exp is a pure function: computing it once per distinct bit pattern gives the very same
// doubles as 16 calls do.
static inline void exp_neg16(const double* in, double* out) {
  uint64_t seen[16]; double val[16]; int ns = 0;
  for (int k = 0; k < 16; k++) {
    uint64_t b; memcpy(&b, &in[k], 8);
    int j = 0; while (j < ns && seen[j] != b) j++;
    if (j == ns) { seen[ns] = b; val[ns] = exp(-1 * in[k]); ns++; }
    out[k] = val[j];
  }
}

static void cs_post_sw(const CsPostConsts& K, const uint32_t* rw, int init_bp, int read_start, FHit& h,
                       const char* qual = nullptr, int qual_delta = 33, bool base_quals = false) {   // qual: the read's QV string (csfastq) or null; base_quals: h.qual even without it
  struct Col { double prior[16], fw[16], bw[16], fs, bs; int col, base_call; };
  std::string& db = h.db; std::string& qr = h.qr;
  static thread_local std::vector<Col> colbuf;
  if (colbuf.size() < db.size() + 1) colbuf.resize(db.size() + 1);
  Col* cols = colbuf.data(); int len = 0;
  auto colour = [&](int j) { return (int)((rw[j >> 3] >> ((j & 7) * 4)) & 0xf); };
  {  // load_local_vectors, ref: sw-post.c:448-528
    int start_run = 0, j, min_qv = 10000;
    for (j = 0; j < read_start; j++) {
      const int c = colour(j);
      if (c == 15) { start_run = 15; min_qv = 0; j = read_start; break; }
      start_run ^= c;
      if (qual) min_qv = std::min(min_qv, (int)qual[K.qoff + j]);
    }
    for (size_t i = 0; i < db.size(); i++) {
      if (qr[i] == '-') continue;
      Col& c = cols[len];
      int let = -2;                                     // -2: no letter emission (insertion); -1: a letter no state matches
      if (db[i] != '-') switch (db[i]) { case 'A': case 'a': let = 0; break; case 'C': case 'c': let = 1; break; case 'G': case 'g': let = 2; break;
                                         case 'T': case 't': let = 3; break; default: let = -1; }
      const int cc = colour(j); int which;
      if ((len == 0 && start_run == 15) || cc == 15) { c.col = 0; which = 1; } else { c.col = cc ^ (len == 0 ? start_run : 0); which = 0; }
      double col_m = K.col_m[which], col_x = K.col_x[which];
      if (qual && which == 0) {                         // the colour's own error rate, ref: sw-post.c:486-491 (use_sanger_qvs = true)
        const int qv = (len == 0 ? std::min(min_qv, (int)qual[K.qoff + j]) : (int)qual[K.qoff + j]) - qual_delta;
        double e = qv <= 0 ? .99999999 : (qv >= 250 ? 1E-25 : pow(10.0, -(double)qv / 10.0));
        if (!K.sanger) e /= (1 + e);
        if (e > .75) e = .75;
        col_m = log(1 - e); col_x = log(e / 3.0);
      }
      c.base_call = -1;
      switch (qr[i]) { case 'A': case 'a': c.base_call = 0; break; case 'C': case 'c': c.base_call = 1; break; case 'G': case 'g': c.base_call = 2; break;
                       case 'T': case 't': c.base_call = 3; break; default: break; }
      for (int st = 0; st < 16; st++) {                 // nodePrior, ref: sw-post.c:111-138
        const int l = (st >> 2) & 3, r = st & 3; double val = 0;
        if (let != -2) val = val - ((r == let) ? K.let_m : K.let_x);
        val = val - (((l ^ r) == c.col) ? col_m : col_x);
        c.prior[st] = val;
      }
      len++; j++;
    }
  }
  if (len == 0) { h.posterior = 0; return; }
  double total;
  {  // do_forwards, ref: sw-post.c:317-360
    Col& a = cols[0]; a.fs = 999999999;
    for (int j = 0; j < 16; j++) { if (((j >> 2) & 3) == init_bp) { a.fw[j] = a.prior[j]; a.fs = (a.fs < a.fw[j]) ? a.fs : a.fw[j]; } else a.fw[j] = HUGE_VAL; }
    for (int j = 0; j < 16; j++) a.fw[j] -= a.fs;
    for (int i = 1; i < len; i++) {
      Col& c = cols[i]; const Col& p = cols[i - 1];
      double e[16], lg[4];
      exp_neg16(p.fw, e);
      for (int l = 0; l < 4; l++) { double sum = 0; for (int k = l; k < 16; k += 4) sum += e[k]; lg[l] = log(sum); }   // states k with right(k) == l, ascending
      c.fs = 999999999;
      for (int j = 0; j < 16; j++) { c.fw[j] = c.prior[j] - lg[(j >> 2) & 3]; c.fs = (c.fs < c.fw[j]) ? c.fs : c.fw[j]; }
      for (int j = 0; j < 16; j++) c.fw[j] -= c.fs;
      c.fs += p.fs;
    }
    double val = 0;
    for (int j = 0; j < 16; j++) val += exp(-1 * (cols[len - 1].fw[j]));
    total = -log(val) + cols[len - 1].fs;
  }
  {  // do_backwards, ref: sw-post.c:269-315
    Col& z = cols[len - 1]; z.bs = 999999999;
    for (int j = 0; j < 16; j++) { z.bw[j] = 0; z.bs = (z.bs < z.bw[j]) ? z.bs : z.bw[j]; }
    for (int j = 0; j < 16; j++) z.bw[j] -= z.bs;
    for (int i = len - 2; i >= 0; i--) {
      Col& c = cols[i]; const Col& n = cols[i + 1];
      double e[16], nl[4];
      { double a[16]; for (int k = 0; k < 16; k++) a[k] = n.prior[k] + n.bw[k]; exp_neg16(a, e); }
      for (int r = 0; r < 4; r++) { double sum = 0; for (int k = 4 * r; k < 4 * r + 4; k++) sum += e[k]; nl[r] = -log(sum); }     // states k with left(k) == r
      c.bs = 999999999;
      for (int j = 0; j < 16; j++) { c.bw[j] = nl[j & 3]; c.bs = (c.bs < c.bw[j]) ? c.bs : c.bw[j]; }
      for (int j = 0; j < 16; j++) c.bw[j] -= c.bs;
      c.bs += n.bs;
    }
  }
  {  // post_traceback + fix_base_calls, ref: sw-post.c:183-212,531-565
    int j = 0, prev_base = init_bp; h.cs_match = h.cs_mismatch = h.cs_xover = 0; h.qual.clear();
    for (size_t i = 0; i < qr.size(); i++) {
      if (qr[i] == '-') continue;
      const Col& c = cols[j];
      double post[4] = {0, 0, 0, 0};
      { double a[16], ev[16]; for (int st = 0; st < 16; st++) a[st] = c.fw[st] + c.bw[st] + c.fs + c.bs - total; exp_neg16(a, ev);
        for (int st = 0; st < 16; st++) post[st & 3] += ev[st]; }
      int crt = 0; for (int b = 1; b < 4; b++) if (post[b] > post[crt]) crt = b;
      if (qual || base_quals) {                         // get_base_qualities, ref: sw-post.c:568-586: of the letter sw_full_cs had called
        int t = c.base_call >= 0 ? qv_from_pr_corr(post[c.base_call]) : 0;
        if (t > 40) t = 40;
        h.qual.push_back((char)(33 + t));
      }
      if ((prev_base ^ crt) == c.col) qr[i] = "ACGT"[crt]; else { qr[i] = "acgt"[crt]; h.cs_xover++; }
      if (db[i] != '-') { if (toupper((unsigned char)db[i]) == toupper((unsigned char)qr[i])) h.cs_match++; else h.cs_mismatch++; }
      prev_base = crt; j++;
    }
  }
  {  // get_posterior, ref: sw-post.c:589-612
    double res = exp(-total);
    for (size_t i = 0; i < db.size(); i++) {
      if (db[i] == '-') { res *= K.pr_ins_extend; if (i == 0 || db[i - 1] != '-') res *= K.pr_ins_open; }
      else if (qr[i] == '-') { res *= K.pr_del_extend; if (i == 0 || qr[i - 1] != '-') res *= K.pr_del_open; }
    }
    h.posterior = res;
  }
}

// -DGM_HOST_PROFILE (diagnostic builds): where the finalisation's cycles go -- rdtsc sums per stage over all worker threads, printed by gm_host_profile_dump()
#ifdef GM_HOST_PROFILE
#include <x86intrin.h>
struct GmHpSlots { unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };
static std::mutex g_hp_m; static std::vector<GmHpSlots*> g_hp_all;
static GmHpSlots& gm_hp_mine() {      // per thread (the pool's threads live as long as the process): no shared counter is touched per read
  static thread_local GmHpSlots* mine = nullptr;
  if (!mine) { mine = new GmHpSlots(); std::lock_guard<std::mutex> lk(g_hp_m); g_hp_all.push_back(mine); }
  return *mine;
}
struct GmHp { unsigned long long t; GmHpSlots& S; GmHp() : t(__rdtsc()), S(gm_hp_mine()) {} void lap(int k) { const unsigned long long n = __rdtsc(); S.v[k] += n - t; t = n; } };
extern "C" void gm_host_profile_dump(void) {
  static const char* nm[8] = {"post_sw / FHit build", "dedup + sort", "mapping qualities", "record text", "unaligned record", "reads (count)", "", ""};
  unsigned long long g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  { std::lock_guard<std::mutex> lk(g_hp_m); for (GmHpSlots* s : g_hp_all) for (int k = 0; k < 8; k++) { g[k] += s->v[k]; s->v[k] = 0; } }
  unsigned long long tot = 0; for (int k = 0; k < 5; k++) tot += g[k];
  for (int k = 0; k < 6; k++) { fprintf(stderr, "[host profile] %-22s %14llu%s %5.1f %%\n", nm[k], g[k], k < 5 ? " cycles" : "       ", k < 5 ? 100.0 * g[k] / (tot ? tot : 1) : 0.0); }
  if (g[5]) fprintf(stderr, "[host profile] %.0f cycles per read\n", (double)tot / (double)g[5]);
}
#define GM_HP_DECL GmHp hp_
#define GM_HP(k) hp_.lap(k)
#else
#define GM_HP_DECL do { } while (0)
#define GM_HP(k) do { } while (0)
#endif
// Scores the pass-2 results of one read set's sub-batch and selects each read's mappings; what it leaves in the FHits is all the record writers need.
struct HitScorer {
  const gm_session* s = nullptr; int read_len = 0, read_words = 0;
  // colour space only -- post_sw reads the colours, the primer letter and the QVs of each read (ref: sw-post.c:448-528):
  const uint32_t* reads = nullptr; const uint8_t* initbp = nullptr;                    // host copy of the packed reads of this sub-batch, and their primer letters
  int ops_half = 0; CsPostConsts csk = CsPostConsts();                                 // ops_stride / 2
  const GmFullRes* res_base = nullptr; const GmPostRes* post_base = nullptr;           // post_sw results of the device, parallel to the sub-batch's result records
  const uint8_t* bq_base = nullptr;                                                    // ... and, for reads with QVs, the base qualities it computed (read_len bytes per result)
  const char* const* qual_ptr = nullptr; int qual_delta = 33;                          // FASTQ input: QUAL string of every read of this sub-batch

  // Rounding guard for results of the device's post_sw (gm_post.hip): its posterior differs from the host routine's in the last bits (ocml exp / log instead of
  // glibc's), which matters only where a value is about to be rounded right at a boundary.  Every such conversion below -- rint() for AS, truncation for MAPQ
  // (with its two cut-offs) and for the Z tags -- checks the distance to the boundary; within guard_tol (1e-7, five orders above the difference) the read's device
  // results are redone by the host routine (same libm as the reference), so the bytes never hang on the device's last bits.
  double guard_tol = 1e-7; std::atomic<uint64_t>* redo_ctr = nullptr;
  bool near_rint(double x) const { return gm_near_rint(x, guard_tol); }
  bool near_trunc(double x) const { return gm_near_trunc(x, guard_tol); }
  bool near_qv(double pr_corr) const { return gm_near_qv(pr_corr, guard_tol); }
  void redo_on_host(FHit& h) const {                    // sw_full_cs's own strings, then the host's post_sw (ref: sw-post.c:636-758), then the posterior score
    const GmFullRes* r = h.r;
    cs_alignment_strings(h.ops, h.ops + ops_half, std::min(r->n_ops, ops_half), h.db, h.qr);
    cs_post_sw(csk, reads + (size_t)r->read_idx * read_words, (int)initbp[r->read_idx], r->read_start, h, qual_ptr ? qual_ptr[r->read_idx] : nullptr, qual_delta);
    h.dev_post = false;
    const double a = s->score_alpha, b = s->score_beta;
    int ps = gm_post_score(a, b, h.posterior, r->rmapped);
    if (ps < 0) ps = 0;
    h.score_full = ps; h.pct_score_full = (1000 * 100 * ps) / r->score_max;
    h.pass2_key = s->P.sw_full_threshold < 0 ? h.score_full : (int)h.pct_score_full;
    if (redo_ctr) redo_ctr->fetch_add(1, std::memory_order_relaxed);
  }
  // hit_run_post_sw for one pass-2 result (ref: mapping.c:1609-1625)
  void post_sw(FHit& h, const GmFullRes* r, const uint8_t* ops) const {
    const gm_params_t& P = s->P;
    h.r = r; h.ops = ops + (size_t)r->ops_off; h.mqv = 255; h.z0 = h.z1 = 0; h.posterior = 0; h.dev_post = false;
    h.z2 = h.z3 = h.pr_top_random = h.insert_size_denom = h.pr_missed_mp = 0;
    h.score_full = r->score;
    h.pct_score_full = (1000 * 100 * h.score_full) / r->score_max;                 // ref: mapping.c:400-401
    if (h.score_full > 0 && gm_mqv_on(P)) {                        // local mode / --no-mapping-qualities: no post_sw (ref: gmapper.c:2325-2328, mapping.c:1648)
      const double a = s->score_alpha, b = s->score_beta;
      if (P.colour_space) {
        if (post_base && (!qual_ptr || bq_base) && post_base[r - res_base].valid == 1) {   // k_post_sw_cs ran: the op record carries the re-called letters in its spare bits
          const GmPostRes& pr = post_base[r - res_base];
          cs_alignment_strings(h.ops, h.ops + ops_half, std::min(r->n_ops, ops_half), h.db, h.qr, true);
          h.posterior = pr.posterior; h.cs_match = pr.cs_match; h.cs_mismatch = pr.cs_mismatch; h.cs_xover = pr.cs_xover; h.qual.clear(); h.dev_post = true;
          if (qual_ptr) {                                                // base qualities of the read positions the alignment covers, in alignment order
            size_t nq = 0; for (char c : h.qr) nq += c != '-';
            h.qual.assign((const char*)bq_base + (size_t)(r - res_base) * read_len, std::min(nq, (size_t)read_len));
          }
          if (near_rint(gm_post_score_x(a, b, h.posterior, r->rmapped))) { redo_on_host(h); return; }      // AS at a rounding boundary
        } else {
        cs_alignment_strings(h.ops, h.ops + ops_half, std::min(r->n_ops, ops_half), h.db, h.qr);
        cs_post_sw(csk, reads + (size_t)r->read_idx * read_words, (int)initbp[r->read_idx], r->read_start, h,
                   qual_ptr ? qual_ptr[r->read_idx] : nullptr, qual_delta);
        }
      }
      int ps;
      if (!P.colour_space) {
        // letter space: posterior and score are functions of (score, mapped read length) alone -- a small per-thread table of the values libm gave for the pairs seen
        // last (reads of one length that map with 0, 1, 2 mismatches share a handful of pairs) instead of a pow and a log per mapping; the same doubles, so the same bytes
        struct Memo { int score, rmapped; double a, b, post; int ps; };
        static thread_local Memo memo[256];                        // (zero-initialised: a == 0 matches no session)
        Memo& m = memo[((unsigned)r->score * 31u + (unsigned)r->rmapped) & 255u];
        if (m.score != r->score || m.rmapped != r->rmapped || m.a != a || m.b != b) {
          m.score = r->score; m.rmapped = r->rmapped; m.a = a; m.b = b;
          m.post = gm_ls_posterior(a, b, r->score, r->rmapped);
          m.ps = gm_post_score(a, b, m.post, r->rmapped);
        }
        h.posterior = m.post; ps = m.ps;
      } else
      ps = gm_post_score(a, b, h.posterior, r->rmapped);
      if (ps < 0) ps = 0;
      h.score_full = ps; h.pct_score_full = (1000 * 100 * ps) / r->score_max;
    }
    else if (h.score_full > 0 && P.colour_space) {                 // colour space, local mode: no post_sw (mapping.c:1648): sw_full_cs's own strings and counts go out
      cs_alignment_strings(h.ops, h.ops + ops_half, std::min(r->n_ops, ops_half), h.db, h.qr);
      h.cs_match = r->n_match; h.cs_mismatch = r->n_mismatch; h.cs_xover = r->n_xover; h.qual.clear();
    }
    h.pass2_key = P.sw_full_threshold < 0 ? h.score_full : (int)h.pct_score_full;
  }
  // read_pass2's selection over the n pass-2 results of one read (ref: mapping.c:1628-1750): p2 = final hits in output order
  void select_hits(const GmFullRes* res, const uint8_t* ops, int n, std::vector<FHit>& fh, std::vector<FHit*>& p2) const {
    const gm_params_t& P = s->P;
    GM_HP_DECL;
    fh.clear(); p2.clear();
    fh.resize(n);
    for (int i = 0; i < n; i++) {
      FHit& h = fh[i]; post_sw(h, &res[i], ops);
      const double thr = gm_full_threshold(P, h.r->score_max);
      if (h.score_full >= thr) p2.push_back(&h);                                   // ref: mapping.c:1661 (double compare)
    }
    GM_HP(0);
    dedup_pass(p2, cmp_gen_start);
    dedup_pass(p2, cmp_gen_end);
    gm_small_stable_sort(p2.begin(), p2.end(), [](const FHit* a, const FHit* b) { return (b->pass2_key - a->pass2_key) < 0; });   // ref :1479-1482,1678
    if ((int)p2.size() > P.num_outputs) p2.resize(P.num_outputs);
    if (P.strata && !p2.empty()) { size_t i = 1; while (i < p2.size() && p2[0]->score_full == p2[i]->score_full) i++; p2.resize(i); }   // ref :1706-1712
    if (P.max_alignments != 0 && (int)p2.size() > P.max_alignments) p2.clear();                                                        // ref :1713-1722
    GM_HP(1);
  }
  // compute_unpaired_mqv over a read's mappings (ref: output.c:777-793,975), then --single-best-mapping
  void unpaired_mqv(std::vector<FHit*>& p2) const {
    for (int pass = 0; pass < 2; pass++) {
      double z1 = 0.0;
      for (auto* h : p2) z1 += h->posterior;
      for (auto* h : p2) { h->z0 = h->posterior; h->z1 = z1; h->mqv = gm_unpaired_mqv(h->posterior, z1); }
      // rounding guard (see post_sw above): MAPQ and the Z0 / Z1 tags of this read's records, when any posterior came from the device
      bool dev = false, near = false;
      for (auto* h : p2) dev = dev || h->dev_post;
      if (pass || !dev) break;
      near = near_trunc(1000.0 * -log(z1));
      for (auto* h : p2) near = near || near_qv(h->posterior / z1) || near_trunc(1000.0 * -log(h->z0));
      if (!near) break;
      for (auto* h : p2) if (h->dev_post) redo_on_host(*h);
    }
    if (s->P.single_best_mapping) {                                                // the first mapping with the highest quality, ref: output.c:977-984
      size_t mx = 0;
      for (size_t i = 1; i < p2.size(); i++) if (p2[i]->mqv > p2[mx]->mqv) mx = i;
      FHit* best = p2[mx]; p2.assign(1, best);
    }
  }

  // the records of one unpaired read (read_output, ref: output.c:944-1047) from its n pass-2 results, appended to out; returns their number
  int finalize_read(const RecCtx& C, const RecRead& rd, const GmFullRes* res, const uint8_t* ops, int n, std::string& out, std::vector<FHit>& fh, std::vector<FHit*>& p2) const {
    const gm_params_t& P = s->P;
    select_hits(res, ops, n, fh, p2);
    GM_HP_DECL;
#ifdef GM_HOST_PROFILE
    hp_.S.v[5]++;
#endif
    if (p2.empty()) {
      if (!P.sam_unaligned) return 0;
      sam_record(C, rd, nullptr, nullptr, out);
      GM_HP(4);
      return 1;
    }
    if (gm_mqv_on(P)) unpaired_mqv(p2);
    GM_HP(2);
    for (auto* h : p2) { if (P.output_format) shrimp_record(C, rd, *h, out); else sam_record(C, rd, h, nullptr, out); }      // --shrimp-format / --pretty, ref: gmapper/output.c:270-296
    GM_HP(3);
    return (int)p2.size();
  }
};
