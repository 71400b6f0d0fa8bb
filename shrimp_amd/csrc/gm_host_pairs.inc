// gm_host_pairs.inc -- host side of paired mode; included by gm_host.hip (same translation unit, after map_impl).
//   handle_readpair            ref: gmapper/mapping.c:2502-2636     readpair_pass2          ref: mapping.c:2181-2314
//   readpair_save_final_hits   ref: mapping.c:2446-2499             compute_paired_mqv      ref: output.c:811-942
//   readpair_output            ref: output.c:1070-1291              hit_output (paired)     ref: output.c:227-774
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

static void hit_ends(const gm_index* ix, const FHit* h, int* gstart, int* gend) {   // ref: mapping.c:414-441
  const GmFullRes& r = *h->r;
  const int read_start = r.read_start + 1, read_end = read_start + r.rmapped - 1;
  const int glen = (int)(ix->contig_off[r.cn + 1] - ix->contig_off[r.cn]);
  if (r.gen_st != 1) *gstart = r.genome_start + 1;
  else *gstart = (glen - r.genome_start) - (read_end - read_start - r.n_del + r.n_ins);
  *gend = *gstart + r.gmapped - 1;
}
static int get_insert_size(const gm_index* ix, const FHit* rh, const FHit* rh_mp) {    // ref: mapping.c:405-456
  if (rh->r->cn != rh_mp->r->cn) return 0;
  int gs_mp, ge_mp, gs, ge; hit_ends(ix, rh_mp, &gs_mp, &ge_mp); hit_ends(ix, rh, &gs, &ge);
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

// hit_output for one mate of a pair (ref: output.c:227-774); rh == nullptr: unmapped-mate line
static void emit_pair_record(const PairCtx& C, std::string& out, const char* qn, size_t qnl, const uint32_t* rw, int read_len, int ops_stride,
                             const FHit* rh, const FHit* rh_mp, bool first_in_pair, bool improper, const char* qual = nullptr, int qual_delta = 33, int initbp = -1,
                             const std::string* mate_seq = nullptr) {
  const gm_index* ix = C.s->ix;
  const bool cs = C.s->P.colour_space != 0;                    // colour space (initbp = the read's primer letter): SEQ / clips / tags as in the unpaired records (ref: output.c:353-355,441-451,485-537,572-580,717-730)
  auto put_csfasta = [&](char* p) { *p++ = "ACGT"[initbp & 3]; for (int i = 0; i < read_len; i++) { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; *p++ = (c < 4) ? (char)('0' + c) : '.'; } return p; };
  const bool paired_alignment = (rh != nullptr && rh_mp != nullptr && !improper);
  const bool query_unmapped = (rh == nullptr), mate_unmapped = (rh_mp == nullptr);
  bool reverse_strand = false, reverse_strand_mp = false;
  int genome_start_mp = 0, genome_end_mp = 0; unsigned mpos = 0;
  const std::string* mrnm = nullptr;
  if (!mate_unmapped) {
    reverse_strand_mp = (rh_mp->r->gen_st == 1);
    hit_ends(ix, rh_mp, &genome_start_mp, &genome_end_mp);
    mpos = (unsigned)genome_start_mp; mrnm = &ix->names[rh_mp->r->cn];
  }
  const size_t n_ops = rh ? (size_t)rh->r->n_ops : 0;
  const size_t need = qnl + 5 * (size_t)read_len + 12 * n_ops + 400 + (rh ? ix->names[rh->r->cn].size() : 0) + (mrnm ? mrnm->size() : 0);
  // (staged on the stack and appended, as in the unpaired writer: the bound is several times the record and std::string::resize zero-fills it)
  char stage[6144]; const bool staged = need <= sizeof stage;
  if (!staged) { const size_t o = out.size(); out.resize(o + need); }
  char* p = staged ? stage : &out[out.size() - need];
  auto commit = [&](char* e) { if (staged) out.append(stage, (size_t)(e - stage)); else out.resize((size_t)(e - out.data())); };
  p = put_str(p, qn, qnl); *p++ = '\t';
  if (query_unmapped) {                                                               // ref: output.c:411-466
    const int flags = 0x1 | 0x4 | (mate_unmapped ? 0x8 : 0) | (reverse_strand_mp ? 0x20 : 0) | (first_in_pair ? 0x40 : 0x80);
    p = put_int(p, flags); p = put_str(p, "\t*\t0\t0\t*\t", 9);
    if (mrnm) p = put_str(p, mrnm->data(), mrnm->size()); else *p++ = '*';
    *p++ = '\t'; p = put_uint(p, mpos); p = put_str(p, "\t0\t", 3);
    if (cs) {                                                                         // ref: output.c:441-451
      p = put_str(p, "*\t*\tCQ:Z:", 9); if (qual) p = put_str(p, qual, (size_t)read_len); else *p++ = '*';
      p = put_str(p, "\tCS:Z:", 6); p = put_csfasta(p); commit(p); Finalizer::sam_tail(C.s->P, out, mate_seq, nullptr, nullptr, nullptr); return; }
    for (int i = 0; i < read_len; i++) { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; *p++ = (c < 4) ? "ACGT"[c] : (c == 4 ? 'U' : 'N'); }
    if (qual) { *p++ = '\t'; p = put_str(p, qual, (size_t)read_len); }               // FASTQ input, verbatim (ref: output.c:419-421)
    else p = put_str(p, "\t*", 2);
    commit(p); Finalizer::sam_tail(C.s->P, out, mate_seq, nullptr, nullptr, nullptr);
    return;
  }
  const GmFullRes& r = *rh->r;
  reverse_strand = (r.gen_st == 1);
  const int read_start = r.read_start + 1, read_end = read_start + r.rmapped - 1;
  int genome_start, genome_end; hit_ends(ix, rh, &genome_start, &genome_end);
  const int flags = 0x1 | (paired_alignment ? 0x2 : 0) | (mate_unmapped ? 0x8 : 0) | (reverse_strand ? 0x10 : 0) | (reverse_strand_mp ? 0x20 : 0) |
                    (first_in_pair ? 0x40 : 0x80);
  p = put_int(p, flags); *p++ = '\t';
  p = put_str(p, ix->names[r.cn].data(), ix->names[r.cn].size()); *p++ = '\t';
  p = put_uint(p, (unsigned)genome_start); *p++ = '\t';
  p = put_int(p, rh->mqv); *p++ = '\t';
  {  // CIGAR (make_cigar, ref: output.c:15-64)
    struct Run { int len; char op; }; Run runs[GM_MAX_OPS]; int nr = 0;
    const char clip = cs ? 'H' : 'S';
    if (read_start > 1) runs[nr++] = {read_start - 1, clip};
    if (cs) {
      const int na = (int)rh->qr.size();
      for (int i = 0; i < na;) {
        const char op = rh->qr[i] == '-' ? 'D' : (rh->db[i] == '-' ? 'I' : 'M'); int j = i;
        while (j < na && (rh->qr[j] == '-' ? 'D' : (rh->db[j] == '-' ? 'I' : 'M')) == op) j++;
        if (nr < GM_MAX_OPS - 1) runs[nr++] = {j - i, op};
        i = j;
      }
    } else {
    const int nops = std::min(r.n_ops, ops_stride);
    for (int i = 0; i < nops;) {
      const char op = (char)rh->ops[i]; int j = i; while (j < nops && rh->ops[j] == (uint8_t)op) j++;
      if (nr < GM_MAX_OPS - 1) runs[nr++] = {j - i, op == 'M' ? 'M' : (op == 'I' ? 'D' : 'I')};
      i = j;
    }
    }
    if (read_end != read_len) runs[nr++] = {read_len - read_end, clip};
    if (!reverse_strand) for (int i = 0; i < nr; i++) { p = put_uint(p, (unsigned)runs[i].len); *p++ = runs[i].op; }
    else for (int i = nr - 1; i >= 0; i--) { p = put_uint(p, (unsigned)runs[i].len); *p++ = runs[i].op; }
  }
  *p++ = '\t';
  int isize = 0;
  if (!mate_unmapped) {                                                               // ref: output.c:640-655
    if (ix->names[r.cn] == *mrnm) {
      *p++ = '=';
      const int fivep = reverse_strand ? genome_end : genome_start - 1;
      const int fivep_mp = reverse_strand_mp ? genome_end_mp : genome_start_mp - 1;
      isize = fivep_mp - fivep;
    } else p = put_str(p, mrnm->data(), mrnm->size());
  } else *p++ = '*';
  *p++ = '\t'; p = put_uint(p, mpos); *p++ = '\t'; p = put_int(p, isize); *p++ = '\t';
  if (cs) {                                                    // the aligned letters post_sw called
    auto up = [](char c) { if (c >= 'a') c -= 32; return (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N') ? c : 'N'; };
    const int na = (int)rh->qr.size();
    if (!reverse_strand) { for (int i = 0; i < na; i++) if (rh->qr[i] != '-') *p++ = up(rh->qr[i]); }
    else for (int i = na - 1; i >= 0; i--) if (rh->qr[i] != '-') *p++ = rc_char(up(rh->qr[i]));
  } else
  if (!reverse_strand) for (int i = 0; i < read_len; i++) { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; *p++ = CODE2SEQ[c]; }
  else for (int i = read_len - 1; i >= 0; i--) { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; *p++ = rc_char(CODE2SEQ[c]); }
  if (cs && qual && !rh->qual.empty()) {                                              // csfastq: post_sw's base qualities (ref: output.c:613-621); --local runs no post_sw: '*'
    *p++ = '\t'; const int nq = (int)rh->qual.size();
    if (!reverse_strand) p = put_str(p, rh->qual.data(), (size_t)nq); else for (int i = nq - 1; i >= 0; i--) *p++ = rh->qual[i];
    p = put_str(p, "\tAS:i:", 6);
  } else
  if (qual && !cs) {                                                                  // FASTQ input: reversed with the read, re-based to PHRED+33 (ref: output.c:539-570)
    *p++ = '\t'; const int dq = 33 - qual_delta;
    if (!reverse_strand) for (int i = 0; i < read_len; i++) *p++ = (char)(qual[i] + dq);
    else for (int i = read_len - 1; i >= 0; i--) *p++ = (char)(qual[i] + dq);
    p = put_str(p, "\tAS:i:", 6);
  } else p = put_str(p, "\t*\tAS:i:", 8);
  p = put_int(p, rh->score_full);
  if (!gm_mqv_on(C.s->P) || C.s->P.all_contigs) {}                                     // no Z tags without mapping qualities or with --all-contigs (ref: output.c:691)
  else if (paired_alignment) {
    p = put_str(p, "\tZ2:i:", 6); p = put_int(p, double_to_neglog(rh->z2));
    p = put_str(p, "\tZ3:i:", 6); p = put_int(p, double_to_neglog(rh->z3));
    p = put_str(p, "\tZ4:i:", 6); p = put_int(p, double_to_neglog(rh->pr_top_random));
    p = put_str(p, "\tZ6:i:", 6); p = put_int(p, double_to_neglog(rh->insert_size_denom));
  } else {
    p = put_str(p, "\tZ0:i:", 6); p = put_int(p, double_to_neglog(rh->z0));
    p = put_str(p, "\tZ1:i:", 6); p = put_int(p, double_to_neglog(rh->z1));
    p = put_str(p, "\tZ4:i:", 6); p = put_int(p, double_to_neglog(rh->pr_top_random));
    p = put_str(p, "\tZ5:i:", 6); p = put_int(p, double_to_neglog(rh->pr_missed_mp));
  }
  p = put_str(p, "\tNM:i:", 6); p = put_int(p, (cs ? rh->cs_mismatch : r.n_mismatch) + r.n_del + r.n_ins);
  if (cs) {
    if (qual) { p = put_str(p, "\tCQ:Z:", 6); p = put_str(p, qual, (size_t)read_len); }           // ref: output.c:724-727
    p = put_str(p, "\tCS:Z:", 6); p = put_csfasta(p);
    p = put_str(p, "\tCM:i:", 6); p = put_int(p, rh->cs_xover);
    p = put_str(p, "\tXX:Z:", 6); p = put_str(p, rh->qr.data(), rh->qr.size());
  }
  commit(p);
  if (C.s->P.extra_sam_fields && !cs) {
    std::string db, qr; Finalizer F{C.s, read_len, (read_len + 7) / 8, nullptr, nullptr, nullptr, 0}; F.hgen = C.s->h_genome.data();
    F.ls_alignment_strings(r, rh->ops, std::min(r.n_ops, ops_stride), rw, db, qr);
    Finalizer::sam_tail(C.s->P, out, mate_seq, rh, &db, &qr);
  } else Finalizer::sam_tail(C.s->P, out, mate_seq, rh, &rh->db, &rh->qr);
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

static int map_pairs_impl(gm_session* s, int n_pairs, int len1, const uint32_t* m1, int len2, const uint32_t* m2,
                          const char* names1, const char* names2, const gm_pair_opts_t* opts, char** sam, size_t* sam_len, gm_map_stats_t* stats,
                          const char* quals1 = nullptr, const char* quals2 = nullptr, int qual_delta = 33,
                          const uint8_t* initbp1 = nullptr, const uint8_t* initbp2 = nullptr, uint32_t* per_pair_bytes = nullptr) {
  if (!s || n_pairs < 0 || len1 < 1 || len2 < 1 || (n_pairs > 0 && (!m1 || !m2))) { gm_set_error("gm_map_pairs: bad arguments"); return GM_E_ARG; }
  GmDevTurn dev_turn(s);
  GM_HIP(hipSetDevice(s->ix->device));
  if ((s->P.output_format || s->P.extra_sam_fields) && s->h_genome.empty()) {      // the SHRiMP / pretty formats and the ZE:Z edit string print genome letters: one download per session
    s->h_genome.resize(s->ix->genome_words);
    GM_HIP(hipMemcpy(s->h_genome.data(), s->ix->d_genome, s->ix->genome_words * 4, hipMemcpyDeviceToHost));
  }
  const bool cs = s->P.colour_space != 0;
  const uint8_t* initbp_in[2] = {initbp1, initbp2};
  if (cs && n_pairs > 0 && (!initbp1 || !initbp2)) { gm_set_error("gm_map_pairs_cs: no primer letters"); return GM_E_ARG; }
  gm_pair_opts_t O; if (opts) O = *opts; else gm_pair_opts_default(&O);
  if (O.pair_mode < GM_PAIR_OPP_IN || O.pair_mode > GM_PAIR_COL_BW) { gm_set_error("gm_map_pairs: pair_mode %d", O.pair_mode); return GM_E_ARG; }
  // half_paired = 0 (--no-half-paired): each mate's list entries are filtered by the other mate's region counts (k_mp_filter, ref: mapping.c:545-608,
  // gmapper.c:2657-2662 use_mp_region_counts = 1) and no unpaired rescue runs afterwards (gmapper.c:2678-2683)
  // match_mode (the reference's -n in paired mode, gmapper.c:2652-2673): 4 as above; 3: the lookup also keeps the entries of regions marked once that the mate reaches
  // with a region it marked twice (GmMpDev; without half-paired the filter then applies rule 3), the window kernel runs hit-list mode 3; 2: no region counts, a window
  // per anchor.  pass 1 asks for two matches only in mode 4 (:2673); the unpaired rescue always does (:2708).
  const int pmode = O.match_mode == 0 ? 4 : O.match_mode;
  if (pmode < 2 || pmode > 4) { gm_set_error("gm_map_pairs: match_mode %d (2, 3 or 4 in paired mode, ref: gmapper.c:2495-2498)", O.match_mode); return GM_E_ARG; }
  const bool mp_counts = !O.half_paired && pmode == 4;
  struct BothStrands { gm_session* s; int v; explicit BothStrands(gm_session* s_) : s(s_), v(s_->sc.skip_strands) { s->sc.skip_strands = 0; } ~BothStrands() { s->sc.skip_strands = v; } }
    both_strands(s);                                           // -C / -F do not apply in paired mode (ref: gmapper.c:2448-2451)
  GmScoreDev scp = s->sc; scp.match_mode = pmode == 4 ? 2 : (pmode == 3 ? 3 : 1); scp.min_matches = pmode == 4 ? 2 : 1;      // hit_list.match_mode, pass1.min_matches of the paired set
  GmScoreDev scr = s->sc; scr.min_matches = 2;                                                                                // the half-paired rescue's pass 1
  const int len[2] = {len1, len2}; const uint32_t* mates[2] = {m1, m2};
  for (int m = 0; m < 2; m++)
    if (len[m] > s->P.longest_read_len || len[m] >= 32768 / std::max(1, s->P.match_score)) { gm_set_error("read length %d out of range (ref: sw-vector.c:393-398)", len[m]); return GM_E_RANGE; }
  GM_HIP(hipSetDevice(s->ix->device));
  if (stats) memset(stats, 0, sizeof *stats);
  s->last_lookup_ms = 0; s->last_lookup_bytes = 0; s->last_lookup_launches = 0;
  const gm_index* ix = s->ix;
  const GmIndexDev dv = ix->dev_view();
  // colour space: a mate the pair mode reverses (read_reverse, ref: gmapper.c:174-185,561-570) keeps its colours and swaps its strand labels (GmIndexDev::cs_flip);
  // letter space: it is stored reverse-complemented (k_revcomp_reads)
  GmIndexDev dvm[2] = {dv, dv};
  hipStream_t q = s->stream_b;                                  // everything after the front
  static const bool pair_reverse[5][2] = {{0, 0}, {0, 0}, {1, 1}, {0, 1}, {1, 0}};   // ref: gmapper-defaults.h:184-191
  int rwords[2], W[2], ovl[2], in_st[2];
  for (int m = 0; m < 2; m++) {
    rwords[m] = (len[m] + 7) / 8; W[m] = window_len_of(s->P, len[m]);
    ovl[m] = (int)(unsigned int)(s->P.window_overlap < 0 ? -s->P.window_overlap : W[m] * (s->P.window_overlap / 100.0));
    in_st[m] = pair_reverse[O.pair_mode][m] ? 1 : 0;
    if (cs) dvm[m].cs_flip = in_st[m];
    DevSet& D = s->set[m];
    if (D.cur_len != len[m] || D.d_pmin == nullptr || (D.caps_pair_mode != pmode && (pmode != 4 || D.caps_pair_mode != 0))) { choose_caps(s, D, len[m], pmode); D.caps_pair_mode = pmode; int rc = alloc_buffers(s, D, len[m], true); if (rc) return rc; }
  }
  // Two pairs of buffer sets: the front (K1, K1b, K2 of both mates; stream A) of sub-batch i + 1 is queued before the host turns to the rest of
  // sub-batch i (stream B), as in map_impl.  GM_OVERLAP=0: one pair, in order.
  DevSet* PS[2][2] = {{&s->set[0], &s->set[1]}, {&s->set2[0], &s->set2[1]}};
  bool overlap = n_pairs > std::min(s->set[0].eff_batch, s->set[1].eff_batch);
  if (const char* e = getenv("GM_OVERLAP")) overlap = overlap && atoi(e) != 0;
  if (overlap)
    for (int m = 0; m < 2; m++) {
      DevSet& D = s->set2[m]; const DevSet& R = s->set[m];
      if (D.cur_len != len[m] || D.d_pmin == nullptr || D.scap != R.scap || D.scap2 != R.scap2 || D.hcap < R.hcap || D.rcap_per_read < R.rcap_per_read) {
        D.scap = R.scap; D.scap2 = R.scap2; D.hcap = std::max(D.hcap, R.hcap); D.rcap_per_read = std::max(D.rcap_per_read, R.rcap_per_read);
        int rc = alloc_buffers(s, D, len[m], true); if (rc) return rc;
      }
    }
  hipStream_t qa = s->stream;
  // readpair_compute_mp_ranges, ref: mapping.c:2317-2442 (only the delta_g_off part is used without mate-pair region counts)
  int dmin[2], dmax[2];
  {
    const int mn = O.min_insert_size, mx = O.max_insert_size;
    int a = mn - W[1], b = mx + (W[0] - len[0]) - len[1], c = -mx + len[0] + (len[1] - W[1]), d = -mn + W[0];
    switch (O.pair_mode) {
      case GM_PAIR_OPP_IN: break;
      case GM_PAIR_OPP_OUT: a += len[0] + len[1]; b += len[0] + len[1]; c -= len[0] + len[1]; d -= len[0] + len[1]; break;
      case GM_PAIR_COL_FW: a += len[1]; b += len[1]; c -= len[1]; d -= len[1]; break;
      default: a += len[0]; b += len[0]; c -= len[0]; d -= len[0]; break;
    }
    dmin[0] = a; dmax[0] = b; dmin[1] = c; dmax[1] = d;
  }
  int dmin2[2], dmax2[2];                                      // the second mate's ranges (ref: mapping.c:2340-2343,2366-2369,2381-2384,2407-2410)
  if (O.pair_mode == GM_PAIR_OPP_IN || O.pair_mode == GM_PAIR_OPP_OUT) { dmin2[0] = -dmax[1]; dmax2[0] = -dmin[1]; dmin2[1] = -dmax[0]; dmax2[1] = -dmin[0]; }
  else { dmin2[0] = -dmax[0]; dmax2[0] = -dmin[0]; dmin2[1] = -dmax[1]; dmax2[1] = -dmin[1]; }
  PairCtx C; C.s = s; C.O = O; C.len[0] = len1; C.len[1] = len2; C.rwords[0] = rwords[0]; C.rwords[1] = rwords[1]; C.total_genome_size = (double)ix->total_len;
  // names
  std::vector<const char*> nptr[2]; std::vector<int> nlen[2];
  const char* names[2] = {names1, names2};
  for (int m = 0; m < 2; m++)
    if (names[m]) { const char* p = names[m]; for (int i = 0; i < n_pairs; i++) { const char* e = strchr(p, '\n'); if (!e) e = p + strlen(p); nptr[m].push_back(p); nlen[m].push_back((int)(e - p)); p = *e ? e + 1 : e; } }
  std::vector<const char*> qptr[2];                            // FASTQ input: QUAL string of every mate
  const char* qualsv[2] = {quals1, quals2};
  if ((quals1 != nullptr) != (quals2 != nullptr)) { gm_set_error("gm_map_pairs_fastq: QUAL strings for both mates or for none"); return GM_E_ARG; }
  for (int m = 0; m < 2; m++)
    if (qualsv[m]) {
      const char* p = qualsv[m];
      for (int i = 0; i < n_pairs; i++) {
        const char* e = strchr(p, '\n'); if (!e) e = p + strlen(p);
        if ((int)(e - p) != len[m]) { gm_set_error("pair %d, mate %d: QUAL string of %d characters for %d bases", i, m + 1, (int)(e - p), len[m]); return GM_E_ARG; }
        qptr[m].push_back(p); p = *e ? e + 1 : e;
      }
    }
  int nthreads = (int)std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
  if (const char* e = getenv("GM_HOST_THREADS")) nthreads = std::max(1, atoi(e));
  auto parallel_chunks = [&](int nchunks, const std::function<void(int)>& fn) {
    std::atomic<int> next(0);
    auto worker = [&]() { for (;;) { int c = next.fetch_add(1); if (c >= nchunks) break; fn(c); } };
    gm_run_on_threads(std::min(nthreads, nchunks), worker);
  };
  GmScoreDev sc_half = s->sc;                                                         // per-mate threshold of the paired pass 2, ref: gmapper.c:2677
  if (s->P.sw_full_threshold < 0) { sc_half.full_thr_frac = -1.0; sc_half.full_abs = (int)(-(s->P.sw_full_threshold * 0.5)); }
  else sc_half.full_thr_frac = (s->P.sw_full_threshold * 0.5) / 100.0;
  const int cs9[9] = {s->P.match_score, s->P.mismatch_score, s->P.crossover_score, -s->P.a_gap_open_score, -s->P.a_gap_extend_score,
                      -s->P.b_gap_open_score, -s->P.b_gap_extend_score, s->P.anchor_width, s->P.indel_taboo_len};   // sw_full_cs_setup's arguments (ref: gmapper.c:2944-2947)
  std::vector<std::string> pieces_all; uint64_t matched = 0, records = 0;
  std::vector<unsigned long long> hraw((size_t)GS_STRIPES * GS_STRIDE); unsigned long long hs[GS_N];
  auto fold = [&]() { for (int k = 0; k < GS_N; k++) { hs[k] = 0; for (int t = 0; t < GS_STRIPES; t++) hs[k] += hraw[(size_t)t * GS_STRIDE + k]; } };
  const bool timing = gm_tune("GM_TIMING") != nullptr;
  // front of one sub-batch on buffer pair k: reads in (stream C, so that the call never queues behind kernels), K1 + K1b + K2 for both mates
  // -n 4 without half-paired: k_mp_filter works on the survivor lists in LDS; a sub-batch in which some pair did not fit its tiers (or a read-strand went to the heavy
  // tier, which re-emits without the mate's counts) is redone through the generic kernel's mate-pair modes (rows of regions marked twice, then rule 1: GmMpDev mode 5),
  // and so is the rest of the call
  bool mp_exact = gm_tune("GM_MP_EXACT") != nullptr;
  GmIndexDev dkm[2][2] = {{dvm[0], dvm[1]}, {dvm[0], dvm[1]}};     // match modes 3 / 2: each mate's view with its mate-pair fields, per buffer pair (the heavy tier reads it again)
  auto front = [&](int k, int base, int n) -> int {
    unsigned long long* dst = s->d_pstats[k];
    GM_HIP(hipMemsetAsync(dst, 0, (size_t)GS_STRIPES * GS_STRIDE * 8, qa));
    for (int m = 0; m < 2; m++)
      GM_HIP(hipMemcpyAsync(PS[k][m]->d_reads, mates[m] + (size_t)base * rwords[m], (size_t)n * rwords[m] * 4, hipMemcpyHostToDevice, s->stream_c));
    if (cs) for (int m = 0; m < 2; m++) GM_HIP(hipMemcpyAsync(PS[k][m]->d_initbp, initbp_in[m] + base, (size_t)n, hipMemcpyHostToDevice, s->stream_c));
    for (int m = 0; m < 2; m++) PS[k][m]->xover_on = false;
    if (cs && quals1) for (int m = 0; m < 2; m++) {              // per-position crossover scores from the QVs, ref: gmapper.c:532-544 (as in map_impl)
      std::vector<int8_t> xbuf((size_t)n * len[m]);
      for (int i = 0; i < n; i++) {
        const char* qv_s = qptr[m][base + i];
        for (int j = 0; j < len[m]; j++) {
          const int qv = (int)qv_s[j] - qual_delta;
          const double pe = qv <= 0 ? .99999999 : (qv >= 250 ? 1E-25 : pow(10.0, -(double)qv / 10.0));   // pr_err_from_qv, ref: util.h:285-293
          int cx = (int)(s->score_alpha * log(pe / 3.0) / log(2.0));
          if (cx > -1) cx = -1; else if (cx < 2 * s->P.crossover_score) cx = 2 * s->P.crossover_score;
          xbuf[(size_t)i * len[m] + j] = (int8_t)cx;
        }
      }
      GM_HIP(hipMemcpyAsync(PS[k][m]->d_xover, xbuf.data(), xbuf.size(), hipMemcpyHostToDevice, s->stream_c));
      GM_HIP(hipStreamSynchronize(s->stream_c));                // xbuf goes out of scope
      PS[k][m]->xover_on = true;
    }
    GM_HIP(hipEventRecord(s->pev[k][8], s->stream_c));
    GM_HIP(hipStreamWaitEvent(qa, s->pev[k][8], 0));
    if (pmode != 4 || (mp_counts && mp_exact)) {
      // -n 2: the lookup keeps every list entry.  -n 3: a first lookup pass lists, per read-strand, the regions it marked twice; the second keeps the entries of such
      // regions and of regions within reach of one the mate (other strand) marked twice -- count_main >= 2 || count_mp >= 2, use_mp_region_counts == 2; without
      // half-paired a pass in between flags, in each row, the regions the mate reaches at all, and the rule is count_mp >= 1 && count_main + count_mp >= 3
      // (GmMpDev modes 1, 2 / 3 + 4).  No prune rules in either mode: K2 takes the rows as they are.
      const MpDelta dl = gm_mp_region_deltas(ix->params.region_bits, dmin, dmax, dmin2, dmax2);
      int rc;
      for (int m = 0; m < 2; m++) {
        DevSet& D = *PS[k][m];
        if (D.d_read_rna) { rc = gm_launch_read_rna_flags(D.d_reads, n, len[m], rwords[m], D.d_read_rna, qa); if (rc) return rc; }      // (before the mate is turned: its complement of U is A)
        if (in_st[m] && !cs) { rc = gm_launch_revcomp_reads(D.d_reads, n, len[m], rwords[m], qa, D.d_read_rna); if (rc) return rc; }
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
          rc = gm_launch_lookup(gm_view_of(d1, D), D.d_reads, n, len[m], rwords[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_heavy_list, D.d_heavy_cnt, 2 * D.eff_batch, dst, qa, &s->k1, nullptr, nullptr);
          if (rc) return rc;
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
          for (int m = 0; m < 2; m++) {
            DevSet& D = *PS[k][m];
            GmIndexDev d3 = dkm[k][m]; d3.mp.mode = 3;
            rc = gm_launch_lookup(gm_view_of(d3, D), D.d_reads, n, len[m], rwords[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_heavy_list, D.d_heavy_cnt, 2 * D.eff_batch, dst, qa, &s->k1, nullptr, nullptr);
            if (rc) return rc;
          }
      }
      for (int m = 0; m < 2; m++) {
        DevSet& D = *PS[k][m];
        GM_HIP(hipEventRecord(s->pkev[k][2 * m], qa));
        rc = gm_launch_lookup(gm_view_of(dkm[k][m], D), D.d_reads, n, len[m], rwords[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_heavy_list, D.d_heavy_cnt, 2 * D.eff_batch, dst, qa, &s->k1, D.d_surv_seg, nullptr);
        if (rc) return rc;
        GM_HIP(hipEventRecord(s->pkev[k][2 * m + 1], qa));
      }
      for (int m = 0; m < 2; m++) {
        DevSet& D = *PS[k][m];
        GmIndexDev dk2 = dv; dk2.mp = dkm[k][m].mp;
        if (pmode != 4) rc = gm_launch_anchors(dk2, scp, n, len[m], W[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, dst, qa);
        else if (D.scap <= 4096) rc = gm_launch_anchors(dv, s->sc, n, len[m], W[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, dst, qa);
        else rc = launch_prune_anchors(s, D, dv, n, len[m], W[m], dst, 0);         // (-n 4: the prune rules hold; what K1b cannot hold goes to the heavy tier, which runs mode 5 too)
        if (rc) return rc;
        GM_HIP(hipMemcpyAsync(&s->h_pin[2 + 2 * k + m], D.d_heavy_cnt, 4, hipMemcpyDeviceToHost, qa));
      }
    } else
    if (mp_counts) {   // K1 of both mates (never fused with the prune: the filter needs every survivor), the mate-pair filter, then K1b + K2 of both
      for (int m = 0; m < 2; m++) {
        DevSet& D = *PS[k][m];
        int rc;
        if (D.d_read_rna) { rc = gm_launch_read_rna_flags(D.d_reads, n, len[m], rwords[m], D.d_read_rna, qa); if (rc) return rc; }      // (before the mate is turned: its complement of U is A)
        if (in_st[m] && !cs) { rc = gm_launch_revcomp_reads(D.d_reads, n, len[m], rwords[m], qa, D.d_read_rna); if (rc) return rc; }
        GM_HIP(hipEventRecord(s->pkev[k][2 * m], qa));
        rc = gm_launch_lookup(gm_view_of(dvm[m], D), D.d_reads, n, len[m], rwords[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_heavy_list, D.d_heavy_cnt, 2 * D.eff_batch, dst, qa, &s->k1, D.d_surv_seg, nullptr);
        if (rc) return rc;
        GM_HIP(hipEventRecord(s->pkev[k][2 * m + 1], qa));
      }
      int rc = gm_launch_mp_filter(n, ix->params.region_bits, ix->params.region_overlap, PS[k][0]->d_surv, PS[k][0]->d_surv_cnt, PS[k][0]->scap,
                                   PS[k][1]->d_surv, PS[k][1]->d_surv_cnt, PS[k][1]->scap, dmin, dmax, dmin2, dmax2, PS[k][0]->d_surv_seg, PS[k][1]->d_surv_seg, ix->n_slabs, dst, qa);
      if (rc) return rc;
      for (int m = 0; m < 2; m++) {
        DevSet& D = *PS[k][m];
        // K2 straight on the filtered survivors when its LDS tier can take a whole row (small and medium genomes): K1b's overflow goes to the heavy tier,
        // which re-emits a read-strand's survivors from the index -- without the mate's counts.  Larger rows keep K1b; a heavy read-strand then has
        // the anchors of the half-paired run (a superset: the filter only removes list entries that cannot pair up).
        if (D.scap <= 4096) rc = gm_launch_anchors(dv, s->sc, n, len[m], W[m], D.d_surv, D.d_surv_cnt, D.scap, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, dst, qa);
        else rc = launch_prune_anchors(s, D, dv, n, len[m], W[m], dst, 0);
        if (rc) return rc;
        GM_HIP(hipMemcpyAsync(&s->h_pin[2 + 2 * k + m], D.d_heavy_cnt, 4, hipMemcpyDeviceToHost, qa));
      }
    } else
    for (int m = 0; m < 2; m++) {
      DevSet& D = *PS[k][m];
      int rc;
      if (D.d_read_rna) { rc = gm_launch_read_rna_flags(D.d_reads, n, len[m], rwords[m], D.d_read_rna, qa); if (rc) return rc; }      // (before the mate is turned: its complement of U is A)
      if (in_st[m] && !cs) { rc = gm_launch_revcomp_reads(D.d_reads, n, len[m], rwords[m], qa, D.d_read_rna); if (rc) return rc; }   // read_reverse, ref: gmapper.c:174-185,567-570
      rc = stage_windows_async(s, D, dvm[m], n, len[m], dst, &s->h_pin[2 + 2 * k + m], s->pkev[k][2 * m], s->pkev[k][2 * m + 1]); if (rc) return rc;
    }
    GM_HIP(hipEventRecord(s->pev[k][6], qa));
    return GM_OK;
  };
  // The output stage of a sub-batch (unpaired selection, mapping qualities, text: ~6 of a sub-batch's ~70 ms, all host) runs on a thread of its own beside the device work of
  // the next sub-batch; at most one is outstanding, and its text is appended -- in order -- before the next one starts.
  struct OutJob { std::thread th; std::vector<std::string> outs; std::vector<uint64_t> cm, cr; double ms = 0; bool failed = false; ~OutJob() { if (th.joinable()) th.join(); } };
  std::unique_ptr<OutJob> pending;
  bool out_failed = false;                                    // (an allocation failed on the output thread: no exception leaves a thread; the call ends with GM_E_NOMEM)
  auto finish_pending = [&]() {
    if (!pending) return;
    if (pending->th.joinable()) pending->th.join();
    out_failed = out_failed || pending->failed;
    if (stats) stats->ms_host += pending->ms;
    for (size_t c = 0; c < pending->outs.size(); c++) { matched += pending->cm[c]; records += pending->cr[c]; pieces_all.push_back(std::move(pending->outs[c])); }
    pending.reset();
  };
  int cur = 0, front_n = 0, out_idx = 0; bool have_front = false;
  for (int base = 0; base < n_pairs;) {
    const int pinset = (out_idx & 1) * 4;
    auto tw = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (timing) { GM_HIP(hipStreamSynchronize(q)); auto n2 = std::chrono::steady_clock::now(); fprintf(stderr, "  pairs %-18s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(n2 - tw).count()); tw = n2; } return 0; };
    DevSet& A = *PS[cur][0]; DevSet& Bs = *PS[cur][1]; DevSet* S[2] = {&A, &Bs};
    unsigned long long* const dst = s->d_pstats[cur];
    const int B = std::min(A.eff_batch, Bs.eff_batch);
    const int n = have_front ? front_n : std::min(B, n_pairs - base);
    if (s->pairs_cap < B) {
      if (s->d_pairs) (void)hipFree(s->d_pairs);
      if (s->d_pair_cnt) (void)hipFree(s->d_pair_cnt);
      s->d_pairs = nullptr; s->d_pair_cnt = nullptr; s->pairs_cap = 0;
      GM_HIP(hipMalloc(&s->d_pairs, (size_t)B * GM_SEL_MAX * 4)); GM_HIP(hipMalloc(&s->d_pair_cnt, (size_t)B * 4)); s->pairs_cap = B;
    }
    bool retry = false;
    auto grow = [&](bool hits_ovf, const uint32_t n_work[2]) -> int {
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
      return GM_OK;
    };
    int rc;
    if (!have_front) { rc = front(cur, base, n); if (rc) return rc; }
    bool have_next = false; int next_n = 0;
    if (overlap && base + n < n_pairs) {
      next_n = std::min(std::min(PS[cur ^ 1][0]->eff_batch, PS[cur ^ 1][1]->eff_batch), n_pairs - (base + n));
      rc = front(cur ^ 1, base + n, next_n); if (rc) return rc;
      have_next = true;
    }
    // a capacity of this pair grew: the sub-batch is redone from its front, and the front queued for the next one is dropped
    auto redo = [&]() -> int { GM_HIP(hipStreamSynchronize(qa)); GM_HIP(hipStreamSynchronize(q)); have_front = false; if (stats) stats->retries++; return GM_OK; };
    GM_HIP(hipEventSynchronize(s->pev[cur][6]));
    {
      float k1 = 0;
      for (int m = 0; m < 2; m++) {                            // K1's own time for both mate sets of this sub-batch (bench.py's roofline leg)
        float ms = 0; GM_HIP(hipEventElapsedTime(&ms, s->pkev[cur][2 * m], s->pkev[cur][2 * m + 1]));
        if (stats) stats->ms_lookup += ms;
        s->last_lookup_ms += ms; s->last_lookup_launches++; k1 += ms;
      }
      // the rest of the front (K1b, K2, the mate-pair filter of --no-half-paired): from the first K1's begin to the front's end, minus the two K1s
      float span = 0; GM_HIP(hipEventElapsedTime(&span, s->pkev[cur][0], s->pev[cur][6]));
      if (stats) stats->ms_anchors += std::max(0.0f, span - k1);
    }
    // stage times of the back part (gm_map_stats_t, as the unpaired path fills them): events on the back stream, read behind the synchronisation points that exist anyway
    auto stage_ms = [&](int e0, int e1, double gm_map_stats_t::* field) -> int {
      float ms = 0; GM_HIP(hipEventElapsedTime(&ms, s->ev[e0], s->ev[e1])); if (stats) stats->*field += ms; return GM_OK; };
    if (mp_counts && !mp_exact && (s->h_pin[2 + 2 * cur] || s->h_pin[2 + 2 * cur + 1])) { mp_exact = true; rc = redo(); if (rc) return rc; continue; }   // (see mp_exact)
    {
      bool heavy = false;
      for (int m = 0; m < 2; m++) {
        const uint32_t n_heavy = s->h_pin[2 + 2 * cur + m];
        if (n_heavy) {
          rc = (pmode == 4 && !mp_exact) ? run_heavy_tier(s, *S[m], dvm[m], n, len[m], rwords[m], W[m], (int)n_heavy, dst)
                          : run_heavy_tier(s, *S[m], dkm[cur][m], n, len[m], rwords[m], W[m], (int)n_heavy, dst, pmode == 4 ? nullptr : &scp);
          if (rc) return rc; heavy = true;
        }
      }
      if (heavy) GM_HIP(hipEventRecord(s->pev[cur][6], qa));
    }
    GM_HIP(hipStreamWaitEvent(q, s->pev[cur][6], 0));
    lap("K1+K1b+K2 x2");
    GM_HIP(hipEventRecord(s->ev[0], q));
    rc = gm_launch_pair_up(n, A.d_hits, A.d_perm, A.d_hit_cnt, A.hcap, Bs.d_hits, Bs.d_perm, Bs.d_hit_cnt, Bs.hcap,
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
    uint32_t n_work[2] = {0, 0};
    for (int m = 0; m < 2; m++) {
      DevSet& D = *S[m];
      rc = gm_launch_build_work(n, D.d_sel_cnt, D.d_sel_off, D.d_work, D.d_n_work, q); if (rc) return rc;
      GM_HIP(hipMemcpyAsync(&n_work[m], D.d_n_work, 4, hipMemcpyDeviceToHost, q));
    }
    GM_HIP(hipEventRecord(s->ev[2], q));
    GM_HIP(hipMemcpyAsync(hraw.data(), dst, hraw.size() * 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    fold();
    rc = stage_ms(0, 1, &gm_map_stats_t::ms_pass1); if (rc) return rc;        // (pair_up + the mates' own pass 1)
    rc = stage_ms(1, 2, &gm_map_stats_t::ms_select); if (rc) return rc;
    if (hs[GS_OVERFLOW_SURV]) { gm_set_error("heavy list overflow"); return GM_E_OVERFLOW; }
    if ((pmode == 3 || (mp_counts && mp_exact)) && hs[GS_MP_UNFILTERED]) {   // a row of regions marked twice beyond GM_MP_CAP: no exact answer
      gm_set_error("gm_map_pairs: mate-pair region counts: %llu read-strands beyond the row capacity (%d regions marked twice)", hs[GS_MP_UNFILTERED], GM_MP_CAP); return GM_E_OVERFLOW;
    }
    if (mp_counts && !mp_exact && hs[GS_MP_UNFILTERED]) { mp_exact = true; rc = redo(); if (rc) return rc; continue; }   // (see mp_exact)
    rc = grow(hs[GS_OVERFLOW_HITS] != 0, n_work); if (rc) return rc;
    if (retry) { rc = redo(); if (rc) return rc; continue; }
    lap("pair_select");
    // paired pass 2 on the unique windows of the selected pairs
    GmPinVec<GmFullRes>* const resP = &s->pin_res[pinset]; GmPinVec<uint8_t>* const opsP = &s->pin_ops[pinset]; std::vector<uint32_t> cntP[2], offP[2];      // (pinned: the copies run at link rate beside the kernels)
    std::vector<uint32_t> plist((size_t)n * GM_SEL_MAX), pcnt(n);
    GM_HIP(hipEventRecord(s->ev[3], q));
    for (int m = 0; m < 2; m++) {
      DevSet& D = *S[m];
      if (m == 1) GM_HIP(hipEventRecord(s->ev[4], q));          // (between the mates: the first one's copies are queued behind this)
      if (cs) rc = gm_launch_pass2_cs(dvm[m], sc_half, cs9, D.d_reads, D.d_initbp, n, len[m], rwords[m], W[m], D.d_hits, D.hcap, D.d_sel, D.d_work, D.d_n_work,
                                      D.d_res, D.d_ops, D.ops_stride, (uint32_t*)D.d_back, D.back_stride / 4, D.p2_grid, dst, q, D.xover_on ? D.d_xover : nullptr, D.d_sel_sidx, D.d_p2_order, D.d_p2_cls);
      else
      rc = gm_launch_pass2(gm_view_of(dv, D), sc_half, D.d_reads, n, len[m], rwords[m], W[m], D.d_hits, D.d_perm, D.hcap, D.d_sel, D.d_sel_cnt, D.d_work, D.d_n_work,
                           D.d_res, D.d_ops, D.ops_stride, D.d_back, D.back_stride, D.p2_grid, dst, q, D.d_sel_sidx, in_st[m], 1, D.d_p2_order, D.d_p2_cls);
      if (rc) return rc;
      if (m == 1) GM_HIP(hipEventRecord(s->ev[5], q));
      rc = resP[m].resize(n_work[m]); if (rc) return rc; rc = opsP[m].resize((size_t)n_work[m] * D.ops_stride); if (rc) return rc; cntP[m].resize(n); offP[m].resize(n);
      if (n_work[m]) {
        GM_HIP(hipMemcpyAsync(resP[m].data(), D.d_res, (size_t)n_work[m] * sizeof(GmFullRes), hipMemcpyDeviceToHost, q));
        GM_HIP(hipMemcpyAsync(opsP[m].data(), D.d_ops, (size_t)n_work[m] * D.ops_stride, hipMemcpyDeviceToHost, q));
      }
      GM_HIP(hipMemcpyAsync(cntP[m].data(), D.d_sel_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, q));
      GM_HIP(hipMemcpyAsync(offP[m].data(), D.d_sel_off, (size_t)n * 4, hipMemcpyDeviceToHost, q));
    }
    GM_HIP(hipMemcpyAsync(plist.data(), s->d_pairs, plist.size() * 4, hipMemcpyDeviceToHost, q));
    GM_HIP(hipMemcpyAsync(pcnt.data(), s->d_pair_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    rc = stage_ms(3, 4, &gm_map_stats_t::ms_pass2); if (rc) return rc;        // (mate 0's pass 2 with its result copies, then mate 1's kernel)
    rc = stage_ms(4, 5, &gm_map_stats_t::ms_pass2); if (rc) return rc;
    lap("pass2 (pairs)+copy");
    // host: pair selection
    const int chunk = 2048, nchunks = (n + chunk - 1) / chunk;
    std::vector<FHit> fhP[2]; fhP[0].resize(n_work[0]); fhP[1].resize(n_work[1]);
    const int NO = std::max(1, s->P.num_outputs);
    std::vector<PPair> fpairs((size_t)n * NO); std::vector<int> fcnt(n, 0);
    std::vector<std::vector<uint32_t>> saved_chunks[2]; saved_chunks[0].resize(nchunks); saved_chunks[1].resize(nchunks);
    Finalizer F0{s, len[0], rwords[0], nullptr, nullptr, nullptr, 0}, F1{s, len[1], rwords[1], nullptr, nullptr, nullptr, 0};
    if (s->P.output_format) F0.hgen = F1.hgen = s->h_genome.data();
    if (cs) {   // post_sw needs the colours and the primer letter of each read (ref: sw-post.c:448-528)
      F0.reads = mates[0] + (size_t)base * rwords[0]; F1.reads = mates[1] + (size_t)base * rwords[1];
      F0.initbp = initbp_in[0] + base; F1.initbp = initbp_in[1] + base;
      F0.ops_half = A.ops_stride / 2; F1.ops_half = Bs.ops_stride / 2; F0.csk = F1.csk = cs_post_consts(s);
      if (quals1) { F0.qual_ptr = qptr[0].data() + base; F1.qual_ptr = qptr[1].data() + base; F0.qual_delta = F1.qual_delta = qual_delta; }   // post_sw with the reads' QVs (ref: sw-post.c:486-491)
    }
    parallel_chunks(nchunks, [&](int c) {
      std::vector<PPair> v;
      for (int pr = c * chunk; pr < std::min(n, (c + 1) * chunk); pr++) {
        FHit* H[2] = {fhP[0].data() + offP[0][pr], fhP[1].data() + offP[1][pr]};
        for (uint32_t a = 0; a < cntP[0][pr]; a++) F0.post_sw(H[0][a], &resP[0][offP[0][pr] + a], opsP[0].data());
        for (uint32_t b = 0; b < cntP[1][pr]; b++) F1.post_sw(H[1][b], &resP[1][offP[1][pr] + b], opsP[1].data());
        pair_pass2(C, H, plist.data() + (size_t)pr * GM_SEL_MAX, (int)pcnt[pr], v);
        fcnt[pr] = (int)v.size();
        for (size_t j = 0; j < v.size(); j++) {
          fpairs[(size_t)pr * NO + j] = v[j];
          for (int m = 0; m < 2; m++) saved_chunks[m][c].push_back(H[m][v[j].h[m]].r->hit_slot);   // ref: mapping.c:2304-2310
        }
      }
    });
    lap("host pair select");
    // device: half-paired fall-back -- handle_read per mate with the windows already there (ref: mapping.c:2598-2625, gmapper.c:2700-2714)
    GmPinVec<GmFullRes>* const resU = &s->pin_res[pinset + 2]; GmPinVec<uint8_t>* const opsU = &s->pin_ops[pinset + 2]; std::vector<uint32_t> cntU[2], offU[2];
    if (O.half_paired) {
      uint32_t n_work2[2] = {0, 0};
      for (int m = 0; m < 2; m++) {
        DevSet& D = *S[m];
        std::vector<uint32_t> sl; for (auto& v : saved_chunks[m]) sl.insert(sl.end(), v.begin(), v.end());
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
      if (retry) { rc = redo(); if (rc) return rc; continue; }
      GM_HIP(hipEventRecord(s->ev[0], q));
      for (int m = 0; m < 2; m++) {
        DevSet& D = *S[m];
        if (m == 1) GM_HIP(hipEventRecord(s->ev[1], q));
        if (cs) rc = gm_launch_pass2_cs(dvm[m], s->sc, cs9, D.d_reads, D.d_initbp, n, len[m], rwords[m], W[m], D.d_hits, D.hcap, D.d_sel, D.d_work, D.d_n_work,
                                        D.d_res, D.d_ops, D.ops_stride, (uint32_t*)D.d_back, D.back_stride / 4, D.p2_grid, dst, q, D.xover_on ? D.d_xover : nullptr, nullptr, D.d_p2_order, D.d_p2_cls);
        else
        rc = gm_launch_pass2(gm_view_of(dv, D), s->sc, D.d_reads, n, len[m], rwords[m], W[m], D.d_hits, D.d_perm, D.hcap, D.d_sel, D.d_sel_cnt, D.d_work, D.d_n_work,
                             D.d_res, D.d_ops, D.ops_stride, D.d_back, D.back_stride, D.p2_grid, dst, q, nullptr, in_st[m], 0, D.d_p2_order, D.d_p2_cls);
        if (rc) return rc;
        if (m == 1) GM_HIP(hipEventRecord(s->ev[2], q));
        rc = resU[m].resize(n_work2[m]); if (rc) return rc; rc = opsU[m].resize((size_t)n_work2[m] * D.ops_stride); if (rc) return rc; cntU[m].resize(n); offU[m].resize(n);
        if (n_work2[m]) {
          GM_HIP(hipMemcpyAsync(resU[m].data(), D.d_res, (size_t)n_work2[m] * sizeof(GmFullRes), hipMemcpyDeviceToHost, q));
          GM_HIP(hipMemcpyAsync(opsU[m].data(), D.d_ops, (size_t)n_work2[m] * D.ops_stride, hipMemcpyDeviceToHost, q));
        }
        GM_HIP(hipMemcpyAsync(cntU[m].data(), D.d_sel_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, q));
        GM_HIP(hipMemcpyAsync(offU[m].data(), D.d_sel_off, (size_t)n * 4, hipMemcpyDeviceToHost, q));
      }
    } else { for (int m = 0; m < 2; m++) { cntU[m].assign(n, 0); offU[m].assign(n, 0); } }
    GM_HIP(hipMemcpyAsync(hraw.data(), dst, hraw.size() * 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    fold();
    if (O.half_paired) { rc = stage_ms(0, 1, &gm_map_stats_t::ms_pass2); if (rc) return rc; rc = stage_ms(1, 2, &gm_map_stats_t::ms_pass2); if (rc) return rc; }      // the rescue's pass 2
    if (stats) {
      stats->lookups += hs[GS_LOOKUPS]; stats->list_entries += hs[GS_ENTRIES]; stats->list_bytes += 12ull * hs[GS_LOOKUPS] + 4ull * hs[GS_ENTRIES];
      stats->survivors += hs[GS_SURVIVORS]; stats->anchors += hs[GS_ANCHORS]; stats->windows += hs[GS_WINDOWS];
      stats->vec_calls += hs[GS_VEC_CALLS]; stats->vec_cells += hs[GS_VEC_CELLS]; stats->vec_bypassed += hs[GS_VEC_BYPASSED];
      stats->full_calls += hs[GS_FULL_CALLS]; stats->full_cells += hs[GS_FULL_CELLS]; stats->exact_order_reads += hs[GS_EXACT_ORDER]; stats->survivors_pruned += hs[GS_PRUNED];
      stats->mp_unfiltered += hs[GS_MP_UNFILTERED];
    }
    lap("rescue p1+sel+p2");
    // host: unpaired selection, mapping qualities, SAM text (readpair_output, ref: output.c:1070-1291) -- on its own thread, see OutJob above
    finish_pending();                                              // (the sub-batch before this one: its text comes first, and its pinned result set is free again after this)
    {
      struct OutState { std::vector<FHit> fhP[2]; std::vector<PPair> fpairs; std::vector<int> fcnt; std::vector<uint32_t> offP[2], cntU[2], offU[2]; };
      auto st = std::make_shared<OutState>();
      for (int m = 0; m < 2; m++) { st->fhP[m] = std::move(fhP[m]); st->offP[m] = std::move(offP[m]); st->cntU[m] = std::move(cntU[m]); st->offU[m] = std::move(offU[m]); }
      st->fpairs = std::move(fpairs); st->fcnt = std::move(fcnt);
      std::unique_ptr<OutJob> J(new OutJob());
      J->outs.assign(nchunks, std::string()); J->cm.assign(nchunks, 0); J->cr.assign(nchunks, 0);
      OutJob* const jp = J.get();
      const int os0 = A.ops_stride, os1 = Bs.ops_stride;
      const PairCtx* const Cp = &C; const std::vector<const char*>* const nptr_p = nptr; const std::vector<int>* const nlen_p = nlen; const std::vector<const char*>* const qptr_p = qptr;
      const uint32_t* const mates0 = mates[0]; const uint32_t* const mates1 = mates[1]; const uint8_t* const ib_in0 = initbp_in[0]; const uint8_t* const ib_in1 = initbp_in[1];
      const int len0 = len[0], len1_ = len[1], rw0n = rwords[0], rw1n = rwords[1];
      const auto* const pc = &parallel_chunks;
      jp->th = std::thread([jp, st, n, base, chunk, nchunks, NO, F0, F1, resU, opsU, os0, os1, Cp, nptr_p, nlen_p, qptr_p, mates0, mates1, ib_in0, ib_in1, len0, len1_, rw0n, rw1n, pc,
                            s, names1, names2, quals1, quals2, cs, qual_delta, per_pair_bytes]() {
        try {
        const auto t0 = std::chrono::steady_clock::now();
        const PairCtx& C = *Cp; const std::vector<const char*>* nptr = nptr_p; const std::vector<int>* nlen = nlen_p; const std::vector<const char*>* qptr = qptr_p;
        const uint32_t* const mates[2] = {mates0, mates1}; const uint8_t* const initbp_in[2] = {ib_in0, ib_in1};
        const int len[2] = {len0, len1_}, rwords[2] = {rw0n, rw1n};
        std::vector<FHit>* const fhP = st->fhP; std::vector<uint32_t>* const offP = st->offP; std::vector<uint32_t>* const cntU = st->cntU; std::vector<uint32_t>* const offU = st->offU;
        std::vector<PPair>& fpairs = st->fpairs; std::vector<int>& fcnt = st->fcnt;
        std::vector<std::string>& outs = jp->outs; std::vector<uint64_t>& cm = jp->cm; std::vector<uint64_t>& cr = jp->cr;
        const int ops_stride[2] = {os0, os1};
        const auto& parallel_chunks = *pc;
    parallel_chunks(nchunks, [&](int c) {
          std::vector<FHit> fhU[2]; std::vector<FHit*> U[2];
          std::string& o = outs[c]; o.reserve((size_t)chunk * (len[0] + len[1] + 300));
          char qbuf[40];
          for (int pr = c * chunk; pr < std::min(n, (c + 1) * chunk); pr++) {
            const size_t o_before = o.size();
            const long gp = (long)base + pr;
            FHit* HP[2] = {fhP[0].data() + offP[0][pr], fhP[1].data() + offP[1][pr]};
            F0.select_hits(cntU[0][pr] ? &resU[0][offU[0][pr]] : nullptr, opsU[0].data(), (int)cntU[0][pr], fhU[0], U[0]);
            F1.select_hits(cntU[1][pr] ? &resU[1][offU[1][pr]] : nullptr, opsU[1].data(), (int)cntU[1][pr], fhU[1], U[1]);
            const PPair* fp = &fpairs[(size_t)pr * NO]; const int nfp = fcnt[pr];
            // what is printed: paired records [first2, last2) of fp, unpaired ones [firstU[m], lastU[m]) of each mate; --single-best-mapping narrows them and may add
            // one improper pair of two unpaired mappings (ref: output.c:1086-1235)
            int first2 = 0, last2 = nfp, firstU[2] = {0, 0}, lastU[2] = {(int)U[0].size(), (int)U[1].size()};
            const FHit* imp[2] = {nullptr, nullptr};
            if (gm_mqv_on(s->P)) {                                                      // --local / --no-mapping-qualities: none (ref: gmapper.c:2258,2325-2328, output.c:1092)
              compute_paired_mqv(C, HP, fp, nfp, U);
              if (s->P.single_best_mapping && (nfp > 0 || !U[0].empty() || !U[1].empty())) {
                int max_idx_unpaired[2] = {-1, -1}, max_mqv_unpaired[2] = {-1, -1}, max_mqv_paired[2] = {-1, -1}; const FHit* max_hit_paired[2] = {nullptr, nullptr};
                for (int nip = 0; nip < 2; nip++) {
                  for (int i = 0; i < (int)U[nip].size(); i++) if (U[nip][i]->mqv > max_mqv_unpaired[nip]) { max_mqv_unpaired[nip] = U[nip][i]->mqv; max_idx_unpaired[nip] = i; }
                  // the pool of paired hits in the order readpair_save_final_hits builds it: first appearance over the pairs (a repeated hit compares equal: strict >)
                  for (int j = 0; j < nfp; j++) { const FHit* h = &HP[nip][fp[j].h[nip]]; if (h->mqv > max_mqv_paired[nip]) { max_mqv_paired[nip] = h->mqv; max_hit_paired[nip] = h; } }
                }
                // get_idx_mp_max_mqv (ref: output.c:1049-1067): of the pairs that hold hit h of mate nip, the first whose other mate has the best quality
                auto pair_of = [&](int nip, const FHit* h) { int best = -1, idx = -1; for (int j = 0; j < nfp; j++) if (&HP[nip][fp[j].h[nip]] == h) { const int q = HP[1 - nip][fp[j].h[1 - nip]].mqv; if (q > best) { best = q; idx = j; } } return idx; };
                if (!s->P.all_contigs) {
                  for (int nip = 0; nip < 2; nip++) if (max_idx_unpaired[nip] >= 0) { firstU[nip] = max_idx_unpaired[nip]; lastU[nip] = firstU[nip] + 1; }
                  const int best_nip = max_mqv_paired[0] > max_mqv_paired[1] ? 0 : 1;
                  if (max_mqv_paired[best_nip] >= 0) { first2 = pair_of(best_nip, max_hit_paired[best_nip]); last2 = first2 + 1; }
                } else {
                  int max_mqv[2]; bool max_is_paired[2];
                  for (int nip = 0; nip < 2; nip++) {
                    if (max_mqv_unpaired[nip] > max_mqv_paired[nip]) { max_mqv[nip] = max_mqv_unpaired[nip]; max_is_paired[nip] = false; }
                    else { max_mqv[nip] = max_mqv_paired[nip]; max_is_paired[nip] = true; }
                  }
                  const int best_nip = max_mqv[0] >= max_mqv[1] ? 0 : 1;
                  if (max_is_paired[best_nip]) { lastU[0] = lastU[1] = 0; first2 = pair_of(best_nip, max_hit_paired[best_nip]); last2 = first2 + 1; }
                  else {
                    int idx_best_other = -1; double max_other_z0 = 0.0;
                    const auto& OU = U[1 - best_nip];
                    for (int i = 0; i < (int)OU.size(); i++) if (OU[i]->z0 > max_other_z0) { max_other_z0 = OU[i]->z0; idx_best_other = i; }
                    int best_other_mqv = -1;
                    if (idx_best_other >= 0) best_other_mqv = qv_from_pr_corr(max_other_z0 / OU[idx_best_other]->z1);
                    if (s->P.no_improper_mappings || max_mqv_unpaired[best_nip] < 10 || best_other_mqv < 10) {
                      last2 = 0; lastU[1 - best_nip] = 0; firstU[best_nip] = max_idx_unpaired[best_nip]; lastU[best_nip] = firstU[best_nip] + 1;
                    } else {                                                            // both good: one improper pair, possibly across contigs
                      imp[best_nip] = U[best_nip][max_idx_unpaired[best_nip]]; imp[1 - best_nip] = OU[idx_best_other];
                      last2 = 0; lastU[0] = lastU[1] = 0;
                    }
                  }
                }
              }
            }
            // QNAME = common prefix of the two names, minus a trailing ':' or '/' (ref: output.c:365-378)
            const char* qn; size_t qnl;
            if (names1 && names2) {
              const char* a = nptr[0][gp]; const char* b = nptr[1][gp]; const size_t na = (size_t)nlen[0][gp], nb = (size_t)nlen[1][gp];
              size_t i = 0; while (i < std::min(na, nb) && a[i] == b[i]) i++;
              if (i > 0 && (a[i - 1] == ':' || a[i - 1] == '/')) i--;
              qn = a; qnl = i;
            } else { qnl = (size_t)snprintf(qbuf, sizeof qbuf, "p%ld", gp); qn = qbuf; }
            const uint32_t* rw0 = mates[0] + (size_t)gp * rwords[0]; const uint32_t* rw1 = mates[1] + (size_t)gp * rwords[1];
            const char* ql0 = quals1 ? qptr[0][gp] : nullptr; const char* ql1 = quals2 ? qptr[1][gp] : nullptr;
            const int ib0 = cs ? (int)initbp_in[0][gp] : -1, ib1 = cs ? (int)initbp_in[1][gp] : -1;
            // --sam-r2: every record carries the MATE's sequence as given (re_mp->seq: letters, or primer + colours; ref: output.c:452-460,729-737)
            std::string mseq[2]; const std::string* ms0 = nullptr; const std::string* ms1 = nullptr;
            if (s->P.sam_r2) {
              for (int m = 0; m < 2; m++) {
                const uint32_t* rw = m ? rw1 : rw0; const int L = len[m];
                if (cs) { mseq[m] += "ACGT"[(m ? ib1 : ib0) & 3]; for (int i = 0; i < L; i++) { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; mseq[m] += (c < 4) ? (char)('0' + c) : '.'; } }
                else for (int i = 0; i < L; i++) { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; mseq[m] += (c < 4) ? "ACGT"[c] : (c == 4 ? 'U' : 'N'); }
              }
              ms0 = &mseq[1]; ms1 = &mseq[0];                                            // (mate 1's records carry mate 2's sequence and the other way round)
            }
            uint64_t k = 0;
            if (s->P.output_format) {
              // --shrimp-format / -P: one line (block) per mapped mate under the mate's own name, ">name" for the unmapped mate of a half-paired
              // mapping (ref: gmapper/output.c:270-296, hit_output called per mate by readpair_output :1070-1291)
              std::string db, qr;
              auto one = [&](int m, const FHit* rh) {
                const char* nm = qn; size_t nl = qnl;
                if (names1 && names2) { nm = nptr[m][gp]; nl = (size_t)nlen[m][gp]; }
                if (!rh) { o += '>'; o.append(nm, nl); o += '\n'; return; }
                const Finalizer& F = m ? F1 : F0; const uint32_t* rw = m ? rw1 : rw0;
                if (cs) F.emit_shrimp(*rh, nm, nl, pr, rw, rh->db, rh->qr, o);
                else { F.ls_alignment_strings(*rh->r, rh->ops, std::min(rh->r->n_ops, ops_stride[m]), rw, db, qr); F.emit_shrimp(*rh, nm, nl, pr, rw, db, qr, o); }
              };
              for (int j = first2; j < last2; j++) { one(0, &HP[0][fp[j].h[0]]); one(1, &HP[1][fp[j].h[1]]); k += 2; }
              if (imp[0]) { one(0, imp[0]); one(1, imp[1]); k += 2; }
              for (int i = firstU[0]; i < lastU[0]; i++) { one(0, U[0][i]); one(1, nullptr); k += 2; }
              for (int i = firstU[1]; i < lastU[1]; i++) { one(0, nullptr); one(1, U[1][i]); k += 2; }
              if (nfp > 0 || !U[0].empty() || !U[1].empty()) cm[c]++;
              cr[c] += k;
              if (per_pair_bytes) per_pair_bytes[gp] = (uint32_t)(o.size() - o_before);
              continue;
            }
            for (int j = first2; j < last2; j++) {
              const FHit* h1 = &HP[0][fp[j].h[0]]; const FHit* h2 = &HP[1][fp[j].h[1]];
              emit_pair_record(C, o, qn, qnl, rw0, len[0], ops_stride[0], h1, h2, true, false, ql0, qual_delta, ib0, ms0);
              emit_pair_record(C, o, qn, qnl, rw1, len[1], ops_stride[1], h2, h1, false, false, ql1, qual_delta, ib1, ms1);
              k += 2;
            }
            if (imp[0]) {
              emit_pair_record(C, o, qn, qnl, rw0, len[0], ops_stride[0], imp[0], imp[1], true, true, ql0, qual_delta, ib0, ms0);
              emit_pair_record(C, o, qn, qnl, rw1, len[1], ops_stride[1], imp[1], imp[0], false, true, ql1, qual_delta, ib1, ms1);
              k += 2;
            }
            for (int ui = firstU[0]; ui < lastU[0]; ui++) { FHit* h = U[0][ui]; emit_pair_record(C, o, qn, qnl, rw0, len[0], ops_stride[0], h, nullptr, true, false, ql0, qual_delta, ib0, ms0); emit_pair_record(C, o, qn, qnl, rw1, len[1], ops_stride[1], nullptr, h, false, false, ql1, qual_delta, ib1, ms1); k += 2; }
            for (int ui = firstU[1]; ui < lastU[1]; ui++) { FHit* h = U[1][ui]; emit_pair_record(C, o, qn, qnl, rw0, len[0], ops_stride[0], nullptr, h, true, false, ql0, qual_delta, ib0, ms0); emit_pair_record(C, o, qn, qnl, rw1, len[1], ops_stride[1], h, nullptr, false, false, ql1, qual_delta, ib1, ms1); k += 2; }
            const bool any = nfp > 0 || !U[0].empty() || !U[1].empty();
            if (!any && s->P.sam_unaligned) {                                               // ref: mapping.c:2627-2633
              emit_pair_record(C, o, qn, qnl, rw0, len[0], ops_stride[0], nullptr, nullptr, true, false, ql0, qual_delta, ib0, ms0);
              emit_pair_record(C, o, qn, qnl, rw1, len[1], ops_stride[1], nullptr, nullptr, false, false, ql1, qual_delta, ib1, ms1);
              k += 2;
            }
            if (any) cm[c]++;
            cr[c] += k;
            if (per_pair_bytes) per_pair_bytes[gp] = (uint32_t)(o.size() - o_before);
          }
        });
        jp->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        } catch (...) { jp->failed = true; }
      });
      pending = std::move(J);
      out_idx++;
    }
    lap("host output");
    base += n;
    if (overlap) cur ^= 1;
    have_front = have_next; front_n = next_n;
  }
  finish_pending();
  if (out_failed) { gm_set_error("gm_map_pairs: out of memory in the output stage"); return GM_E_NOMEM; }
  if (stats) { stats->reads = 2ull * (uint64_t)n_pairs; stats->reads_matched = matched; stats->sam_records = records; }
  size_t total = 0; for (auto& p : pieces_all) total += p.size();
  if (sam) {
    size_t cap = 0; char* r = outcache_take(total + 1, &cap);      // the text buffer of the last call, if it was given back (gm_free parks large ones)
    if (!r) { cap = total + 1 + total / 16; r = (char*)malloc(cap); }      // (some room: the next call's text is a little longer half of the time, and a parked buffer that is too small is a fresh one's page faults)
    if (!r) return GM_E_NOMEM;
    outcache_track(r, cap);
    size_t o = 0; for (auto& p : pieces_all) { memcpy(r + o, p.data(), p.size()); o += p.size(); }
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
