// gm_host_pair_mappings.inc -- paired pass 2 as a seam: gm_pair_mappings (a chunk of read pairs to mapping arrays in one call); part of gm_host.hip.
//
// The call object and the stages are gm_map_pairs' (PairRun, gm_host_pairs.inc): front, finish_front, pass1_select, paired_pass2, rescue, collect_stats, with the same
// sub-batch walk, capacity growth and buffer-set pairs.  Two stages differ.  The pair selection of readpair_pass2 runs on the device (select_pairs_dev: k_pair_sel_items and
// k_sel_pair_pass2, gm_pair_select.hip) where gm_map_pairs runs its host loop, pair_pass2; hit_run_post_sw's doubles stay with the host's libm, so what goes up is one
// score_full a window and what comes down is the final pairs.  And in place of the output thread's text, harvest() hands the sub-batch's results out as arrays: it
// settles every pair through settle_pair -- the unpaired selection, compute_paired_mqv and plan_pair_output that emit_pair calls -- and copies what the plan names.
// Last, k_sw_text over the hits some mapping names (pm_text), as pass2_text does for unpaired reads.

extern "C" int gm_pair_mapping_size(void) { return (int)sizeof(gm_pair_mapping_t); }
extern "C" int gm_pair_mappings_size(void) { return (int)sizeof(gm_pair_mappings_t); }
static_assert(sizeof(gm_pair_mapping_t) == 112, "gm_pair_mapping_t: 12 x 32 bits + 8 doubles");

extern "C" void gm_pair_mappings_free(gm_pair_mappings_t* out) {
  if (!out) return;
  for (int m = 0; m < 2; m++) {
    void* ptrs[] = {out->hits[m], out->hit_off[m], out->hit_kind[m], out->recs[m], out->umaps[m], out->umap_off[m], out->umap_z45[m], out->cigar[m], out->cigar_off[m],
                    out->edit[m], out->edit_off[m], out->ops[m]};
    for (void* p : ptrs) free(p);
  }
  free(out->pmaps); free(out->pmap_off);
  memset(out, 0, sizeof *out);
}

// the integer threshold of readpair_pass2 for two windows whose score_max sum to smax, in the host's own double expression (pair_pass2's; ref: mapping.c:2246-2262)
static inline int gm_pair_thresh_int(const gm_params_t& P, int smax) { return P.sw_full_threshold < 0 ? (int)(-P.sw_full_threshold) : (int)(smax * (P.sw_full_threshold / 100.0)); }

// k_pair_sel_items and k_sel_pair_pass2 over n pairs whose paired pass-2 records are on the device: out[pr * GM_SEL_MAX + k] / cnt[pr], on the host when it returns
static int pair_select_device(hipStream_t q, GmDevMem& mem, const gm_params_t& P, int n, const int* d_thr, int thr_n, const uint32_t* d_plist, const uint32_t* d_pcnt,
                              const GmFullRes* const d_res[2], const std::vector<int32_t> sf[2], const uint32_t* const d_off[2], const uint32_t* const d_cnt[2],
                              std::vector<uint32_t>& out, std::vector<uint32_t>& cnt) {
  GmPairSelItem* d_items[2] = {nullptr, nullptr}; uint32_t *d_out = nullptr, *d_ocnt = nullptr;
  for (int m = 0; m < 2; m++) {
    int32_t* d_sf = nullptr;
    if (sf[m].empty()) continue;
    GM_HIP(mem.up(&d_sf, sf[m].data(), sf[m].size(), q)); GM_HIP(mem.get(&d_items[m], sf[m].size() * sizeof(GmPairSelItem)));
    int rc = gm_launch_pair_sel_items((int)sf[m].size(), d_res[m], d_sf, d_items[m], q); if (rc) return rc;
  }
  GM_HIP(mem.get(&d_out, (size_t)n * GM_SEL_MAX * 4)); GM_HIP(mem.get(&d_ocnt, (size_t)n * 4));
  int rc = gm_launch_sel_pair_pass2(n, P.sw_full_threshold < 0 ? 1 : 0, P.num_outputs, P.strata ? 1 : 0, P.max_alignments, d_thr, thr_n, d_plist, d_pcnt,
                                    d_items[0], d_off[0], d_cnt[0], d_items[1], d_off[1], d_cnt[1], d_out, d_ocnt, q);
  if (rc) return rc;
  out.resize((size_t)n * GM_SEL_MAX); cnt.resize(n);
  GM_HIP(hipMemcpyAsync(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipMemcpyAsync(cnt.data(), d_ocnt, (size_t)n * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  return GM_OK;
}

namespace {
// the call's results so far, on the host; the hits, records and offsets of both mates grow sub-batch by sub-batch
struct PairMapCall {
  bool want_ops = false, want_edit = false;
  std::vector<gm_pass1_hit_t> hits[2]; std::vector<uint64_t> hit_off[2]; std::vector<uint8_t> kind[2]; std::vector<gm_sw_full_rec_t> recs[2];
  std::vector<gm_pair_mapping_t> pmaps; std::vector<uint64_t> pmap_off;
  std::vector<gm_mapping_t> umaps[2]; std::vector<uint64_t> umap_off[2]; std::vector<double> uz[2];
  std::vector<char> cigar[2], edit[2]; std::vector<uint64_t> cigar_off[2], edit_off[2];
  std::vector<uint8_t> ops[2]; uint64_t ops_len[2] = {0, 0};
  uint64_t matched = 0;
  int* d_thr = nullptr; int thr_n = 0;                           // (the call's GmDevMem owns the table)
};
// what a worker leaves of its chunk of pairs: the mappings in pair order, their numbers per pair
struct PairMapChunk { std::vector<gm_pair_mapping_t> pm; std::vector<gm_mapping_t> um[2]; std::vector<double> uz[2]; std::vector<uint32_t> npm, num[2]; uint64_t matched = 0; };

struct PairMapRun : PairRun {
  PairMapCall K;
  // the pair selection of readpair_pass2 on the device: hit_run_post_sw per window on the host threads (as select_pairs_host), one score_full a window up, the final
  // pairs down; compute_paired_hit fills each of them in, and the windows of the final pairs are saved from the rescue
  int select_pairs_dev(PairOut& b, PairSel& t) {
    select_setup(b, t);
    std::vector<int32_t> sf[2]; sf[0].assign(t.n_work[0], 0); sf[1].assign(t.n_work[1], 0);
    parallel_chunks(b.nchunks, [&](int c) {
      for (int pr = c * b.chunk; pr < std::min(b.n, (c + 1) * b.chunk); pr++)
        for (int m = 0; m < 2; m++)
          for (uint32_t a = 0; a < t.cntP[m][pr]; a++) {
            FHit& h = b.fhP[m][b.offP[m][pr] + a];
            b.F[m].post_sw(h, &b.resP[m][b.offP[m][pr] + a], b.opsP[m].data());
            sf[m][b.offP[m][pr] + a] = h.score_full;
          }
    });
    GmDevMem mem; std::vector<uint32_t> out, cnt;
    const GmFullRes* d_res[2] = {S[0]->d_res, S[1]->d_res}; const uint32_t* d_off[2] = {S[0]->d_sel_off, S[1]->d_sel_off}; const uint32_t* d_cnt[2] = {S[0]->d_sel_cnt, S[1]->d_sel_cnt};
    int rc = pair_select_device(q, mem, s->P, b.n, K.d_thr, K.thr_n, s->d_pairs, s->d_pair_cnt, d_res, sf, d_off, d_cnt, out, cnt); if (rc) return rc;
    for (int pr = 0; pr < b.n; pr++) {
      const int c = pr / b.chunk, m2 = (int)cnt[pr];
      if (m2 > b.NO || m2 > GM_SEL_MAX || (uint32_t)m2 > t.pcnt[pr]) { gm_set_error("gm_pair_mappings: pair %d: %d final pairs of %u candidates", b.base + pr, m2, t.pcnt[pr]); return GM_E_OVERFLOW; }
      FHit* H[2] = {b.fhP[0].data() + b.offP[0][pr], b.fhP[1].data() + b.offP[1][pr]};
      b.fcnt[pr] = m2;
      for (int j = 0; j < m2; j++) {
        const uint32_t p = out[(size_t)pr * GM_SEL_MAX + j];
        PPair d; d.h[0] = (int)(p >> 8); d.h[1] = (int)(p & 0xffu);
        if ((uint32_t)d.h[0] >= t.cntP[0][pr] || (uint32_t)d.h[1] >= t.cntP[1][pr]) { gm_set_error("gm_pair_mappings: pair %d: final pair %d names windows %d, %d of %u, %u", b.base + pr, j, d.h[0], d.h[1], t.cntP[0][pr], t.cntP[1][pr]); return GM_E_OVERFLOW; }
        compute_paired_hit(C, H, d);
        b.fpairs[(size_t)pr * b.NO + j] = d;
        for (int m = 0; m < 2; m++) t.saved_chunks[m][c].push_back(H[m][d.h[m]].r->hit_slot);      // ref: mapping.c:2304-2310
      }
    }
    lap("device pair select");
    return GM_OK;
  }

  // a hit and its record from the pipeline's pass-2 result: the window as reverse_hit left it, ZV in score_vector; a window under its threshold has the zero record
  static void fill_hit(int pair, const GmFullRes& r, gm_pass1_hit_t& h, gm_sw_full_rec_t& R) {
    memset(&h, 0, sizeof h); memset(&R, 0, sizeof R);
    h.read = pair; h.st = r.st; h.win = -1; h.cn = (int32_t)r.cn; h.gen_st = r.gen_st; h.g_off = r.g_off; h.w_len = r.w_len;
    h.score_vector = r.score_vector; h.score_max = r.score_max; h.pct_score_vector = r.score_max ? (1000 * 100 * r.score_vector) / r.score_max : 0;
    h.matches = r.matches; h.score_window_gen = r.score_window_gen;
    if (r.score <= 0) return;
    R.score = r.score; R.read_start = r.read_start; R.rmapped = r.rmapped; R.gmapped = r.gmapped; R.matches = r.n_match; R.mismatches = r.n_mismatch;
    R.insertions = r.n_ins; R.deletions = r.n_del; R.genome_start = r.genome_start;
  }

  // The sub-batch's results as arrays.  Serial: the hits, records and operations of every pair, paired hits first, then the rescue's.  On the host threads: settle_pair
  // per pair and the mappings its plan names.  Serial again: the chunks' mappings appended in pair order.  Then the text of the hits some mapping names.
  int harvest(PairOut& b, const PairSel& sel) {
    const std::vector<uint32_t>* const cntP = sel.cntP;
    const int n = b.n;
    size_t hb[2]; std::vector<const uint8_t*> opsptr[2]; std::vector<uint8_t> mapped[2];
    for (int m = 0; m < 2; m++) {
      hb[m] = K.hits[m].size();
      size_t tot = 0; for (int pr = 0; pr < n; pr++) tot += (size_t)cntP[m][pr] + b.cntU[m][pr];
      K.hits[m].resize(hb[m] + tot); K.recs[m].resize(hb[m] + tot); K.kind[m].resize(hb[m] + tot); opsptr[m].assign(tot, nullptr); mapped[m].assign(tot, 0);
      size_t i = hb[m];
      for (int pr = 0; pr < n; pr++) {
        for (int kind = 0; kind < 2; kind++) {
          const uint32_t cn = kind ? b.cntU[m][pr] : cntP[m][pr];
          const GmFullRes* res = kind ? b.resU[m].data() + b.offU[m][pr] : b.resP[m].data() + b.offP[m][pr];
          const uint8_t* ops = kind ? b.opsU[m].data() : b.opsP[m].data();
          for (uint32_t a = 0; a < cn; a++, i++) {
            const GmFullRes& r = res[a];
            fill_hit(b.base + pr, r, K.hits[m][i], K.recs[m][i]); K.kind[m][i] = (uint8_t)kind;
            gm_sw_full_rec_t& R = K.recs[m][i];
            R.ops_off = K.ops_len[m];
            if (r.score > 0) {
              R.n_ops = (uint32_t)std::max(0, std::min(r.n_ops, b.ops_stride[m]));
              opsptr[m][i - hb[m]] = ops + (size_t)r.ops_off;
              if (K.want_ops) K.ops[m].insert(K.ops[m].end(), opsptr[m][i - hb[m]], opsptr[m][i - hb[m]] + R.n_ops);
              K.ops_len[m] += R.n_ops;
            }
          }
        }
        K.hit_off[m].push_back(i);
      }
    }
    std::vector<PairMapChunk> ch(b.nchunks);
    const PairCall& call = *this;
    parallel_chunks(b.nchunks, [&](int c) {
      PairScratch t; PairMapChunk& o = ch[c];
      for (int pr = c * b.chunk; pr < std::min(n, (c + 1) * b.chunk); pr++) {
        const PairPlan p = settle_pair(call, b, pr, t);
        const int gp = b.base + pr;
        FHit* HP[2] = {b.fhP[0].data() + b.offP[0][pr], b.fhP[1].data() + b.offP[1][pr]};
        const PPair* fp = &b.fpairs[(size_t)pr * b.NO];
        // the first hit of the pair in this sub-batch's part of hits[m]; a rescue hit's index within the pair
        size_t first[2]; for (int m = 0; m < 2; m++) first[m] = (size_t)K.hit_off[m][(size_t)gp] - hb[m];
        auto u_local = [&](int m, const FHit* h) { return (int)cntP[m][pr] + (int)(h - t.fhU[m].data()); };
        uint32_t npm = 0;
        for (int j = p.first2; j < p.last2; j++) {
          gm_pair_mapping_t e; memset(&e, 0, sizeof e);
          e.pair = gp; e.score = fp[j].score; e.pct_score = fp[j].pct_score; e.key = fp[j].key; e.insert_size = fp[j].insert_size;
          for (int m = 0; m < 2; m++) {
            const FHit& h = HP[m][fp[j].h[m]];
            e.hit[m] = fp[j].h[m]; e.mapq[m] = h.mqv; e.as[m] = h.score_full;
            e.z[m][0] = h.z2; e.z[m][1] = h.z3; e.z[m][2] = h.pr_top_random; e.z[m][3] = h.insert_size_denom;
            mapped[m][first[m] + (size_t)e.hit[m]] = 1;
          }
          o.pm.push_back(e); npm++;
        }
        if (p.imp[0]) {                                          // the one improper pair of two unpaired mappings (ref: output.c:1178-1226)
          gm_pair_mapping_t e; memset(&e, 0, sizeof e);
          e.pair = gp; e.improper = 1; e.score = p.imp[0]->score_full + p.imp[1]->score_full;
          for (int m = 0; m < 2; m++) {
            const FHit& h = *p.imp[m];
            e.hit[m] = u_local(m, &h); e.mapq[m] = h.mqv; e.as[m] = h.score_full;
            e.z[m][0] = h.z0; e.z[m][1] = h.z1; e.z[m][2] = h.pr_top_random; e.z[m][3] = h.pr_missed_mp;
            mapped[m][first[m] + (size_t)e.hit[m]] = 1;
          }
          o.pm.push_back(e); npm++;
        }
        o.npm.push_back(npm);
        for (int m = 0; m < 2; m++) {
          for (int ui = p.firstU[m]; ui < p.lastU[m]; ui++) {
            const FHit& h = *t.U[m][ui];
            const int loc = u_local(m, &h);
            gm_mapping_t e; e.read = gp; e.hit = (int32_t)(K.hit_off[m][(size_t)gp] + (uint64_t)loc); e.score_full = h.score_full; e.pct_score_full = (int32_t)h.pct_score_full;
            e.mqv = h.mqv; e.flags = 0; e.posterior = h.posterior; e.z0 = h.z0; e.z1 = h.z1;
            o.um[m].push_back(e); o.uz[m].push_back(h.pr_top_random); o.uz[m].push_back(h.pr_missed_mp);
            mapped[m][first[m] + (size_t)loc] = 1;
          }
          o.num[m].push_back((uint32_t)std::max(0, p.lastU[m] - p.firstU[m]));
        }
        if (b.fcnt[pr] > 0 || !t.U[0].empty() || !t.U[1].empty()) o.matched++;
      }
    });
    for (auto& o : ch) {
      K.pmaps.insert(K.pmaps.end(), o.pm.begin(), o.pm.end());
      for (uint32_t k : o.npm) K.pmap_off.push_back(K.pmap_off.back() + k);
      for (int m = 0; m < 2; m++) {
        K.umaps[m].insert(K.umaps[m].end(), o.um[m].begin(), o.um[m].end()); K.uz[m].insert(K.uz[m].end(), o.uz[m].begin(), o.uz[m].end());
        for (uint32_t k : o.num[m]) K.umap_off[m].push_back(K.umap_off[m].back() + k);
      }
      K.matched += o.matched;
    }
    for (int m = 0; m < 2; m++) { int rc = pm_text(b, m, hb[m], opsptr[m], mapped[m]); if (rc) return rc; }
    lap("harvest + text");
    return GM_OK;
  }

  // The CIGAR -- with extra_sam_fields the edit string too -- of mate m's hits that some mapping names, through k_sw_text: their operations go up packed, the mate's reads
  // of the sub-batch as the caller gave them (the pipeline's own copy of a mate the pair mode turns is reverse-complemented), the sizing launch, the host scan, the
  // writing launch.  Every other hit has an empty slice.
  int pm_text(PairOut& b, int m, size_t hb, const std::vector<const uint8_t*>& opsptr, const std::vector<uint8_t>& mapped) {
    const size_t nh = mapped.size();
    std::vector<GmTextItem> titems; std::vector<uint32_t> towner; std::vector<uint8_t> pack;
    for (size_t i = 0; i < nh; i++) {
      if (!mapped[i]) continue;
      const gm_pass1_hit_t& h = K.hits[m][hb + i]; const gm_sw_full_rec_t& R = K.recs[m][hb + i];
      const long long clen = (long long)ix->contig_off[h.cn + 1] - (long long)ix->contig_off[h.cn];
      if (R.score <= 0 || !opsptr[i] || R.genome_start < 0 || R.read_start < 0 || R.read_start + R.rmapped > len[m] || R.genome_start + R.gmapped > clen) {
        gm_set_error("gm_pair_mappings: mate %d, hit %zu: a mapping whose record lies outside its window", m + 1, hb + i); return GM_E_OVERFLOW; }
      GmTextItem it; memset(&it, 0, sizeof it);
      it.ops_off = pack.size(); it.n_ops = R.n_ops; it.genome_start = R.genome_start; it.read_start = R.read_start; it.tail = len[m] - R.read_start - R.rmapped;
      it.idx = h.read - b.base;
      it.gbase = (long long)ix->contig_off[h.cn] + (h.gen_st ? clen - 1 : 0);
      it.flags = (h.gen_st ? 1 | 4 : 0) | ((ix->rna_ready && ix->contig_rna[h.cn]) ? 2 : 0);
      pack.insert(pack.end(), opsptr[i], opsptr[i] + R.n_ops);
      titems.push_back(it); towner.push_back((uint32_t)i);
    }
    const size_t nt = titems.size();
    const int what = GM_TEXT_CIGAR | (K.want_edit ? GM_TEXT_EDIT : 0);
    std::vector<uint32_t> lens(nt * 2, 0); std::vector<unsigned long long> offs(nt * 2, 0);
    uint64_t cig_total = 0, edit_total = 0;
    const size_t cig0 = K.cigar[m].size(), ed0 = K.edit[m].size();
    GmDevMem mem;
    if (nt) {
      GmTextItem* d_ti = nullptr; uint32_t* d_lens = nullptr; unsigned long long* d_offs = nullptr; uint8_t *d_cig = nullptr, *d_ed = nullptr, *d_pack = nullptr; uint32_t* d_rd = nullptr;
      GM_HIP(mem.up(&d_ti, titems.data(), nt, q)); GM_HIP(mem.get(&d_lens, nt * 2 * sizeof(uint32_t))); GM_HIP(mem.get(&d_offs, nt * 2 * sizeof(unsigned long long)));
      GM_HIP(mem.up(&d_pack, pack.data(), pack.size(), q, 16));
      GM_HIP(mem.up(&d_rd, mates[m] + (size_t)b.base * rwords[m], (size_t)b.n * rwords[m], q));
      int rc = gm_launch_sw_text((int)nt, d_ti, 0, what, 0, d_pack, ix->d_genome, d_rd, rwords[m], 0, nullptr, 'S', d_lens, d_offs, nullptr, nullptr, nullptr, nullptr, q, 1);
      if (rc != GM_OK) { gm_set_error("gm_pair_mappings: the text kernel's launch failed"); return rc; }
      GM_HIP(hipMemcpyAsync(lens.data(), d_lens, nt * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
      GM_HIP(hipStreamSynchronize(q));
      for (size_t k = 0; k < nt; k++) { offs[2 * k] = cig_total; offs[2 * k + 1] = edit_total; cig_total += lens[2 * k]; edit_total += lens[2 * k + 1]; }
      GM_HIP(hipMemcpyAsync(d_offs, offs.data(), nt * 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, q));
      GM_HIP(mem.get(&d_cig, (size_t)cig_total + 16));
      if (K.want_edit) GM_HIP(mem.get(&d_ed, (size_t)edit_total + 16));
      rc = gm_launch_sw_text((int)nt, d_ti, 0, what, 1, d_pack, ix->d_genome, d_rd, rwords[m], 0, nullptr, 'S', d_lens, d_offs, nullptr, nullptr, d_cig, d_ed, q, 1);
      if (rc != GM_OK) { gm_set_error("gm_pair_mappings: the text kernel's launch failed"); return rc; }
      K.cigar[m].resize(cig0 + (size_t)cig_total); K.edit[m].resize(ed0 + (size_t)edit_total);
      if (cig_total) GM_HIP(hipMemcpyAsync(K.cigar[m].data() + cig0, d_cig, (size_t)cig_total, hipMemcpyDeviceToHost, q));
      if (K.want_edit && edit_total) GM_HIP(hipMemcpyAsync(K.edit[m].data() + ed0, d_ed, (size_t)edit_total, hipMemcpyDeviceToHost, q));
      GM_HIP(hipStreamSynchronize(q));
    }
    size_t k = 0; uint64_t c = cig0, e = ed0;
    for (size_t i = 0; i < nh; i++) {
      if (k < nt && towner[k] == (uint32_t)i) { c += lens[2 * k]; e += lens[2 * k + 1]; k++; }
      K.cigar_off[m].push_back(c); if (K.want_edit) K.edit_off[m].push_back(e);
    }
    return GM_OK;
  }
};
}  // namespace

// the refusals of gm_pair_mappings that are its own (everything else is PairCall::init's, the function gm_map_pairs goes through)
static int pair_mappings_check(const gm_session* s, const gm_pair_opts_t* opts) {
  if (s->P.colour_space) { gm_set_error("gm_pair_mappings: a colour-space session: letter space only (colour-space pairs go through gm_map_pairs_cs)"); return GM_E_ARG; }
  if (s->P.output_format) { gm_set_error("gm_pair_mappings: output_format %d: the arrays stand for SAM records (output_format 0)", s->P.output_format); return GM_E_ARG; }
  if (opts && opts->match_mode == 2) { gm_set_error("gm_pair_mappings: match_mode 2 is not covered by this entry (4 or 3)"); return GM_E_ARG; }
  if (s->P.num_tmp_outputs > GM_SEL_MAX) { gm_set_error("gm_pair_mappings: num_tmp_outputs %d is beyond the %d candidate pairs this entry selects from", s->P.num_tmp_outputs, GM_SEL_MAX); return GM_E_RANGE; }
  return GM_OK;
}

extern "C" int gm_pair_mappings(gm_session_t* s, int n_pairs, int len1, const uint32_t* mates1_packed, int len2, const uint32_t* mates2_packed, const gm_pair_opts_t* opts,
                                int want_ops, gm_pair_mappings_t* out, gm_map_stats_t* stats) {
  if (!s || !out) { gm_set_error("gm_pair_mappings: bad arguments (the session and the result struct are required)"); return GM_E_ARG; }
  memset(out, 0, sizeof *out);
  if (stats) memset(stats, 0, sizeof *stats);
  if (n_pairs < 0 || len1 < 1 || len2 < 1 || (n_pairs > 0 && (!mates1_packed || !mates2_packed))) { gm_set_error("gm_pair_mappings: bad arguments"); return GM_E_ARG; }
  if (int rc = pair_mappings_check(s, opts)) return rc;
  GmDevTurn dev_turn(s);
  PairMapRun R; PairMapCall& K = R.K;
  K.want_ops = want_ops != 0; K.want_edit = s->P.extra_sam_fields != 0;
  K.pmap_off.push_back(0);
  for (int m = 0; m < 2; m++) { K.hit_off[m].push_back(0); K.umap_off[m].push_back(0); K.cigar_off[m].push_back(0); if (K.want_edit) K.edit_off[m].push_back(0); }
  int rc = R.init(s, n_pairs, len1, mates1_packed, len2, mates2_packed, nullptr, nullptr, opts, stats, nullptr, nullptr, 33, nullptr, nullptr, nullptr);
  if (rc) { if (stats) memset(stats, 0, sizeof *stats); return rc; }
  for (int k = 0; k < 2; k++) for (int m = 0; m < 2; m++) R.dkm[k][m] = R.dvm[m];
  GmDevMem call_mem;
  // every failure from here on: both streams are drained before the call's memory goes
  auto fail = [&](int code) { (void)hipStreamSynchronize(R.qa); (void)hipStreamSynchronize(R.q); if (stats) memset(stats, 0, sizeof *stats); return code; };
  if (n_pairs > 0) {
    K.thr_n = (len1 + len2) * std::max(1, s->P.match_score) + 1;
    std::vector<int> tab((size_t)K.thr_n);
    for (int v = 0; v < K.thr_n; v++) tab[v] = gm_pair_thresh_int(s->P, v);
    const hipError_t e = call_mem.up(&K.d_thr, tab.data(), tab.size(), gm_sync);
    if (e != hipSuccess) { gm_set_error("gm_pair_mappings: the threshold table: %s", hipGetErrorString(e)); return fail(GM_E_NODEVICE); }
  }
  int cur = 0, front_n = 0; bool have_front = false;
  for (int base = 0; base < n_pairs;) {
    const int B = std::min(R.PS[cur][0]->eff_batch, R.PS[cur][1]->eff_batch);
    const int n = have_front ? front_n : std::min(B, n_pairs - base);
    rc = R.use_pair(cur, B); if (rc) return fail(rc);
    if (!have_front) { rc = R.front(cur, base, n); if (rc) return fail(rc); }
    bool have_next = false; int next_n = 0;
    if (R.overlap && base + n < n_pairs) {
      next_n = std::min(std::min(R.PS[cur ^ 1][0]->eff_batch, R.PS[cur ^ 1][1]->eff_batch), n_pairs - (base + n));
      rc = R.front(cur ^ 1, base + n, next_n); if (rc) return fail(rc);
      have_next = true;
    }
    PairOut b; PairSel t;
    b.base = base; b.n = n; b.resP = &s->pin_res[0]; b.opsP = &s->pin_ops[0]; b.resU = &s->pin_res[2]; b.opsU = &s->pin_ops[2];
    for (int m = 0; m < 2; m++) b.ops_stride[m] = R.S[m]->ops_stride;
    rc = R.finish_front(n);
    if (!rc) rc = R.pass1_select(n, t.n_work);
    if (!rc) rc = R.paired_pass2(b, t);
    if (!rc) rc = R.select_pairs_dev(b, t);
    if (!rc) rc = R.rescue(b, t);
    if (rc == GM_REDO) { rc = R.redo(); if (rc) return fail(rc); have_front = false; continue; }
    if (!rc) rc = R.collect_stats();
    if (!rc) rc = R.harvest(b, t);
    if (rc) return fail(rc);
    base += n;
    if (R.overlap) cur ^= 1;
    have_front = have_next; front_n = next_n;
  }
  gm_pair_mappings_t G; memset(&G, 0, sizeof G);
  G.n_pairs = n_pairs; G.has_edit = K.want_edit ? 1 : 0; G.n_pmaps = K.pmaps.size();
  bool ok = pass2_give(K.pmaps, &G.pmaps) && pass2_give(K.pmap_off, &G.pmap_off);
  for (int m = 0; m < 2 && ok; m++) {
    G.n_hits[m] = K.hits[m].size(); G.n_umaps[m] = K.umaps[m].size(); G.cigar_len[m] = K.cigar[m].size(); G.edit_len[m] = K.edit[m].size(); G.ops_len[m] = K.ops_len[m];
    ok = pass2_give(K.hits[m], &G.hits[m]) && pass2_give(K.hit_off[m], &G.hit_off[m]) && pass2_give(K.kind[m], &G.hit_kind[m]) && pass2_give(K.recs[m], &G.recs[m]) &&
         pass2_give(K.umaps[m], &G.umaps[m]) && pass2_give(K.umap_off[m], &G.umap_off[m]) && pass2_give(K.uz[m], &G.umap_z45[m]) && pass2_give(K.cigar[m], &G.cigar[m]) &&
         pass2_give(K.cigar_off[m], &G.cigar_off[m]) && pass2_give(K.edit[m], &G.edit[m]) && pass2_give(K.edit_off[m], &G.edit_off[m]) && pass2_give(K.ops[m], &G.ops[m]);
  }
  if (!ok) { gm_pair_mappings_free(&G); gm_set_error("gm_pair_mappings: out of memory at %zu + %zu hits", K.hits[0].size(), K.hits[1].size()); return fail(GM_E_NOMEM); }
  if (stats) { stats->reads = 2ull * (uint64_t)n_pairs; stats->reads_matched = K.matched; }
  *out = G;
  return GM_OK;
}

// Debug hook of the tests: k_pair_sel_items and k_sel_pair_pass2 beside the host loop gm_map_pairs runs (pair_pass2), on hand-made candidate lists under the session's
// num_outputs, strata, max_alignments and sw_full_threshold.  wins{0,1}: 9 x int32 a window -- cn, gen_st, genome_start, rmapped, deletions, insertions, score_full,
// score_max, sort_idx -- pair pr's cnt{0,1}[pr] windows one after the other; plist[pr * 64 ..]: its pcnt[pr] candidates (a << 8) | b.  Both answers come back in plist's
// form, n_pairs x 64 words and n_pairs counts each.
extern "C" int gm_debug_pair_select(gm_session_t* s, int pair_mode, int n_pairs, const uint32_t* cnt0, const int32_t* wins0, const uint32_t* cnt1, const int32_t* wins1,
                                    const uint32_t* plist, const uint32_t* pcnt, uint32_t* dev_out, uint32_t* dev_cnt, uint32_t* host_out, uint32_t* host_cnt) {
  if (!s || n_pairs < 1 || !cnt0 || !cnt1 || !plist || !pcnt || !dev_out || !dev_cnt || !host_out || !host_cnt) { gm_set_error("gm_debug_pair_select: bad arguments"); return GM_E_ARG; }
  if (pair_mode < GM_PAIR_OPP_IN || pair_mode > GM_PAIR_COL_BW) { gm_set_error("gm_debug_pair_select: pair_mode %d", pair_mode); return GM_E_ARG; }
  const uint32_t* cnt[2] = {cnt0, cnt1}; const int32_t* wins[2] = {wins0, wins1};
  std::vector<GmFullRes> res[2]; std::vector<int32_t> sf[2]; std::vector<uint32_t> off[2]; std::vector<FHit> fh[2]; int smax_top[2] = {0, 0};
  for (int m = 0; m < 2; m++) {
    off[m].resize(n_pairs); size_t tot = 0;
    for (int pr = 0; pr < n_pairs; pr++) { if (cnt[m][pr] > GM_SEL_MAX) { gm_set_error("gm_debug_pair_select: pair %d has %u windows", pr, cnt[m][pr]); return GM_E_ARG; } off[m][pr] = (uint32_t)tot; tot += cnt[m][pr]; }
    if (tot && !wins[m]) { gm_set_error("gm_debug_pair_select: no windows"); return GM_E_ARG; }
    res[m].resize(tot); sf[m].resize(tot); fh[m].resize(tot);
    for (size_t i = 0; i < tot; i++) {
      const int32_t* w = wins[m] + i * 9; GmFullRes& r = res[m][i]; memset(&r, 0, sizeof r);
      if (w[0] < 0 || (size_t)w[0] + 1 >= s->ix->contig_off.size() || (w[1] & ~1) || w[7] < 1) { gm_set_error("gm_debug_pair_select: mate %d, window %zu: cn %d, gen_st %d, score_max %d", m + 1, i, w[0], w[1], w[7]); return GM_E_ARG; }
      r.cn = (uint32_t)w[0]; r.gen_st = (int16_t)w[1]; r.genome_start = w[2]; r.rmapped = w[3]; r.gmapped = w[3]; r.n_del = w[4]; r.n_ins = w[5]; r.score = w[6]; r.score_max = w[7]; r.sort_idx = w[8];
      sf[m][i] = w[6]; smax_top[m] = std::max(smax_top[m], w[7]);
      FHit& h = fh[m][i]; h.r = &r; h.ops = nullptr; h.score_full = w[6]; h.pass2_key = 0; h.pct_score_full = 0; h.posterior = 0; h.mqv = 255; h.z0 = h.z1 = 0;
    }
  }
  for (int pr = 0; pr < n_pairs; pr++) if (pcnt[pr] > GM_SEL_MAX) { gm_set_error("gm_debug_pair_select: pair %d has %u candidates", pr, pcnt[pr]); return GM_E_ARG; }
  // the host loop
  PairCtx C; C.s = s; gm_pair_opts_default(&C.O); C.O.pair_mode = pair_mode; C.len[0] = C.len[1] = 0; C.rwords[0] = C.rwords[1] = 0; C.total_genome_size = (double)s->ix->total_len;
  std::vector<PPair> v;
  for (int pr = 0; pr < n_pairs; pr++) {
    FHit* H[2] = {fh[0].data() + off[0][pr], fh[1].data() + off[1][pr]};
    for (uint32_t k = 0; k < pcnt[pr]; k++) { const uint32_t p = plist[(size_t)pr * GM_SEL_MAX + k]; if ((p >> 8) >= cnt0[pr] || (p & 0xffu) >= cnt1[pr]) { gm_set_error("gm_debug_pair_select: pair %d, candidate %u names a window it does not have", pr, k); return GM_E_ARG; } }
    pair_pass2(C, H, plist + (size_t)pr * GM_SEL_MAX, (int)pcnt[pr], v);
    host_cnt[pr] = (uint32_t)v.size();
    for (size_t j = 0; j < v.size() && j < GM_SEL_MAX; j++) host_out[(size_t)pr * GM_SEL_MAX + j] = ((uint32_t)v[j].h[0] << 8) | (uint32_t)v[j].h[1];
  }
  // the kernels
  GmDevTurn dev_turn(s);
  GM_HIP(hipSetDevice(s->ix->device));
  const int thr_n = smax_top[0] + smax_top[1] + 1;
  std::vector<int> tab((size_t)thr_n); for (int x = 0; x < thr_n; x++) tab[x] = gm_pair_thresh_int(s->P, x);      // (before mem: the copies from it are drained when mem goes)
  hipStream_t q = s->stream_b; GmDevMem mem;
  int* d_thr = nullptr; uint32_t *d_plist = nullptr, *d_pcnt = nullptr; GmFullRes* d_res[2] = {nullptr, nullptr}; uint32_t *d_off[2] = {nullptr, nullptr}, *d_cnt[2] = {nullptr, nullptr};
  GM_HIP(mem.up(&d_thr, tab.data(), tab.size(), q)); GM_HIP(mem.up(&d_plist, plist, (size_t)n_pairs * GM_SEL_MAX, q)); GM_HIP(mem.up(&d_pcnt, pcnt, (size_t)n_pairs, q));
  for (int m = 0; m < 2; m++) { GM_HIP(mem.up(&d_res[m], res[m].data(), res[m].size(), q)); GM_HIP(mem.up(&d_off[m], off[m].data(), (size_t)n_pairs, q)); GM_HIP(mem.up(&d_cnt[m], cnt[m], (size_t)n_pairs, q)); }
  std::vector<uint32_t> o, c;
  int rc = pair_select_device(q, mem, s->P, n_pairs, d_thr, thr_n, d_plist, d_pcnt, d_res, sf, d_off, d_cnt, o, c);
  (void)hipStreamSynchronize(q);
  if (rc) return rc;
  for (int pr = 0; pr < n_pairs; pr++) {
    dev_cnt[pr] = c[pr];
    for (uint32_t j = 0; j < c[pr] && j < GM_SEL_MAX; j++) dev_out[(size_t)pr * GM_SEL_MAX + j] = o[(size_t)pr * GM_SEL_MAX + j];
  }
  return GM_OK;
}
