// gm_host_seams_ix.inc -- the batch seams on the resident index (gm_*_ix) and gm_index_get_windows, and with them the two bodies they share with the caller-bitfield
// batch forms (sw_full_batch_impl, post_sw_batch_impl: both need ix_window and IxScope) followed by those forms' entries; part of gm_host.hip.
//
// The _ix entries are the twins of the batch entries with (genome, genome_words, g_off) replaced by (ix, cn[], gen_st[], g_off[]): the kernels read ix->d_genome /
// d_genome_cs, so a call uploads the window descriptors, the reads and the per-item scalars -- a fixed number of buffers, copies and launches, none sized by the genome.

// ---- index-resident seams: one window as the reference addresses it ------------------------------------------------------------------------------------------
// Checks (cn, gen_st, g_off, glen) against the index before anything is read through it and turns it into the forward coordinates the kernels take.  whole_contig
// (the gapless seam, the post form's contig bounds): g_off and glen are not looked at, the window is the whole contig of the strand.  Returns the reason of a
// refusal, or null.
static const char* ix_window(const gm_index* ix, int cn, int gen_st, int64_t g_off, int glen, GmWin* w, bool whole_contig = false) {
  if (cn < 0 || cn >= ix->n_contigs) return "cn outside the index's contigs";
  if (gen_st > 1) return "gen_st is neither 0 nor 1";
  const int64_t clen = (int64_t)ix->contig_off[cn + 1] - (int64_t)ix->contig_off[cn];
  if (whole_contig) { g_off = 0; glen = (int)std::min<int64_t>(clen, INT_MAX); }
  if (g_off < 0) return "g_off < 0";
  if (glen < 1) return "glen < 1";
  if (g_off > clen || (int64_t)glen > clen - g_off) return "the window runs past the end of the contig";
  w->cn = cn; w->rc = gen_st ? 1 : 0; w->glen = glen; w->foff = (uint32_t)(gen_st ? clen - g_off - glen : g_off);
  return nullptr;
}
// What every _ix entry does first: the index's device (the caller's current device is set back when the scope ends), its RNA flags (once per index, under
// gm_index_derive_rna's lock), the view the kernels take with the call's is_rna (-1: the index's own)
struct IxScope {
  int prev = -1; GmIndexDev view;
  int enter(const gm_index_t* ix, int is_rna) {
    GM_HIP(hipGetDevice(&prev));
    GM_HIP(hipSetDevice(ix->device));
    { const int rc = gm_index_derive_rna(const_cast<gm_index*>(ix), nullptr); if (rc) return rc; }
    view = ix->dev_view();
    view.genome_is_rna = is_rna < 0 ? ix->genome_is_rna : (is_rna ? 1 : 0);
    return GM_OK;
  }
  ~IxScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

#define GM_IX_NULL(who) do { if (!ix) { gm_set_error(who ": ix is NULL"); return GM_E_ARG; } } while (0)
// the windows of a call without per-item status: the first bad one fails the call
static int ix_windows(const gm_index_t* ix, const char* who, int n, const int* cn, const uint8_t* gen_st, const int64_t* g_off, const int* glen, std::vector<GmWin>& w) {
  w.resize(n);
  const bool whole = !g_off || !glen;      // (the gapless form passes neither: the whole contig of the strand)
  for (int i = 0; i < n; i++)
    if (const char* why = ix_window(ix, cn[i], gen_st[i], whole ? 0 : g_off[i], whole ? 0 : glen[i], &w[i], whole)) { gm_set_error("%s: item %d: %s", who, i, why); return GM_E_ARG; }
  return GM_OK;
}
// an upload of an _ix entry: asynchronous on the null stream, 32 bytes of room behind the array
#define GM_IX_UP(d, h, count) GM_HIP(mem.up(&(d), (h), (size_t)(count), 0, 32))

extern "C" int gm_index_genome_is_rna(const gm_index_t* ix) {
  GM_IX_NULL("gm_index_genome_is_rna");
  IxScope scope; { const int rc = scope.enter(ix, -1); if (rc) return rc; }
  return ix->genome_is_rna ? 1 : 0;
}

extern "C" int gm_index_get_windows(const gm_index_t* ix, int n, const int* cn, const uint8_t* gen_st, const int64_t* g_off, const int* glen,
                                    int colours, uint32_t* words, int stride_words) {
  GM_IX_NULL("gm_index_get_windows");
  if (n <= 0) return GM_OK;
  if (!cn || !gen_st || !g_off || !glen || !words || stride_words < 1) { gm_set_error("gm_index_get_windows: a required argument is missing"); return GM_E_ARG; }
  if (colours && !ix->d_genome_cs) { gm_set_error("gm_index_get_windows: colours need an index built with colour_space = 1"); return GM_E_ARG; }
  std::vector<GmWin> w;
  { const int rc = ix_windows(ix, "gm_index_get_windows", n, cn, gen_st, g_off, glen, w); if (rc) return rc; }
  for (int i = 0; i < n; i++) if ((glen[i] + 7) / 8 > stride_words) { gm_set_error("gm_index_get_windows: item %d: the window does not fit stride_words", i); return GM_E_ARG; }
  IxScope scope; { const int rc = scope.enter(ix, -1); if (rc) return rc; }
  const GmIndexDev& view = scope.view;
  GmDevMem mem; GmWin* dw = nullptr; uint32_t* dout = nullptr;
  GM_IX_UP(dw, w.data(), n);
  GM_HIP(mem.get(&dout, (size_t)n * stride_words * 4)); GM_HIP(hipMemsetAsync(dout, 0, (size_t)n * stride_words * 4, 0));
  { const int rc = gm_launch_get_windows(view, n, dw, colours ? 1 : 0, dout, stride_words, 0); if (rc) { (void)hipDeviceSynchronize(); return rc; } }
  GM_HIP(hipMemcpyAsync(words, dout, (size_t)n * stride_words * 4, hipMemcpyDeviceToHost, 0));
  GM_HIP(hipStreamSynchronize(0));
  return GM_OK;
}

// shared body: colour = gm_sw_full_cs_batch; ix: the _ix forms -- window i is (cn, gen_st, g_off, glen) of the resident genome, nothing of it is uploaded; seam: sw_full_ls /
// sw_full_cs with their one item (declared, with the default arguments, in gm_host_seams.inc)
static int sw_full_batch_impl(bool colour, int n, const uint32_t* genome, uint64_t genome_words, const int64_t* g_off, const int* glen, const uint32_t* reads, int read_words,
                              const int* rlen, const uint8_t* initbp, const struct gm_anchor* anchors, const uint8_t* revcmpl, const int* threshscore, const int* maxscore,
                              const int* xover, int xover_stride, int is_rna, int local, gm_sw_full_rec_t* recs, uint8_t** ops, uint64_t* ops_len,
                              const gm_index_t* ix, const int* cn, const uint8_t* gen_st, bool seam) {
  const char* who = seam ? (colour ? "sw_full_cs" : "sw_full_ls") : ix ? (colour ? "gm_sw_full_cs_batch_ix" : "gm_sw_full_ls_batch_ix") : (colour ? "gm_sw_full_cs_batch" : "gm_sw_full_ls_batch");
  if (ops) *ops = nullptr; if (ops_len) *ops_len = 0;
  if (colour ? !g_sc.init : !g_sf.init) { gm_set_error("%s called before sw_full_%s_setup", who, colour ? "cs" : "ls"); return GM_E_NOTSETUP; }
  if (n <= 0) return GM_OK;
  if ((ix ? (!cn || !gen_st) : !genome) || !g_off || !glen || !reads || !rlen || !threshscore || !recs || !ops || !ops_len || read_words < 1 || (colour && !initbp) ||
      (xover && xover_stride < 1) || (!colour && local && !maxscore)) { gm_set_error("%s: a required argument is missing", who); return GM_E_ARG; }
  double uncounted = 0;
  SeamTimer tm(seam ? &uncounted : colour ? &g_sc.secs : &g_sf.secs);
  IxScope scope;
  if (ix) { const int rc = scope.enter(ix, is_rna); if (rc) return rc; is_rna = scope.view.genome_is_rna; }
  auto win_of = [&](int i, GmWin* w) -> const char* { return ix_window(ix, cn[i], gen_st[i], g_off[i], glen[i], w); };      // (index forms only)
  const int dblen = colour ? g_sc.dblen : g_sf.dblen, qrlen = colour ? g_sc.qrlen : g_sf.qrlen;
  std::vector<GmFullItem> items; items.reserve(n);
  std::vector<int8_t> xrows;
  const int xstride = xover ? ((xover_stride + 15) & ~15) : 0;
  if (xover) xrows.assign((size_t)n * xstride, 0);
  unsigned long long ops_total = 0;
  // LDS is laid out for the longest read and the longest window of a launch, which may belong to different items: an item is admitted when its window fits beside the
  // longest read of the call that is otherwise in order (so whatever the launch classes turn out to be, each fits)
  auto in_order = [&](int i) { return glen[i] >= 1 && rlen[i] >= 1 && g_off[i] >= 0 && (ix ? [&] { GmWin w; return !win_of(i, &w); }() : (uint64_t)g_off[i] + (uint64_t)glen[i] <= genome_words * 8) &&
                                      ((uint64_t)rlen[i] + 7) / 8 <= (uint64_t)read_words && glen[i] <= dblen && rlen[i] <= qrlen; };
  int call_max_r = 1;
  for (int i = 0; i < n; i++) if (in_order(i)) call_max_r = std::max(call_max_r, rlen[i]);
  for (int i = 0; i < n; i++) {
    gm_sw_full_rec_t& R = recs[i]; memset(&R, 0, sizeof R);
    auto refuse = [&](int code, const char* why) { R.status = code; gm_set_error("%s: item %d refused: %s", who, i, why); };
    GmWin win;                                                                        // this item's window on the index
    if (ix) { if (const char* why = win_of(i, &win)) { refuse(GM_E_ARG, why); continue; } }
    if (glen[i] < 1 || rlen[i] < 1 || g_off[i] < 0 || (!ix && (uint64_t)g_off[i] + (uint64_t)glen[i] > genome_words * 8) || ((uint64_t)rlen[i] + 7) / 8 > (uint64_t)read_words) {
      refuse(GM_E_ARG, "window or read outside the bitfields"); continue; }
    if (glen[i] > dblen || rlen[i] > qrlen) { refuse(GM_E_ARG, "window / read longer than the setup sizes"); continue; }
    const bool has_anchor = anchors && (seam || anchors[i].length > 0);
    if (colour) {
      if (!has_anchor && g_sc.p[7] >= 0) { refuse(GM_E_ARG, "colour space needs one anchor box (gmapper's call, ref: mapping.c:375-379)"); continue; }      // (anchor_width -1: the threshold band, box or none)
      if (initbp[i] > 3) { refuse(GM_E_ARG, "initbp outside 0..3"); continue; }
      if (gm_sw_full_cs_batch_lds(glen[i], call_max_r) > GM_SWF_LDS_LIMIT) { refuse(GM_E_ARG, "the window does not fit LDS (48 bytes a column) beside the call's longest read"); continue; }
      if (xover) {
        if (xover_stride < rlen[i]) { refuse(GM_E_ARG, "xover_stride shorter than the read"); continue; }
        bool ok = true;
        for (int k = 0; k < rlen[i]; k++) { const int v = xover[(size_t)i * xover_stride + k]; if (v < -128 || v > 127) { ok = false; break; } xrows[(size_t)i * xstride + k] = (int8_t)v; }
        if (!ok) { refuse(GM_E_RANGE, "a per-position crossover score outside [-128, 127] (the device keeps them in 8 bits)"); continue; }
      }
    } else if (gm_sw_full_batch_lds(glen[i], call_max_r) > GM_SWF_LDS_LIMIT) { refuse(GM_E_ARG, "the window does not fit LDS beside the call's longest read"); continue; }
    GmFullItem it; memset(&it, 0, sizeof it);
    it.goff = g_off[i]; it.glen = glen[i]; it.rlen = rlen[i];
    if (has_anchor) { it.ax = anchors[i].x; it.ay = anchors[i].y; it.alen = anchors[i].length; it.awidth = anchors[i].width; } else { it.alen = it.awidth = 1; }
    it.thresh = threshscore[i]; it.maxscore = maxscore ? maxscore[i] : 0;
    it.flags = (has_anchor ? 1 : 0) | ((revcmpl && revcmpl[i]) ? 2 : 0);
    if (ix) {
      it.goff = (long long)ix->contig_off[win.cn] + (long long)win.foff;
      it.flags |= (win.rc ? 4 : 0) | ((ix->rna_ready && ix->contig_rna[win.cn]) ? 8 : 0);
    }
    it.initbp = colour ? ((int)initbp[i] | (is_rna ? GM_SEAM_RNA : 0)) : 0;
    it.ops_cap = glen[i] + rlen[i] + 8; it.ops_off = ops_total; it.idx = i;           // exclusive scan of the caps, in item order
    ops_total += (unsigned long long)it.ops_cap;
    items.push_back(it);
  }
  if (items.empty()) return GM_OK;
  std::vector<SwfLaunch> launches; size_t pool = 0;
  swf_plan(items, colour ? 12 : 1, launches, &pool);
  GmDevMem mem;
  uint32_t *dg = nullptr, *dr = nullptr; GmFullItem* di = nullptr; GmFullOut* dout = nullptr; uint8_t *dops = nullptr, *dback = nullptr; int8_t* dx = nullptr;
  if (ix) dg = ix->d_genome; else GM_HIP(mem.get(&dg, (genome_words + 8) * 4));
  GM_HIP(mem.get(&dr, (size_t)n * read_words * 4 + 32)); GM_HIP(mem.get(&di, items.size() * sizeof(GmFullItem)));
  GM_HIP(mem.get(&dout, (size_t)n * sizeof(GmFullOut))); GM_HIP(mem.get(&dops, (size_t)ops_total + 16)); GM_HIP(mem.get(&dback, pool));
  if (xover) GM_HIP(mem.get(&dx, xrows.size() + 16));
  if (!ix) {
    GM_HIP(hipMemsetAsync(dg + genome_words, 0, 8 * 4, 0));
    GM_HIP(hipMemcpyAsync(dg, genome, genome_words * 4, hipMemcpyHostToDevice, 0));
  }
  GM_HIP(hipMemcpyAsync(dr, reads, (size_t)n * read_words * 4, hipMemcpyHostToDevice, 0));
  GM_HIP(hipMemcpyAsync(di, items.data(), items.size() * sizeof(GmFullItem), hipMemcpyHostToDevice, 0));
  if (xover) GM_HIP(hipMemcpyAsync(dx, xrows.data(), xrows.size(), hipMemcpyHostToDevice, 0));
  for (const SwfLaunch& L : launches) {
    const int rc = colour ? gm_launch_sw_full_cs_batch(g_sc.p, L.first, L.count, L.grid, di, dg, dr, read_words, L.max_g, L.max_r, dx, xstride, (uint32_t*)dback, L.stride / 4, dout,
                                                       dops, local ? 1 : 0, 0, ix ? 1 : 0)
                          : gm_launch_sw_full_batch(g_sf.sc, L.first, L.count, L.grid, di, dg, dr, read_words, L.max_g, L.max_r, dback, L.stride, dout, dops, local ? 1 : 0, 0, ix ? 1 : 0);
    if (rc != GM_OK) { (void)hipDeviceSynchronize(); return rc; }
  }
  std::vector<GmFullOut> out(n); std::vector<uint8_t> hops((size_t)ops_total);
  GM_HIP(hipMemcpyAsync(hops.data(), dops, (size_t)ops_total, hipMemcpyDeviceToHost, 0));
  GM_HIP(hipMemcpyAsync(out.data(), dout, (size_t)n * sizeof(GmFullOut), hipMemcpyDeviceToHost, 0));
  GM_HIP(hipStreamSynchronize(0));
  if (!seam) for (const GmFullItem& it : items) {                                    // (the items that ran: a refused item, or a call that failed before here, scored nothing)
    if (colour) { g_sc.invocs++; g_sc.cells += 4ull * (uint64_t)it.glen * (uint64_t)it.rlen; }
    else { g_sf.invocs++; g_sf.cells += (uint64_t)it.glen * (uint64_t)it.rlen; }
  }
  // the used lengths, compacted in item order
  std::sort(items.begin(), items.end(), [](const GmFullItem& a, const GmFullItem& b) { return a.idx < b.idx; });
  uint64_t used = 0;
  for (const GmFullItem& it : items) { const int* v = out[it.idx].v; if (v[0] > 0) used += (uint64_t)std::min(v[10], it.ops_cap); }
  uint8_t* obuf = (uint8_t*)malloc(used ? used : 1);
  if (!obuf) { gm_set_error("%s: out of memory", who); return GM_E_NOMEM; }
  uint64_t at = 0;
  for (const GmFullItem& it : items) {
    const int* v = out[it.idx].v; gm_sw_full_rec_t& R = recs[it.idx];
    R.score = v[0];
    if (v[0] > 0) {
      R.read_start = v[1]; R.rmapped = v[2]; R.genome_start = g_off[it.idx] + v[3]; R.gmapped = v[4];      // (g_off: the caller's -- on the index, counted on the strand's contig)
      R.matches = v[5]; R.mismatches = v[6]; R.insertions = v[7]; R.deletions = v[8]; R.crossovers = v[9];
      R.n_ops = (uint32_t)std::min(v[10], it.ops_cap); R.ops_off = at;
      memcpy(obuf + at, hops.data() + it.ops_off, R.n_ops); at += R.n_ops;
    } else if (!colour) { R.score = v[0] < 0 ? 0 : v[0]; R.rmapped = 1; R.gmapped = 1; R.genome_start = g_off[it.idx]; R.ops_off = at; }      // as sw_full_ls leaves a window without alignment
    else { R.score = 0; R.ops_off = at; }
  }
  *ops = obuf; *ops_len = used;
  return GM_OK;
}
extern "C" int gm_sw_full_ls_batch(int n, const uint32_t* genome, uint64_t genome_words, const int64_t* g_off, const int* glen, const uint32_t* reads, int read_words,
                                   const int* rlen, const struct gm_anchor* anchors, const uint8_t* revcmpl, const int* threshscore, const int* maxscore,
                                   int local_alignment, gm_sw_full_rec_t* recs, uint8_t** ops, uint64_t* ops_len) {
  return sw_full_batch_impl(false, n, genome, genome_words, g_off, glen, reads, read_words, rlen, nullptr, anchors, revcmpl, threshscore, maxscore, nullptr, 0, 0,
                            local_alignment, recs, ops, ops_len);
}
extern "C" int gm_sw_full_cs_batch(int n, const uint32_t* genome_ls, uint64_t genome_words, const int64_t* g_off, const int* glen, const uint32_t* reads, int read_words,
                                   const int* rlen, const uint8_t* initbp, const struct gm_anchor* anchors, const uint8_t* revcmpl, const int* threshscore,
                                   const int* crossover_scores, int xover_stride, int is_rna, int local_alignment, gm_sw_full_rec_t* recs, uint8_t** ops, uint64_t* ops_len) {
  return sw_full_batch_impl(true, n, genome_ls, genome_words, g_off, glen, reads, read_words, rlen, initbp, anchors, revcmpl, threshscore, nullptr, crossover_scores,
                            xover_stride, is_rna, local_alignment, recs, ops, ops_len);
}

// shared body; ix: gm_post_sw_batch_ix -- record i lies on strand gen_st[i] of contig cn[i] of the resident genome (genome_start counted on that strand's contig)
static int post_sw_batch_impl(int n, const gm_sw_full_rec_t* recs, const uint8_t* ops, uint64_t ops_len, const uint32_t* genome_ls, uint64_t genome_words,
                              const uint32_t* reads, int read_words, const int* rlen, const uint8_t* initbp, const char* const* quals, int is_rna,
                              gm_post_rec_t* post, char** qralign_out, char** quals_out, uint64_t* quals_len,
                              const gm_index_t* ix = nullptr, const int* cn = nullptr, const uint8_t* gen_st = nullptr) {
  const char* who = ix ? "gm_post_sw_batch_ix" : "gm_post_sw_batch";
  if (!g_ps.init) { gm_set_error("%s called before post_sw_setup", who); return GM_E_NOTSETUP; }
  if (n <= 0) return GM_OK;
  if (!recs || (!ops && ops_len) || (ix ? (!cn || !gen_st) : !genome_ls) || !reads || read_words < 1 || !rlen || !initbp || !post || !qralign_out || !quals_out || !quals_len) {
    gm_set_error("%s: a required argument is missing", who); return GM_E_ARG; }
  *qralign_out = *quals_out = nullptr; *quals_len = 0;
  SeamTimer tm(&g_ps.secs);
  IxScope scope;
  if (ix) { const int rc = scope.enter(ix, is_rna); if (rc) return rc; is_rna = scope.view.genome_is_rna; }
  const bool use_qvs = g_ps.use_read_qvs; const int qoff = g_ps.K.qoff, qv_stride = read_words * 8;
  // the longest alignment 64 thread slots can hold inside the budget
  const uint64_t slot_max = GM_POST_BUDGET / (64 * GM_POST_COL_BYTES);
  std::vector<GmPostItem> items; items.reserve(n);
  std::vector<uint8_t> qv; if (use_qvs) qv.assign((size_t)n * qv_stride, 0);
  uint64_t quals_total = 0; g_post_plan.n = 0;
  for (int i = 0; i < n; i++) {
    gm_post_rec_t& P = post[i]; memset(&P, 0, sizeof P);
    const gm_sw_full_rec_t& R = recs[i];
    if (R.status < 0) { P.status = R.status; continue; }
    if (R.score <= 0) continue;                                           // no alignment: status 0, posterior 0, no base qualities
    auto refuse = [&](const char* why) { P.status = GM_E_ARG; gm_set_error("%s: item %d refused: %s", who, i, why); };
    uint64_t genome_len = genome_words * 8; GmWin win;
    if (ix) {
      if (const char* why = ix_window(ix, cn[i], gen_st[i], 0, 0, &win, true)) { refuse(why); continue; }
      genome_len = (uint64_t)ix->contig_off[win.cn + 1] - (uint64_t)ix->contig_off[win.cn];
    }
    if (rlen[i] < 1 || ((uint64_t)rlen[i] + 7) / 8 > (uint64_t)read_words || initbp[i] > 3) { refuse("read outside the bitfield, or initbp outside 0..3"); continue; }
    uint64_t len = 0;
    if (const char* why = swf_rec_check(true, &R, ops, ops_len, genome_len, rlen[i], &len)) { refuse(why); continue; }
    if ((int64_t)R.n_ops > (int64_t)g_ps.max_len) { refuse("an alignment longer than post_sw_setup's max_len"); continue; }
    if (len > slot_max) { refuse("an alignment too long for the column scratch of one wave"); continue; }
    if (use_qvs) {
      const size_t need = (size_t)qoff + (size_t)rlen[i];
      if (!quals || !quals[i] || strnlen(quals[i], need) < need) { refuse("a QV string is missing or shorter than the read"); continue; }
      for (int j = 0; j < rlen[i]; j++)                                   // what the error-rate formula distinguishes (qv <= 0, qv >= 250, ref: util.h:285-293)
        qv[(size_t)i * qv_stride + j] = (uint8_t)std::min(250, std::max(0, (int)quals[i][qoff + j] - g_ps.qual_delta));
    }
    GmPostItem it; memset(&it, 0, sizeof it);
    it.ops_off = R.ops_off; it.n_ops = R.n_ops; it.genome_start = R.genome_start; it.read_start = R.read_start; it.rlen = rlen[i]; it.len = (int)len;
    it.initbp = initbp[i]; it.idx = i; it.qual_off = quals_total;
    if (ix) {
      it.gbase = (long long)ix->contig_off[win.cn] + (win.rc ? (long long)genome_len - 1 : 0);
      it.flags = (win.rc ? 1 : 0) | ((ix->rna_ready && ix->contig_rna[win.cn]) ? 2 : 0);
    }
    P.qual_off = quals_total; P.qual_len = (uint32_t)len; quals_total += len;
    items.push_back(it);
  }
  GmDevMem results;      // (the two result buffers only: the device buffers have a holder and a scope of their own below)
  char* qa = results.host(ops_len ? ops_len : 1, true); char* qo = results.host(quals_total ? quals_total : 1);
  if (!qa || !qo) { gm_set_error("%s: out of memory", who); return GM_E_NOMEM; }
  std::vector<GmPostRes> res(items.size());
  std::vector<PostLaunch> launches;
  // an item without a read position never reaches the device: the host routine's early return answers it
  std::vector<GmPostItem> dev; dev.reserve(items.size());
  for (const GmPostItem& it : items) if (it.len > 0) dev.push_back(it);
  post_plan(dev, launches);
  if (!dev.empty()) {
    if (gm_device_count() < 1) { gm_set_error("no HIP device"); return GM_E_NODEVICE; }
    GmCsPostDev K; const CsPostConsts& c = g_ps.K;
    K.let_m = c.let_m; K.let_x = c.let_x; K.col_m[0] = c.col_m[0]; K.col_m[1] = c.col_m[1]; K.col_x[0] = c.col_x[0]; K.col_x[1] = c.col_x[1];
    K.pr_del_open = c.pr_del_open; K.pr_del_extend = c.pr_del_extend; K.pr_ins_open = c.pr_ins_open; K.pr_ins_extend = c.pr_ins_extend; K.qv = nullptr; K.qtab = nullptr; K.bq = nullptr;
    size_t fw_bytes = 0, info_bytes = 0;
    for (const PostLaunch& L : launches) { fw_bytes = std::max(fw_bytes, (size_t)L.threads * L.max_len * 17 * 8); info_bytes = std::max(info_bytes, (size_t)L.threads * L.max_len * 4); }
    GmDevMem mem;
    uint32_t *dg = nullptr, *dr = nullptr, *dinfo = nullptr; GmPostItem* di = nullptr; GmPostRes* dres = nullptr; uint8_t *dops = nullptr, *dqa = nullptr, *dqo = nullptr, *dqv = nullptr;
    double *dfw = nullptr, *dqt = nullptr;
    if (ix) dg = ix->d_genome; else GM_HIP(mem.get(&dg, (genome_words + 8) * 4));
    GM_HIP(mem.get(&dr, (size_t)n * read_words * 4 + 32)); GM_HIP(mem.get(&di, dev.size() * sizeof(GmPostItem)));
    GM_HIP(mem.get(&dres, dev.size() * sizeof(GmPostRes))); GM_HIP(mem.get(&dops, (size_t)ops_len + 16)); GM_HIP(mem.get(&dqa, (size_t)ops_len + 16));
    GM_HIP(mem.get(&dqo, (size_t)quals_total + 16)); GM_HIP(mem.get(&dfw, fw_bytes)); GM_HIP(mem.get(&dinfo, info_bytes));
    if (!ix) GM_HIP(hipMemcpyAsync(dg, genome_ls, genome_words * 4, hipMemcpyHostToDevice, 0));
    GM_HIP(hipMemcpyAsync(dr, reads, (size_t)n * read_words * 4, hipMemcpyHostToDevice, 0));
    GM_HIP(hipMemcpyAsync(di, dev.data(), dev.size() * sizeof(GmPostItem), hipMemcpyHostToDevice, 0));
    GM_HIP(hipMemcpyAsync(dops, ops, (size_t)ops_len, hipMemcpyHostToDevice, 0));
    GM_HIP(hipMemsetAsync(dqa, 0, (size_t)ops_len + 16, 0));                                   // (the slices of refused items and of those the host answers)
    GM_HIP(hipMemsetAsync(dqo, 0, (size_t)quals_total + 16, 0));
    std::vector<double> qt;
    if (use_qvs) {
      // the per-colour error rates of every QV the formula distinguishes, from the host's libm: the very doubles cs_post_sw computes (ref: sw-post.c:486-491)
      qt = cs_qv_table(c.sanger);
      GM_HIP(mem.up(&dqv, qv.data(), qv.size(), 0, 16)); GM_HIP(mem.up(&dqt, qt.data(), qt.size(), 0));
      K.qv = dqv; K.qtab = dqt;
    }
    for (const PostLaunch& L : launches) {
      const int rc = gm_launch_post_sw_batch(K, L.first, L.count, L.threads, di, dops, dg, dr, read_words, qv_stride, is_rna ? 1 : 0, dres, dqa, dqo, dfw, dinfo, 0, ix ? 1 : 0);
      if (rc != GM_OK) { (void)hipDeviceSynchronize(); gm_set_error("%s: the kernel launch failed", who); return rc; }
    }
    res.resize(dev.size());
    GM_HIP(hipMemcpyAsync(res.data(), dres, dev.size() * sizeof(GmPostRes), hipMemcpyDeviceToHost, 0));
    if (ops_len) GM_HIP(hipMemcpyAsync(qa, dqa, (size_t)ops_len, hipMemcpyDeviceToHost, 0));
    if (quals_total) GM_HIP(hipMemcpyAsync(qo, dqo, (size_t)quals_total, hipMemcpyDeviceToHost, 0));
    GM_HIP(hipStreamSynchronize(0));
    g_post_plan.n = (int)launches.size(); for (size_t k = 0; k < launches.size() && k < 3; k++) g_post_plan.l[k] = launches[k];
  }
  // the device's answers; then the items the host routine takes: flagged by the kernel, or without a read position
  std::vector<uint8_t> by_dev((size_t)n, 0);
  for (size_t k = 0; k < dev.size(); k++) {
    if (res[k].valid != 1) continue;
    gm_post_rec_t& P = post[dev[k].idx]; by_dev[dev[k].idx] = 1;
    P.posterior = res[k].posterior; P.matches = res[k].cs_match; P.mismatches = res[k].cs_mismatch; P.crossovers = res[k].cs_xover;
  }
  // on the index, the host routine's items get the genome stretch of their alignment in one more call (gm_index_get_windows), each as a bitfield of its own
  std::vector<uint32_t> hw; std::vector<int> hslot((size_t)n, -1); int hstride = 0;
  if (ix) {
    std::vector<int> hcn, hlen; std::vector<uint8_t> hst; std::vector<int64_t> hoff;
    for (const GmPostItem& it : items) {
      if (by_dev[it.idx]) continue;
      int adv_g = 0; for (uint32_t k = 0; k < it.n_ops; k++) { const int type = ops[it.ops_off + k] & 0x0f; if (!(type >= 2 && type <= 5)) adv_g++; }
      if (adv_g < 1) continue;
      hslot[it.idx] = (int)hcn.size(); hcn.push_back(cn[it.idx]); hst.push_back(gen_st[it.idx]); hoff.push_back(it.genome_start); hlen.push_back(adv_g);
      hstride = std::max(hstride, (adv_g + 7) / 8);
    }
    if (!hcn.empty()) {
      hw.assign((size_t)hcn.size() * hstride, 0);
      const int rc = gm_index_get_windows(ix, (int)hcn.size(), hcn.data(), hst.data(), hoff.data(), hlen.data(), 0, hw.data(), hstride);
      if (rc != GM_OK) return rc;
    }
  }
  for (const GmPostItem& it : items) {
    g_ps.invocs++; g_ps.cells += 16 * (uint64_t)it.len;                                        // as one post_sw call counts (above)
    if (by_dev[it.idx]) continue;
    const int i = it.idx; gm_post_rec_t& P = post[i];
    char *db = nullptr, *qr = nullptr;
    gm_sw_full_rec_t rloc = recs[i]; const uint32_t* hg = genome_ls; uint64_t hg_len = genome_words * 8;
    static const uint32_t no_genome[1] = {0};
    if (ix) {                                                                                  // the record against its own stretch: genome_start 0
      rloc.genome_start = 0;
      if (hslot[i] >= 0) { hg = hw.data() + (size_t)hslot[i] * hstride; hg_len = (uint64_t)hstride * 8; } else { hg = no_genome; hg_len = 0; }
    }
    const int rc = gm_sw_full_batch_strings(1, &rloc, ops, ops_len, hg, hg_len, reads + (size_t)i * read_words, rlen[i], initbp[i], is_rna, &db, &qr);
    if (rc != GM_OK || !db || !qr) { free(db); free(qr); P.status = rc != GM_OK ? rc : GM_E_ARG; P.qual_len = 0; continue; }
    FHit h; h.db = db; h.qr = qr; free(db); free(qr);
    cs_post_sw(g_ps.K, reads + (size_t)i * read_words, initbp[i], rloc.read_start, h, use_qvs ? quals[i] : nullptr, g_ps.qual_delta, true);
    P.posterior = h.posterior; P.matches = h.cs_match; P.mismatches = h.cs_mismatch; P.crossovers = h.cs_xover; P.by_host = 1;
    memcpy(qa + it.ops_off, h.qr.data(), std::min<size_t>(h.qr.size(), it.n_ops));
    memcpy(qo + it.qual_off, h.qual.data(), std::min<size_t>(h.qual.size(), (size_t)it.len));
  }
  *qralign_out = results.give(qa); *quals_out = results.give(qo); *quals_len = quals_total;
  return GM_OK;
}
extern "C" int gm_post_sw_batch(int n, const gm_sw_full_rec_t* recs, const uint8_t* ops, uint64_t ops_len, const uint32_t* genome_ls, uint64_t genome_words,
                                const uint32_t* reads, int read_words, const int* rlen, const uint8_t* initbp, const char* const* quals, int is_rna,
                                gm_post_rec_t* post, char** qralign_out, char** quals_out, uint64_t* quals_len) {
  return post_sw_batch_impl(n, recs, ops, ops_len, genome_ls, genome_words, reads, read_words, rlen, initbp, quals, is_rna, post, qralign_out, quals_out, quals_len);
}

static int sw_vector_batch_ix_impl(const char* who, const gm_index_t* ix, int n, const int* cn, const uint8_t* gen_st, const int64_t* g_off, const int* glen,
                                   const uint32_t* reads, int read_words, const int* rlen, const int* initbp, int is_rna, int* scores, int early_thr, uint8_t* stopped) {
  if (!g_sv.init) { gm_set_error("%s called before sw_vector_setup", who); return GM_E_NOTSETUP; }
  if (n <= 0) return GM_OK;
  const bool cs = g_sv.colours;
  if (!cn || !gen_st || !g_off || !glen || !reads || !rlen || !scores || read_words < 1 || (cs && !initbp)) { gm_set_error("%s: a required argument is missing", who); return GM_E_ARG; }
  if (cs && !ix->d_genome_cs) { gm_set_error("%s: sw_vector_setup chose colour space, the index was built without colour_space", who); return GM_E_ARG; }
  if (cs && stopped) { gm_set_error("%s: the bounded form is letter space only", who); return GM_E_ARG; }
  std::vector<GmWin> w;
  { const int rc = ix_windows(ix, who, n, cn, gen_st, g_off, glen, w); if (rc) return rc; }
  int max_g = 0, max_r = 0;
  for (int i = 0; i < n; i++) {
    if (rlen[i] < 1 || (rlen[i] + 7) / 8 > read_words || (cs && (initbp[i] < 0 || initbp[i] > 3))) { gm_set_error("%s: item %d: read outside its bitfield, or initbp outside 0..3", who, i); return GM_E_ARG; }
    if (glen[i] > g_sv.dblen || rlen[i] > g_sv.qrlen) { gm_set_error("%s: item %d: window / read longer than the sw_vector_setup sizes", who, i); return GM_E_ARG; }
    max_g = std::max(max_g, glen[i]); max_r = std::max(max_r, rlen[i]);
  }
  const auto t0 = std::chrono::steady_clock::now();
  IxScope scope; { const int rc = scope.enter(ix, is_rna); if (rc) return rc; }
  const GmIndexDev& view = scope.view;
  GmDevMem mem; GmWin* dw = nullptr; uint32_t* dr = nullptr; int *drl = nullptr, *dib = nullptr, *ds = nullptr; uint8_t* dst = nullptr;
  GM_IX_UP(dw, w.data(), n); GM_IX_UP(dr, reads, (size_t)n * read_words); GM_IX_UP(drl, rlen, n);
  if (cs) GM_IX_UP(dib, initbp, n);
  GM_HIP(mem.get(&ds, (size_t)n * 4));
  if (stopped) GM_HIP(mem.get(&dst, (size_t)n));
  const GmScoreDev& sv = g_sv.sc;      // (the early stop's conditions: see sw_vector_batch_impl)
  if (!(sv.match > 0 && sv.mismatch <= sv.match && sv.a_go >= 0 && sv.a_ge >= 0 && sv.b_go >= 0 && sv.b_ge >= 0 && sv.match * (2 * 128 + 2) < 32000)) early_thr = 0;
  const int rc = gm_launch_sw_vector_batch_ix(view, g_sv.sc, n, dw, dr, read_words, drl, dib, max_g, max_r, ds, 0, early_thr, dst);
  if (rc != GM_OK) { (void)hipDeviceSynchronize(); return rc; }
  GM_HIP(hipMemcpyAsync(scores, ds, (size_t)n * 4, hipMemcpyDeviceToHost, 0));
  if (stopped) GM_HIP(hipMemcpyAsync(stopped, dst, (size_t)n, hipMemcpyDeviceToHost, 0));
  GM_HIP(hipStreamSynchronize(0));
  for (int i = 0; i < n; i++) { g_sv.invocs++; g_sv.cells += (uint64_t)glen[i] * rlen[i]; }
  g_sv.secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return GM_OK;
}
extern "C" int gm_sw_vector_batch_ix(const gm_index_t* ix, int n, const int* cn, const uint8_t* gen_st, const int64_t* g_off, const int* glen,
                                     const uint32_t* reads, int read_words, const int* rlen, const int* initbp, int is_rna, int* scores) {
  GM_IX_NULL("gm_sw_vector_batch_ix");
  return sw_vector_batch_ix_impl("gm_sw_vector_batch_ix", ix, n, cn, gen_st, g_off, glen, reads, read_words, rlen, initbp, is_rna, scores, 0, nullptr);
}
extern "C" int gm_sw_vector_batch_bounded_ix(const gm_index_t* ix, int n, const int* cn, const uint8_t* gen_st, const int64_t* g_off, const int* glen,
                                             const uint32_t* reads, int read_words, const int* rlen, int threshold, int* scores, uint8_t* stopped) {
  GM_IX_NULL("gm_sw_vector_batch_bounded_ix");
  if (threshold <= 0 || !stopped) { gm_set_error("gm_sw_vector_batch_bounded_ix: threshold > 0 and a stopped[] array are required"); return GM_E_ARG; }
  return sw_vector_batch_ix_impl("gm_sw_vector_batch_bounded_ix", ix, n, cn, gen_st, g_off, glen, reads, read_words, rlen, nullptr, 0, scores, threshold, stopped);
}

extern "C" int gm_sw_gapless_batch_ix(const gm_index_t* ix, int n, const int* cn, const uint8_t* gen_st, int colour_space,
                                      const uint32_t* reads, int read_words, const int* rlen, const int* g_idx, const int* r_idx, const int* initbp, int is_rna, int* scores) {
  GM_IX_NULL("gm_sw_gapless_batch_ix");
  if (!g_sg.init) { gm_set_error("gm_sw_gapless_batch_ix called before sw_gapless_setup"); return GM_E_NOTSETUP; }
  if (n <= 0) return GM_OK;
  if (!cn || !gen_st || !reads || !rlen || !g_idx || !r_idx || !scores || read_words < 1 || (colour_space && !initbp)) {
    gm_set_error("gm_sw_gapless_batch_ix: a required argument is missing"); return GM_E_ARG; }
  if (colour_space && !ix->d_genome_cs) { gm_set_error("gm_sw_gapless_batch_ix: colour_space = 1 needs an index built with colour_space = 1"); return GM_E_ARG; }
  std::vector<GmWin> w;
  { const int rc = ix_windows(ix, "gm_sw_gapless_batch_ix", n, cn, gen_st, nullptr, nullptr, w); if (rc) return rc; }
  int max_r = 0;
  for (int i = 0; i < n; i++) {
    const int64_t clen = (int64_t)ix->contig_off[cn[i] + 1] - (int64_t)ix->contig_off[cn[i]];
    if (rlen[i] < 1 || g_idx[i] < 0 || r_idx[i] < 0 || (int64_t)g_idx[i] >= clen || r_idx[i] >= rlen[i] || (rlen[i] + 7) / 8 > read_words ||
        (colour_space && (initbp[i] < 0 || initbp[i] > 3))) { gm_set_error("gm_sw_gapless_batch_ix: item %d out of range", i); return GM_E_ARG; }
    max_r = std::max(max_r, rlen[i]);
  }
  const auto t0 = std::chrono::steady_clock::now();
  IxScope scope; { const int rc = scope.enter(ix, is_rna); if (rc) return rc; }
  const GmIndexDev& view = scope.view;
  GmDevMem mem; GmWin* dw = nullptr; uint32_t* dr = nullptr; int *drl = nullptr, *dgi = nullptr, *dri = nullptr, *dib = nullptr, *ds = nullptr;
  GM_IX_UP(dw, w.data(), n); GM_IX_UP(dr, reads, (size_t)n * read_words); GM_IX_UP(drl, rlen, n); GM_IX_UP(dgi, g_idx, n); GM_IX_UP(dri, r_idx, n);
  if (colour_space) GM_IX_UP(dib, initbp, n);
  GM_HIP(mem.get(&ds, (size_t)n * 4));
  const int rc = gm_launch_sw_gapless_batch_ix(view, n, g_sg.match, g_sg.mismatch, dw, colour_space ? 1 : 0, dr, read_words, drl, dgi, dri, dib, max_r, ds, 0);
  if (rc != GM_OK) { (void)hipDeviceSynchronize(); return rc; }
  GM_HIP(hipMemcpyAsync(scores, ds, (size_t)n * 4, hipMemcpyDeviceToHost, 0));
  GM_HIP(hipStreamSynchronize(0));
  for (int i = 0; i < n; i++) { g_sg.invocs++; g_sg.cells += (uint64_t)rlen[i]; }
  g_sg.ticks += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  return GM_OK;
}

extern "C" int gm_sw_full_ls_batch_ix(const gm_index_t* ix, int n, const int* cn, const uint8_t* gen_st, const int64_t* g_off, const int* glen,
                                      const uint32_t* reads, int read_words, const int* rlen, const struct gm_anchor* anchors, const uint8_t* revcmpl,
                                      const int* threshscore, const int* maxscore, int local_alignment, gm_sw_full_rec_t* recs, uint8_t** ops, uint64_t* ops_len) {
  GM_IX_NULL("gm_sw_full_ls_batch_ix");
  return sw_full_batch_impl(false, n, nullptr, 0, g_off, glen, reads, read_words, rlen, nullptr, anchors, revcmpl, threshscore, maxscore, nullptr, 0, 0,
                            local_alignment, recs, ops, ops_len, ix, cn, gen_st);
}
extern "C" int gm_sw_full_cs_batch_ix(const gm_index_t* ix, int n, const int* cn, const uint8_t* gen_st, const int64_t* g_off, const int* glen,
                                      const uint32_t* reads, int read_words, const int* rlen, const uint8_t* initbp, const struct gm_anchor* anchors, const uint8_t* revcmpl,
                                      const int* threshscore, const int* crossover_scores, int xover_stride, int is_rna, int local_alignment,
                                      gm_sw_full_rec_t* recs, uint8_t** ops, uint64_t* ops_len) {
  GM_IX_NULL("gm_sw_full_cs_batch_ix");
  return sw_full_batch_impl(true, n, nullptr, 0, g_off, glen, reads, read_words, rlen, initbp, anchors, revcmpl, threshscore, nullptr, crossover_scores,
                            xover_stride, is_rna, local_alignment, recs, ops, ops_len, ix, cn, gen_st);
}
extern "C" int gm_post_sw_batch_ix(const gm_index_t* ix, int n, const int* cn, const uint8_t* gen_st, const gm_sw_full_rec_t* recs, const uint8_t* ops, uint64_t ops_len,
                                   const uint32_t* reads, int read_words, const int* rlen, const uint8_t* initbp, const char* const* quals, int is_rna,
                                   gm_post_rec_t* post, char** qralign_out, char** quals_out, uint64_t* quals_len) {
  GM_IX_NULL("gm_post_sw_batch_ix");
  return post_sw_batch_impl(n, recs, ops, ops_len, nullptr, 0, reads, read_words, rlen, initbp, quals, is_rna, post, qralign_out, quals_out, quals_len, ix, cn, gen_st);
}
