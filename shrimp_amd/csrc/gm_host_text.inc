// gm_host_text.inc -- the text of a batch's alignments: gm_sw_full_batch_text[_ix] (k_sw_text, gm_text.hip); part of gm_host.hip.
//
// dbalign / qralign as gm_sw_full_batch_strings builds them, the CIGAR and the edit string of every record of one gm_sw_full_*_batch[_ix] call, in one call: a fixed
// number of device buffers, copies and launches whatever n is.  A record is checked here, on the host, before anything is uploaded; the sizing launch leaves the
// CIGAR / edit-string lengths of the accepted ones, their exclusive scan in item order gives the tight offsets the writing launch stores at.
static int sw_full_batch_text_impl(int colour, int what, int n, const gm_sw_full_rec_t* recs, const uint8_t* ops, uint64_t ops_len, const uint32_t* genome, uint64_t genome_words,
                                   const uint32_t* reads, int read_words, const int* rlen, const uint8_t* initbp, int is_rna, const char* qralign_in, const uint8_t* reverse,
                                   int clip_char, int* status, char** dbalign_out, char** qralign_out, char** cigar_out, uint64_t* cigar_off, char** edit_out, uint64_t* edit_off,
                                   const gm_index_t* ix = nullptr, const int* cn = nullptr, const uint8_t* gen_st = nullptr) {
  const char* who = ix ? "gm_sw_full_batch_text_ix" : "gm_sw_full_batch_text";
  if (what <= 0 || (what & ~(GM_TEXT_ALIGN | GM_TEXT_CIGAR | GM_TEXT_EDIT))) { gm_set_error("%s: what is none of GM_TEXT_ALIGN | GM_TEXT_CIGAR | GM_TEXT_EDIT", who); return GM_E_ARG; }
  if (n <= 0) return GM_OK;
  const bool want_al = what & GM_TEXT_ALIGN, want_cig = what & GM_TEXT_CIGAR, want_ed = what & GM_TEXT_EDIT, strings = want_al || want_ed;
  if (!recs || (!ops && ops_len) || (ix ? (!cn || !gen_st) : !genome) || !rlen || !status || (strings && !qralign_in && (!reads || read_words < 1)) ||
      (colour && strings && !qralign_in && !initbp) || (want_al && (!dbalign_out || !qralign_out)) || (want_cig && (!cigar_out || !cigar_off)) || (want_ed && (!edit_out || !edit_off))) {
    gm_set_error("%s: a required argument is missing", who); return GM_E_ARG; }
  if (want_cig && clip_char != 'S' && clip_char != 'H') { gm_set_error("%s: clip_char is neither 'S' nor 'H'", who); return GM_E_ARG; }
  IxScope scope;
  if (ix) { const int rc = scope.enter(ix, is_rna); if (rc) return rc; is_rna = scope.view.genome_is_rna; }
  const bool translate = colour && strings && !qralign_in, use_reads = strings && !qralign_in;
  std::vector<GmTextItem> items; items.reserve(n);
  for (int i = 0; i < n; i++) {
    const gm_sw_full_rec_t& R = recs[i];
    status[i] = 0;
    if (R.status < 0) { status[i] = R.status; continue; }
    if (R.score <= 0) continue;                                           // no alignment: status 0, empty slices
    auto refuse = [&](const char* why) { status[i] = GM_E_ARG; gm_set_error("%s: item %d refused: %s", who, i, why); };
    uint64_t genome_len = genome_words * 8; GmWin win;
    if (ix) {
      if (const char* why = ix_window(ix, cn[i], gen_st[i], 0, 0, &win, true)) { refuse(why); continue; }
      genome_len = (uint64_t)ix->contig_off[win.cn + 1] - (uint64_t)ix->contig_off[win.cn];
    }
    if (use_reads && (rlen[i] < 0 || ((uint64_t)rlen[i] + 7) / 8 > (uint64_t)read_words)) { refuse("read outside the bitfield"); continue; }
    if (colour && initbp && initbp[i] > 3) { refuse("initbp outside 0..3"); continue; }
    uint64_t adv_r = 0;
    if (const char* why = swf_rec_check(colour != 0, &R, ops, ops_len, genome_len, rlen[i], &adv_r)) { refuse(why); continue; }
    if (R.n_ops > (1u << 27)) { refuse("an alignment of more than 2^27 columns"); continue; }
    if (qralign_in && strings) {                                          // its gaps are the operations' (post_sw re-calls letters, it moves no gap)
      const uint8_t* o = ops + R.ops_off; const char* q = qralign_in + R.ops_off; bool same = true;
      for (uint32_t k = 0; k < R.n_ops && same; k++) same = (q[k] == '-') == (colour ? (o[k] & 0x0f) == 1 : o[k] == 'I');
      if (!same) { refuse("qralign_in has a gap where the operations have none, or none where they have one"); continue; }
    }
    GmTextItem it; memset(&it, 0, sizeof it);
    it.ops_off = R.ops_off; it.n_ops = R.n_ops; it.genome_start = R.genome_start; it.read_start = R.read_start; it.tail = (int)((int64_t)rlen[i] - R.read_start - (int64_t)adv_r);
    it.initbp = translate ? initbp[i] : 0; it.idx = i; it.flags = (reverse && reverse[i]) ? 4 : 0;
    if (ix) {
      it.gbase = (long long)ix->contig_off[win.cn] + (win.rc ? (long long)genome_len - 1 : 0);
      it.flags |= (win.rc ? 1 : 0) | ((ix->rna_ready && ix->contig_rna[win.cn]) ? 2 : 0);
    }
    items.push_back(it);
  }
  const size_t m = items.size();
  std::vector<uint64_t> coff, eoff;                                       // n + 1 each, in item order
  if (want_cig) coff.assign((size_t)n + 1, 0);
  if (want_ed) eoff.assign((size_t)n + 1, 0);
  GmDevMem results; char* hp[4] = {nullptr, nullptr, nullptr, nullptr};      // dbalign, qralign, cigar, edit (the device buffers have a holder and a scope of their own below)
  if (want_al) { hp[0] = results.host(ops_len ? ops_len : 1, true); hp[1] = results.host(ops_len ? ops_len : 1, true); if (!hp[0] || !hp[1]) { gm_set_error("%s: out of memory", who); return GM_E_NOMEM; } }
  uint64_t cig_total = 0, edit_total = 0;
  if (m) {
    if (gm_device_count() < 1) { gm_set_error("no HIP device"); return GM_E_NODEVICE; }
    GmDevMem mem;
    uint32_t *dg = nullptr, *dr = nullptr, *dlens = nullptr; GmTextItem* di = nullptr; unsigned long long* doffs = nullptr;
    uint8_t *dops = nullptr, *dqin = nullptr, *ddb = nullptr, *dqr = nullptr, *dcig = nullptr, *ded = nullptr;
    if (strings) {
      if (ix) dg = ix->d_genome;
      else {
        GM_HIP(mem.get(&dg, (genome_words + 8) * 4));
        GM_HIP(hipMemsetAsync(dg + genome_words, 0, 8 * 4, 0));
        GM_HIP(hipMemcpyAsync(dg, genome, genome_words * 4, hipMemcpyHostToDevice, 0));
      }
      if (use_reads) GM_HIP(mem.up(&dr, reads, (size_t)n * read_words, 0, 32));
      else { GM_HIP(mem.get(&dqin, (size_t)ops_len + 16)); GM_HIP(hipMemcpyAsync(dqin, qralign_in, (size_t)ops_len, hipMemcpyHostToDevice, 0)); }
    }
    GM_HIP(mem.up(&di, items.data(), m, 0));
    GM_HIP(mem.get(&dops, (size_t)ops_len + 16)); GM_HIP(hipMemcpyAsync(dops, ops, (size_t)ops_len, hipMemcpyHostToDevice, 0));
    GM_HIP(mem.get(&dlens, m * 2 * sizeof(uint32_t))); GM_HIP(mem.get(&doffs, m * 2 * sizeof(unsigned long long)));
    std::vector<unsigned long long> offs(m * 2, 0);
    if (want_cig || want_ed) {
      int rc = gm_launch_sw_text((int)m, di, colour ? 1 : 0, what, 0, dops, dg, dr, read_words, is_rna ? 1 : 0, dqin, clip_char, dlens, doffs, nullptr, nullptr, nullptr, nullptr, 0, ix ? 1 : 0);
      if (rc != GM_OK) { (void)hipDeviceSynchronize(); gm_set_error("%s: the kernel launch failed", who); return rc; }
      std::vector<uint32_t> lens(m * 2);
      GM_HIP(hipMemcpyAsync(lens.data(), dlens, m * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, 0));
      GM_HIP(hipStreamSynchronize(0));
      // the exclusive scan in item order (items[] is in item order: refused items and those without alignment take no bytes)
      size_t k = 0;
      for (int i = 0; i < n; i++) {
        if (want_cig) coff[i] = cig_total;
        if (want_ed) eoff[i] = edit_total;
        if (k < m && items[k].idx == i) { offs[2 * k] = cig_total; offs[2 * k + 1] = edit_total; cig_total += lens[2 * k]; edit_total += lens[2 * k + 1]; k++; }
      }
      if (want_cig) coff[n] = cig_total;
      if (want_ed) eoff[n] = edit_total;
      GM_HIP(hipMemcpyAsync(doffs, offs.data(), m * 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, 0));
    }
    if (want_al) {
      GM_HIP(mem.get(&ddb, (size_t)ops_len + 16)); GM_HIP(mem.get(&dqr, (size_t)ops_len + 16));
      GM_HIP(hipMemsetAsync(ddb, 0, (size_t)ops_len + 16, 0)); GM_HIP(hipMemsetAsync(dqr, 0, (size_t)ops_len + 16, 0));
    }
    if (want_cig) GM_HIP(mem.get(&dcig, (size_t)cig_total + 16));
    if (want_ed) GM_HIP(mem.get(&ded, (size_t)edit_total + 16));
    int rc = gm_launch_sw_text((int)m, di, colour ? 1 : 0, what, 1, dops, dg, dr, read_words, is_rna ? 1 : 0, dqin, clip_char, dlens, doffs, ddb, dqr, dcig, ded, 0, ix ? 1 : 0);
    if (rc != GM_OK) { (void)hipDeviceSynchronize(); gm_set_error("%s: the kernel launch failed", who); return rc; }
    if (want_cig) { hp[2] = results.host(cig_total ? cig_total : 1); if (!hp[2]) { (void)hipDeviceSynchronize(); gm_set_error("%s: out of memory", who); return GM_E_NOMEM; } }
    if (want_ed) { hp[3] = results.host(edit_total ? edit_total : 1); if (!hp[3]) { (void)hipDeviceSynchronize(); gm_set_error("%s: out of memory", who); return GM_E_NOMEM; } }
    if (want_al && ops_len) {
      GM_HIP(hipMemcpyAsync(hp[0], ddb, (size_t)ops_len, hipMemcpyDeviceToHost, 0));
      GM_HIP(hipMemcpyAsync(hp[1], dqr, (size_t)ops_len, hipMemcpyDeviceToHost, 0));
    }
    if (want_cig && cig_total) GM_HIP(hipMemcpyAsync(hp[2], dcig, (size_t)cig_total, hipMemcpyDeviceToHost, 0));
    if (want_ed && edit_total) GM_HIP(hipMemcpyAsync(hp[3], ded, (size_t)edit_total, hipMemcpyDeviceToHost, 0));
    GM_HIP(hipStreamSynchronize(0));
  } else {
    if (want_cig) hp[2] = results.host(1);
    if (want_ed) hp[3] = results.host(1);
    if ((want_cig && !hp[2]) || (want_ed && !hp[3])) { gm_set_error("%s: out of memory", who); return GM_E_NOMEM; }
  }
  if (want_al) { *dbalign_out = results.give(hp[0]); *qralign_out = results.give(hp[1]); }
  if (want_cig) { *cigar_out = results.give(hp[2]); memcpy(cigar_off, coff.data(), ((size_t)n + 1) * sizeof(uint64_t)); }
  if (want_ed) { *edit_out = results.give(hp[3]); memcpy(edit_off, eoff.data(), ((size_t)n + 1) * sizeof(uint64_t)); }
  return GM_OK;
}
extern "C" int gm_sw_full_batch_text(int colour_space, int what, int n, const gm_sw_full_rec_t* recs, const uint8_t* ops, uint64_t ops_len, const uint32_t* genome, uint64_t genome_words,
                                     const uint32_t* reads, int read_words, const int* rlen, const uint8_t* initbp, int is_rna, const char* qralign_in, const uint8_t* reverse,
                                     int clip_char, int* status, char** dbalign_out, char** qralign_out, char** cigar_out, uint64_t* cigar_off, char** edit_out, uint64_t* edit_off) {
  return sw_full_batch_text_impl(colour_space, what, n, recs, ops, ops_len, genome, genome_words, reads, read_words, rlen, initbp, is_rna ? 1 : 0, qralign_in, reverse, clip_char, status,
                                 dbalign_out, qralign_out, cigar_out, cigar_off, edit_out, edit_off);
}
extern "C" int gm_sw_full_batch_text_ix(const gm_index_t* ix, int colour_space, int what, int n, const int* cn, const uint8_t* gen_st, const gm_sw_full_rec_t* recs, const uint8_t* ops,
                                        uint64_t ops_len, const uint32_t* reads, int read_words, const int* rlen, const uint8_t* initbp, int is_rna, const char* qralign_in,
                                        const uint8_t* reverse, int clip_char, int* status, char** dbalign_out, char** qralign_out, char** cigar_out, uint64_t* cigar_off,
                                        char** edit_out, uint64_t* edit_off) {
  GM_IX_NULL("gm_sw_full_batch_text_ix");
  return sw_full_batch_text_impl(colour_space, what, n, recs, ops, ops_len, nullptr, 0, reads, read_words, rlen, initbp, is_rna, qralign_in, reverse, clip_char, status,
                                 dbalign_out, qralign_out, cigar_out, cigar_off, edit_out, edit_off, ix, cn, gen_st);
}
