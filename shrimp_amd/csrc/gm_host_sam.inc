// gm_host_sam.inc -- gm_sam_records: the SAM text of a chunk's mappings from the arrays of the batch seams; part of gm_host.hip.
//
// The host checks every array against the others, lists the output records (per read its mappings, or its unaligned record) with every integer a record prints --
// POS, NM, and Z0 / Z1 through double_to_neglog, the function the finalisation of the mapping entries prints them with -- and uploads the list beside the caller's
// buffers as they are.  k_sam_records sizes the records, k_win_scan (the scan of gm_read_windows) turns the sizes into offsets, k_sam_records writes the bytes, and the
// offsets and the text come back.  Every buffer is sized by the call's arrays: a fixed number of allocations, copies and launches.

namespace {
// n lines of `want` characters each, '\n' between them (one behind the last is allowed): the bytes to upload, or 0 with the error set
size_t sam_fixed_lines(const char* text, int n, size_t want, const char* what) {
  const char* p = text;
  for (int i = 0; i < n; i++) {
    const size_t avail = strnlen(p, want + 1);                   // (never past the text's end)
    const char* e = (const char*)memchr(p, '\n', avail);
    const size_t len = e ? (size_t)(e - p) : avail;
    if (len != want) { gm_set_error("gm_sam_records: %s: line %d has %s%zu characters, expected %zu", what, i, len > want ? "more than " : "", std::min(len, want), want); return 0; }
    p += want;
    if (i + 1 < n) { if (*p != '\n') { gm_set_error("gm_sam_records: %s: %d lines for %d reads", what, i + 1, n); return 0; } p++; }
  }
  return (size_t)(p - text);
}
}  // namespace

extern "C" int gm_sam_input_size(void) { return (int)sizeof(gm_sam_input_t); }

extern "C" int gm_sam_records(gm_session_t* s, const gm_sam_input_t* in, char** sam, size_t* sam_len, uint64_t* read_off) {
  if (!s || !in || !sam || !sam_len || !read_off) { gm_set_error("gm_sam_records: bad arguments"); return GM_E_ARG; }
  *sam = nullptr; *sam_len = 0; read_off[0] = 0;
  const gm_params_t& P = s->P; const gm_index* ix = s->ix;
  if (P.output_format) { gm_set_error("gm_sam_records: the session prints the SHRiMP format (output_format %d); this entry makes SAM records only", P.output_format); return GM_E_ARG; }
  const int n = in->n_reads, L = in->read_len;
  if (n <= 0) return GM_OK;
  const bool cs = P.colour_space != 0, mqv_on = gm_mqv_on(P), extra = P.extra_sam_fields != 0;
  if (L < 1 || !in->reads_packed) { gm_set_error("gm_sam_records: reads_packed is missing or read_len %d", L); return GM_E_ARG; }
  if (cs != (in->initbp != nullptr)) { gm_set_error(cs ? "gm_sam_records: a colour-space session needs initbp" : "gm_sam_records: initbp belongs to a colour-space session"); return GM_E_ARG; }
  if (!in->map_off) { gm_set_error("gm_sam_records: map_off is missing"); return GM_E_ARG; }
  const uint64_t nm = in->n_maps, nh = in->n_hits;
  if (in->map_off[0] != 0 || in->map_off[n] != nm) { gm_set_error("gm_sam_records: map_off runs from %llu to %llu, the mappings from 0 to %llu", (unsigned long long)in->map_off[0], (unsigned long long)in->map_off[n], (unsigned long long)nm); return GM_E_ARG; }
  for (int r = 0; r < n; r++) if (in->map_off[r + 1] < in->map_off[r] || in->map_off[r + 1] > nm) { gm_set_error("gm_sam_records: map_off not ascending at read %d", r); return GM_E_ARG; }
  if (nm) {
    const char* miss = !in->maps ? "maps" : !in->hits ? "hits" : !in->recs ? "recs" : !in->cigar ? "cigar" : !in->cigar_off ? "cigar_off" : (extra && !in->edit) ? "edit" :
                       (extra && !in->edit_off) ? "edit_off" : (cs && !in->qralign) ? "qralign" : nullptr;
    if (miss) { gm_set_error("gm_sam_records: %s is missing", miss); return GM_E_ARG; }
  }
  // names, seqs, quals: one line a read
  size_t names_bytes = 0, seqs_bytes = 0, quals_bytes = 0;
  std::vector<unsigned long long> name_off;
  if (in->names) {
    name_off.resize((size_t)n + 1);
    const char* p = in->names;
    for (int i = 0; i < n; i++) {
      const char* e = strchr(p, '\n'); if (!e) e = p + strlen(p);
      name_off[i] = (unsigned long long)(p - in->names);
      if (i + 1 < n && !*e) { gm_set_error("gm_sam_records: names: %d lines for %d reads", i + 1, n); return GM_E_ARG; }
      p = e + 1;
    }
    name_off[n] = (unsigned long long)(p - in->names); names_bytes = (size_t)name_off[n] - 1;
  }
  if (in->seqs && !(seqs_bytes = sam_fixed_lines(in->seqs, n, (size_t)L + (cs ? 1 : 0), "seqs"))) return GM_E_ARG;
  if (in->quals && !(quals_bytes = sam_fixed_lines(in->quals, n, (size_t)L, "quals"))) return GM_E_ARG;
  const bool use_pq = cs && in->quals && in->post && in->post_quals;      // post_sw's base qualities (none without QVs, none in local mode)
  // the records
  uint64_t n_recs = 0;
  for (int r = 0; r < n; r++) { const uint64_t m = in->map_off[r + 1] - in->map_off[r]; n_recs += m ? m : (P.sam_unaligned ? 1 : 0); }
  for (int r = 0; r <= n; r++) read_off[r] = 0;
  if (n_recs == 0) return GM_OK;
  if (n_recs >= (1ull << 31)) { gm_set_error("gm_sam_records: %llu records in one call", (unsigned long long)n_recs); read_off[0] = 0; return GM_E_RANGE; }
  std::vector<GmSamRec> recs((size_t)n_recs);
  std::vector<uint64_t> first((size_t)n + 1);
  uint64_t w = 0, ops_hi = 0;
  for (int r = 0; r < n; r++) {
    first[r] = w;
    if (in->map_off[r + 1] == in->map_off[r]) {
      if (P.sam_unaligned) { GmSamRec& o = recs[w++]; memset(&o, 0, sizeof o); o.read = r; o.cn = -1; }
      continue;
    }
    for (uint64_t k = in->map_off[r]; k < in->map_off[r + 1]; k++) {
      const gm_mapping_t& m = in->maps[k];
      if (m.read != r) { gm_set_error("gm_sam_records: mapping %llu says read %d among the mappings of read %d", (unsigned long long)k, m.read, r); return GM_E_ARG; }
      if (m.hit < 0 || (uint64_t)m.hit >= nh) { gm_set_error("gm_sam_records: mapping %llu: hit %d of %llu", (unsigned long long)k, m.hit, (unsigned long long)nh); return GM_E_ARG; }
      const size_t i = (size_t)m.hit;
      const gm_pass1_hit_t& h = in->hits[i]; const gm_sw_full_rec_t& rec = in->recs[i];
      if (h.cn < 0 || h.cn >= ix->n_contigs || h.gen_st < 0 || h.gen_st > 1) { gm_set_error("gm_sam_records: hit %zu: contig %d of %d, strand %d", i, h.cn, ix->n_contigs, h.gen_st); return GM_E_ARG; }
      if (rec.status < 0 || rec.score <= 0) { gm_set_error("gm_sam_records: mapping %llu points to record %zu, which holds no alignment (status %d, score %d)", (unsigned long long)k, i, rec.status, rec.score); return GM_E_ARG; }
      GmSamRec& o = recs[w++]; memset(&o, 0, sizeof o);
      if (in->cigar_off[i + 1] < in->cigar_off[i] || in->cigar_off[i + 1] > in->cigar_off[nh] || in->cigar_off[i + 1] - in->cigar_off[i] > 0xffffffffull) { gm_set_error("gm_sam_records: hit %zu: its cigar slice lies outside the buffer", i); return GM_E_ARG; }
      o.cigar_off = in->cigar_off[i]; o.cigar_len = (uint32_t)(in->cigar_off[i + 1] - in->cigar_off[i]);
      if (extra) {
        if (in->edit_off[i + 1] < in->edit_off[i] || in->edit_off[i + 1] > in->edit_off[nh] || in->edit_off[i + 1] - in->edit_off[i] > 0xffffffffull) { gm_set_error("gm_sam_records: hit %zu: its edit slice lies outside the buffer", i); return GM_E_ARG; }
        o.edit_off = in->edit_off[i]; o.edit_len = (uint32_t)(in->edit_off[i + 1] - in->edit_off[i]);
      }
      int mism = rec.mismatches, xov = rec.crossovers;
      if (cs) {
        if (rec.ops_off > in->ops_len || rec.n_ops > in->ops_len - rec.ops_off) { gm_set_error("gm_sam_records: hit %zu: its qralign slice lies outside the buffer of %llu bytes", i, (unsigned long long)in->ops_len); return GM_E_ARG; }
        long long nq = 0; const char* q = in->qralign + rec.ops_off;
        for (uint32_t t = 0; t < rec.n_ops; t++) nq += q[t] != '-';
        if (rec.read_start < 0 || rec.rmapped < 0 || nq != rec.rmapped || (long long)rec.read_start + nq > L) {
          gm_set_error("gm_sam_records: hit %zu: a qralign slice of %lld read positions behind a clip of %d in a record of %d, read_len %d", i, nq, rec.read_start, rec.rmapped, L); return GM_E_ARG; }
        o.qr_off = rec.ops_off; o.qr_len = rec.n_ops; ops_hi = std::max<uint64_t>(ops_hi, rec.ops_off + rec.n_ops);
        if (in->post) { mism = in->post[i].mismatches; xov = in->post[i].crossovers; }
        if (use_pq && in->post[i].qual_len) {
          const gm_post_rec_t& pr = in->post[i];
          if (pr.qual_off > in->post_quals_len || pr.qual_len > in->post_quals_len - pr.qual_off) { gm_set_error("gm_sam_records: hit %zu: its post_quals slice lies outside the buffer of %llu bytes", i, (unsigned long long)in->post_quals_len); return GM_E_ARG; }
          o.pq_off = pr.qual_off; o.pq_len = pr.qual_len;
        }
      }
      const long long glen = (long long)ix->contig_off[h.cn + 1] - (long long)ix->contig_off[h.cn];
      const long long pos = h.gen_st == 0 ? (long long)rec.genome_start + 1
                                          : (glen - (long long)rec.genome_start) - ((long long)rec.rmapped - 1 - rec.deletions + rec.insertions);   // ref: output.c:626-634
      o.pos = (uint32_t)(unsigned long long)pos;
      o.read = r; o.cn = h.cn; o.flags = h.gen_st; o.mqv = m.mqv; o.as = m.score_full;
      if (mqv_on && !P.all_contigs) { o.z0 = double_to_neglog(m.z0); o.z1 = double_to_neglog(m.z1); }
      o.nm = mism + rec.deletions + rec.insertions; o.cm = xov;
      o.zm = h.matches; o.zr = h.score_window_gen; o.zv = in->score_vector ? in->score_vector[i] : h.score_vector; o.zh = rec.score;
      o.keep_lo = rec.read_start; o.keep_hi = rec.read_start + rec.rmapped;
    }
  }
  first[n] = w;
  // contig names and the read group, end to end
  const size_t rg_len = strnlen(P.read_group, sizeof P.read_group);
  std::vector<uint32_t> cname_off((size_t)ix->n_contigs + 2); std::string cnames;
  for (int c = 0; c < ix->n_contigs; c++) { cname_off[c] = (uint32_t)cnames.size(); cnames += ix->names[c]; }
  cname_off[ix->n_contigs] = (uint32_t)cnames.size(); cnames.append(P.read_group, rg_len); cname_off[(size_t)ix->n_contigs + 1] = (uint32_t)cnames.size();
  const int read_words = (L + 7) / 8;
  const size_t cigar_bytes = nm ? (size_t)in->cigar_off[nh] : 0, edit_bytes = nm && extra ? (size_t)in->edit_off[nh] : 0;
  const size_t pq_bytes = use_pq ? (size_t)in->post_quals_len : 0;
  std::vector<unsigned long long> offs((size_t)n_recs + 1);
  GmDevTurn dev_turn(s);     // (admitted like the mapping entries)
  GM_HIP(hipSetDevice(ix->device));
  hipStream_t q = s->stream;
  GmDevMem mem;
  GmSamArgs A = {};                    // (an absent array stays a null pointer on the device: up() leaves it as it is here)
  A.n_recs = (int)n_recs; A.colour = cs ? 1 : 0; A.read_len = L; A.read_words = read_words; A.n_contigs = ix->n_contigs;
  A.rg_len = (int)rg_len; A.dq = 33 - in->qual_delta; A.ztags = mqv_on && !P.all_contigs ? 1 : 0; A.extra = extra ? 1 : 0;
  GM_HIP(mem.up(&A.recs, recs.data(), (size_t)n_recs, q));
  GM_HIP(mem.up(&A.reads, in->reads_packed, (size_t)n * read_words, q));
  GM_HIP(mem.up(&A.initbp, in->initbp, (size_t)n, q));
  GM_HIP(mem.up(&A.names, in->names, std::max<size_t>(names_bytes, 1), q));
  GM_HIP(mem.up(&A.name_off, name_off.data(), name_off.size(), q));
  GM_HIP(mem.up(&A.seqs, in->seqs, seqs_bytes, q));
  GM_HIP(mem.up(&A.quals, in->quals, quals_bytes, q));
  GM_HIP(mem.up(&A.cigar, in->cigar, cigar_bytes, q));
  GM_HIP(mem.up(&A.edit, in->edit, edit_bytes, q));
  GM_HIP(mem.up(&A.qralign, cs ? in->qralign : nullptr, (size_t)ops_hi, q));
  GM_HIP(mem.up(&A.post_quals, in->post_quals, pq_bytes, q));
  GM_HIP(mem.up(&A.cnames, cnames.data(), std::max<size_t>(cnames.size(), 1), q));
  GM_HIP(mem.up(&A.cname_off, cname_off.data(), cname_off.size(), q));
  GM_HIP(mem.get(&A.lens, (size_t)n_recs * 4));
  unsigned long long* d_offs = nullptr; GM_HIP(mem.get(&d_offs, ((size_t)n_recs + 1) * 8)); A.offs = d_offs;
  int rc = gm_launch_sam_records(A, 0, q); if (rc) return rc;
  rc = gm_launch_win_scan(A.lens, (int)n_recs, 0x7fffffff, d_offs, q); if (rc) return rc;
  GM_HIP(hipMemcpyAsync(offs.data(), d_offs, offs.size() * 8, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  const unsigned long long total = offs[(size_t)n_recs];
  char* text = mem.host((size_t)total + 1);
  if (!text) { gm_set_error("gm_sam_records: out of memory at %llu bytes of text", total); return GM_E_NOMEM; }
  GM_HIP(mem.get(&A.out, (size_t)total));
  rc = gm_launch_sam_records(A, 1, q); if (rc) return rc;
  GM_HIP(hipMemcpyAsync(text, A.out, (size_t)total, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  text[total] = 0;
  for (int r = 0; r <= n; r++) read_off[r] = offs[(size_t)first[r]];
  *sam = mem.give(text); *sam_len = (size_t)total;
  return GM_OK;
}
