// gm_host_records.inc -- the text of a mapping; included by gm_host.hip behind gm_host_finalize.inc (FHit).  Free functions only: what they know of a call is
// RecCtx, what they know of a read is RecRead.
//   sam_record      hit_output, unpaired and paired          ref: gmapper/output.c:227-774 (unmapped :411-466)
//   put_cigar       make_cigar                               ref: output.c:15-64
//   hit_ends        POS and the end of a mapping             ref: mapping.c:414-441, output.c:626-634
//   shrimp_record   --shrimp-format / --pretty               ref: gmapper/output.c:270-296, common/output.c:118-352
struct RecCtx {                     // what text needs of the session
  const gm_params_t& P; const std::vector<std::string>& names; const std::vector<uint32_t>& contig_off;
  const uint32_t* hgen;             // the packed genome on the host (SHRiMP / pretty rows, --extra-sam-fields in letter space)
};
struct RecRead {                    // one read as the records print it
  const char* name; size_t name_len;
  const uint32_t* words; int len;   // packed codes: letters, or colours
  int primer;                       // colour space: the primer letter's code; -1 in letter space
  const char* qual; int qual_delta; // FASTQ input: the QUAL line (null without) and its offset
  const char* text;                 // text input: the read as it stood in the file (letters, or primer + colours); null otherwise
  int ops_stride;                   // bytes an op record may hold
};
struct RecMate {                    // paired mode: the other mate of the record in hand
  bool first, improper;             // this record is the first in its pair; the two mappings are no proper pair
  const FHit* hit;                  // the mate's mapping, null when it has none
  const std::string* seq;           // --sam-r2: the mate's sequence as given, else null
};

static inline char* put_uint(char* p, unsigned long long v) {      // two digits per division (a 64-bit division is ~25 cycles; a record prints half a dozen numbers)
  static const char D2[201] = "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
  if (v < 10) { *p++ = (char)('0' + v); return p; }
  char tmp[24]; int n = 0;
  if (v <= 0xFFFFFFFFull) { uint32_t w = (uint32_t)v; while (w >= 100) { const uint32_t r = w % 100; w /= 100; tmp[n++] = D2[2 * r + 1]; tmp[n++] = D2[2 * r]; } if (w >= 10) { tmp[n++] = D2[2 * w + 1]; tmp[n++] = D2[2 * w]; } else tmp[n++] = (char)('0' + w); }
  else { while (v >= 100) { const unsigned r = (unsigned)(v % 100); v /= 100; tmp[n++] = D2[2 * r + 1]; tmp[n++] = D2[2 * r]; } if (v >= 10) { tmp[n++] = D2[2 * v + 1]; tmp[n++] = D2[2 * v]; } else tmp[n++] = (char)('0' + v); }
  while (n) *p++ = tmp[--n];
  return p;
}
static inline char* put_int(char* p, long long v) { if (v < 0) { *p++ = '-'; return put_uint(p, (unsigned long long)(-v)); } return put_uint(p, (unsigned long long)v); }
static inline char* put_str(char* p, const char* s, size_t n) { memcpy(p, s, n); return p + n; }

static const char CODE2SEQ[17] = "ACGTNNNNNNNNNNNN";   // SEQ letter of an aligned read base (ref: output.c:485-533: non-ACGTN -> N)
static inline char seq_from_text(char c) {          // ref: gmapper/output.c:326-351
  switch (c) { case 'R': case 'Y': case 'S': case 'W': case 'K': case 'M': case 'B': case 'D': case 'H': case 'V': return 'N'; default: return c >= 'a' ? (char)(c - 32) : c; }
}
static inline char rc_char(char c) { switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return 'N'; } }

// dbalign / qralign of a colour-space alignment from the backtrace bytes and letter codes k_pass2_cs wrote (pretty_print, ref: sw-full-cs.c:945-1060)
// recalled: the read letters and lower-case marks k_post_sw_cs left in the spare bits of the backtrace bytes (gm_post.hip) instead of sw_full_cs's own
static void cs_alignment_strings(const uint8_t* bt, const uint8_t* codes, int n, std::string& db, std::string& qr, bool recalled) {
  static const char L[17] = "ACGTUMRWSYKVHDBN";
  db.clear(); qr.clear();
  for (int t = 0; t < n; t++) {
    const int type = bt[t] & 0x0f; const bool xov = recalled ? (bt[t] & 0x40) != 0 : (bt[t] & 0x80) != 0;
    if (type == 1) { db.push_back(L[codes[t] >> 4]); qr.push_back('-'); continue; }
    char q = recalled ? L[(bt[t] >> 4) & 3] : L[codes[t] & 15]; if (xov) q = (char)tolower((unsigned char)q);
    if (type >= 2 && type <= 5) { db.push_back('-'); qr.push_back(q); continue; }
    const char d = L[codes[t] >> 4];
    if (q == 'n' || q == 'N') q = xov ? (char)tolower((unsigned char)d) : d;      // an unknown read letter is shown as the genome's
    db.push_back(d); qr.push_back(q);
  }
}

// dbalign / qralign of a letter-space result from its op record ('M' both, 'I' genome only, 'D' read only), the genome and the read: what sw_full_ls
// hands to the output routines (ref: sw-full-ls.c pretty_print).  A reverse-strand result aligned the read to the reverse complement of the contig.
static void ls_alignment_strings(const RecCtx& C, const GmFullRes& r, const uint8_t* ops, int nops, const uint32_t* rw, std::string& db, std::string& qr) {
  static const char L[17] = "ACGTUMRWSYKVHDBN";
  const uint32_t* hgen = C.hgen; const uint64_t base = C.contig_off[r.cn]; const int glen = (int)(C.contig_off[r.cn + 1] - C.contig_off[r.cn]);
  auto gcode = [&](int j) -> int {
    const uint64_t p = base + (uint64_t)(r.gen_st ? glen - 1 - j : j); int c = (int)((hgen[p >> 3] >> ((p & 7) * 4)) & 0xf);
    if (r.gen_st) c = (int)((0xFBCDE56879A00123ull >> (c * 4)) & 0xf);                    // complement_base, ref: util.h:125-151
    return c; };
  db.clear(); qr.clear();
  int gi = r.genome_start, ri = r.read_start;
  for (int k = 0; k < nops; k++) {
    const char op = (char)ops[k];
    if (op == 'M') { db.push_back(L[gcode(gi++)]); qr.push_back(L[(rw[ri >> 3] >> ((ri & 7) * 4)) & 0xf]); ri++; }
    else if (op == 'I') { db.push_back(L[gcode(gi++)]); qr.push_back('-'); }
    else { db.push_back('-'); qr.push_back(L[(rw[ri >> 3] >> ((ri & 7) * 4)) & 0xf]); ri++; }
  }
}
// ref: common/output.c:36-115
static void edit_string(const std::string& db, const std::string& qr, std::string& o) {
  const int len = (int)db.size(); int consec = 0; bool refgap = false; char nb[16];
  for (int i = 0; i <= len; i++) {
    if (i != len && db[i] == qr[i] && db[i] != '-') { consec++; continue; }
    if (refgap && (consec != 0 || (i == len ? '\0' : db[i]) != '-')) { o += ')'; refgap = false; }
    if (consec != 0) { o.append(nb, snprintf(nb, sizeof nb, "%d", consec)); consec = 0; }
    if (i == len) break;
    if (db[i] == '-') { if (islower((unsigned char)qr[i])) o += 'x'; if (!refgap) o += '('; o += (char)toupper((unsigned char)qr[i]); refgap = true; continue; }
    if (qr[i] == '-') o += '-';
    else if (db[i] == toupper((unsigned char)qr[i])) { o += 'x'; consec++; }
    else if (islower((unsigned char)qr[i])) { o += 'x'; o += (char)toupper((unsigned char)qr[i]); }
    else o += qr[i];
  }
}
// reverse_alignment_edit_string, ref: gmapper/output.c:83-122
static void reverse_edit_string(std::string& e) {
  const int n = (int)e.size(); std::string r(e.size(), ' ');
  for (int i = 0; i < n;) {
    const char c = e[n - 1 - i];
    if (isdigit((unsigned char)c)) { int j = i + 1; while (j < n && isdigit((unsigned char)e[n - 1 - j])) j++; j--; memcpy(&r[i], &e[n - 1 - j], (size_t)(j - i + 1)); i = j + 1; }
    else { r[i] = c == ')' ? '(' : c == '(' ? ')' : c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; i++; }
  }
  e.swap(r);
}
// the optional tail of a SAM record and its newline (ref: output.c:452-465,729-761): R2:Z / X2:Z (--sam-r2), RG:Z (--read-group), --extra-sam-fields of a mapping
static void sam_tail(const gm_params_t& P, std::string& out, const std::string* mate_seq, const FHit* h, const std::string* db, const std::string* qr) {
  if (mate_seq) { out += P.colour_space ? "\tX2:Z:" : "\tR2:Z:"; out += *mate_seq; }
  if (P.read_group[0]) { out += "\tRG:Z:"; out.append(P.read_group, strnlen(P.read_group, sizeof P.read_group)); }
  if (h && P.extra_sam_fields) {
    char b[96]; const GmFullRes& r = *h->r;
    out.append(b, (size_t)snprintf(b, sizeof b, "\tZM:i:%d\tZR:i:%d\tZV:i:%d\tZH:i:%d\tZE:Z:", r.matches, r.score_window_gen, r.score_vector, r.score));
    std::string e; edit_string(*db, *qr, e);
    if (r.gen_st == 1) reverse_edit_string(e);
    out += e;
  }
  out += '\n';
}
// one mapping in the SHRiMP format, with the pretty rows when asked (ref: gmapper/output.c:270-296; common/output.c:280-352 output_normal, :118-262 output_pretty)
static void emit_shrimp(const RecCtx& C, const RecRead& rd, const FHit& h, const std::string& db, const std::string& qr, std::string& out) {
  const gm_params_t& P = C.P; const GmFullRes& r = *h.r; const uint32_t* rw = rd.words; const uint32_t* hgen = C.hgen; const int read_len = rd.len;
  const bool rev = r.gen_st == 1, cs = P.colour_space != 0;
  const uint32_t glen = (uint32_t)(C.contig_off[r.cn + 1] - C.contig_off[r.cn]);
  const uint32_t gs = (uint32_t)r.genome_start, ge = gs + (uint32_t)r.gmapped - 1;
  const uint32_t igs = rev ? glen - ge - 1 : gs, ige = rev ? glen - gs - 1 : ge;
  char b[160];
  out += '>'; out.append(rd.name, rd.name_len); out += '\t'; out += C.names[r.cn]; out += '\t'; out += rev ? '-' : '+';
  out.append(b, snprintf(b, sizeof b, "\t%u\t%u\t%d\t%d\t%d\t%d\t", igs + 1, ige + 1, r.read_start + 1, r.read_start + r.rmapped, read_len, h.score_full));
  edit_string(db, qr, out); out += '\t';
  std::string rstr;                                                                   // readtostr, ref: common/output.c:17-34
  auto read_text = [&]() { static const char LS[17] = "ACGTUMRWSYKVHDBN", CS[17] = "0123!@#$%^&*?~;."; rstr.clear(); if (cs) rstr += LS[rd.primer & 15];
    for (int i = 0; i < read_len; i++) { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; rstr += cs ? CS[c] : LS[c]; } };
  if (P.print_read_seq) { read_text(); out += rstr; }
  out += '\n';
  if (P.output_format != 2) return;
  static const char LS[17] = "ACGTUMRWSYKVHDBN";
  const uint64_t base = C.contig_off[r.cn];
  auto fwd_letter = [&](uint32_t j) { const uint64_t p = base + j; return LS[(hgen[p >> 3] >> ((p & 7) * 4)) & 0xf]; };   // (the reference reads the forward contig here on either strand)
  const uint32_t read_start = (uint32_t)r.read_start, read_end = (uint32_t)(r.read_start + r.rmapped - 1);
  std::string gpre, gpost, lspre, lspost, mpre;
  for (uint32_t j = 0; j < read_start; j++) { gpre += (gs + j > read_start) ? fwd_letter(gs - read_start + j) : '-'; lspre += '-'; mpre += ' '; }
  if (read_end < (uint32_t)read_len - 1) for (uint32_t j = 0; j < (uint32_t)read_len - read_end - 1; j++) { gpost += (ge + 1 + j < glen) ? fwd_letter(ge + 1 + j) : '-'; lspost += '-'; }
  out.append(b, snprintf(b, sizeof b, "G: %10lld    ", (long long)(rev ? ige + 1 : igs + 1))); out += gpre; out += db; out += gpost;
  out.append(b, snprintf(b, sizeof b, "    %-10lld\n", (long long)(rev ? igs + 1 : ige + 1)));
  out.append(b, snprintf(b, sizeof b, "%16s ", "")); out += mpre;
  for (size_t j = 0; j < db.size(); j++) {
    if (db[j] == qr[j] && db[j] != '-') out += '|';
    else if (db[j] == toupper((unsigned char)qr[j])) out += 'X';
    else if (islower((unsigned char)qr[j])) out += 'x';
    else out += ' ';
  }
  out += '\n';
  if (cs) { out.append(b, snprintf(b, sizeof b, "T: %10s    ", "")); out += lspre; out += qr; out += lspost; out += '\n'; }
  else { out.append(b, snprintf(b, sizeof b, "R: %10u    ", read_start + 1)); out += lspre; out += qr; out += lspost; out.append(b, snprintf(b, sizeof b, "    %-10u\n", read_end + 1)); }
  if (cs) {
    out.append(b, snprintf(b, sizeof b, "R: %10u   ", read_start + 1));
    read_text(); size_t k = 0; out += rstr[k++];
    for (uint32_t j = 0; j < read_start; j++) out += rstr[k++];
    for (size_t j = 0; k < rstr.size();) { if (j < qr.size() && qr[j] == '-') out += '-'; else out += rstr[k++]; if (j < qr.size()) j++; }
    out.append(b, snprintf(b, sizeof b, "    %-10u\n", read_end + 1));
  }
  out += '\n';
}
// ... from the mapping alone: the alignment strings are post_sw's in colour space, and built from the op record and the host genome in letter space
static void shrimp_record(const RecCtx& C, const RecRead& rd, const FHit& h, std::string& out) {
  if (C.P.colour_space) { emit_shrimp(C, rd, h, h.db, h.qr, out); return; }
  std::string db, qr; ls_alignment_strings(C, *h.r, h.ops, std::min(h.r->n_ops, rd.ops_stride), rd.words, db, qr);
  emit_shrimp(C, rd, h, db, qr, out);
}

// POS and the last position of a mapping, 1-based on the forward strand (ref: mapping.c:414-441, output.c:626-634)
static void hit_ends(const std::vector<uint32_t>& contig_off, const FHit* h, int* gstart, int* gend) {
  const GmFullRes& r = *h->r;
  const int read_start = r.read_start + 1, read_end = read_start + r.rmapped - 1;
  const int glen = (int)(contig_off[r.cn + 1] - contig_off[r.cn]);
  if (r.gen_st != 1) *gstart = r.genome_start + 1;
  else *gstart = (glen - r.genome_start) - (read_end - read_start - r.n_del + r.n_ins);
  *gend = *gstart + r.gmapped - 1;
}

// CIGAR (make_cigar, ref: output.c:15-64).  Letter space: the runs of the op record ('I' op = gap in the read -> D; 'D' op = gap in the genome -> I), clipped ends
// as S; colour space: the runs of dbalign / qralign, clipped ends as H (ref: output.c:575-579).  Written backwards on the reverse strand.
static char* put_cigar(char* p, bool cs, const FHit& h, int read_len, int ops_stride) {
  const GmFullRes& r = *h.r;
  const int read_start = r.read_start + 1, read_end = read_start + r.rmapped - 1;
  struct Run { int len; char op; }; Run runs[GM_MAX_OPS]; int nr = 0;
  const char clip = cs ? 'H' : 'S';
  if (read_start > 1) runs[nr++] = {read_start - 1, clip};
  if (cs) {
    const int na = (int)h.qr.size();
    for (int i = 0; i < na;) {
      const char op = h.qr[i] == '-' ? 'D' : (h.db[i] == '-' ? 'I' : 'M'); int j = i;
      while (j < na && (h.qr[j] == '-' ? 'D' : (h.db[j] == '-' ? 'I' : 'M')) == op) j++;
      if (nr < GM_MAX_OPS - 1) runs[nr++] = {j - i, op};
      i = j;
    }
  } else {
    const int nops = std::min(r.n_ops, ops_stride);
    for (int i = 0; i < nops;) {
      const char op = (char)h.ops[i]; int j = i; while (j < nops && h.ops[j] == (uint8_t)op) j++;
      if (nr < GM_MAX_OPS - 1) runs[nr++] = {j - i, op == 'M' ? 'M' : (op == 'I' ? 'D' : 'I')};
      i = j;
    }
  }
  if (read_end != read_len) runs[nr++] = {read_len - read_end, clip};
  if (r.gen_st != 1) for (int i = 0; i < nr; i++) { p = put_uint(p, (unsigned)runs[i].len); *p++ = runs[i].op; }
  else for (int i = nr - 1; i >= 0; i--) { p = put_uint(p, (unsigned)runs[i].len); *p++ = runs[i].op; }
  return p;
}

// One SAM record (hit_output, ref: output.c:227-774): the mapping h of read rd, or its unmapped record when h is null (ref: output.c:411-466); mate: null for an
// unpaired read, else the other mate of the pair.  Where the unpaired and the paired records of the reference differ, the difference hangs on `mate`.
static void sam_record(const RecCtx& C, const RecRead& rd, const FHit* h, const RecMate* mate, std::string& out) {
  const gm_params_t& P = C.P; const bool cs = P.colour_space != 0;
  const uint32_t* rw = rd.words; const int read_len = rd.len; const char* qual = rd.qual;
  const FHit* mh = mate ? mate->hit : nullptr; const std::string* mate_seq = mate ? mate->seq : nullptr;
  const bool rev_mp = mh && mh->r->gen_st == 1;
  int gstart_mp = 0, gend_mp = 0; const std::string* mrnm = nullptr;                   // PNEXT stays 0 and RNEXT '*' without a mapped mate
  if (mh) { hit_ends(C.contig_off, mh, &gstart_mp, &gend_mp); mrnm = &C.names[mh->r->cn]; }
  const int pair_flags = !mate ? 0 : 0x1 | (mh ? 0 : 0x8) | (rev_mp ? 0x20 : 0) | (mate->first ? 0x40 : 0x80);
  // The record is assembled in a buffer on the stack and appended (its bound -- every CIGAR operation a run of its own; SEQ, QUAL and in colour space CQ, CS, XX --
  // is several times the record, and std::string::resize zero-fills what it adds); a record beyond the buffer grows the string in place.
  const size_t bound = rd.name_len + (cs ? 8 : 5) * (size_t)read_len + 400 + (h ? 12 * (size_t)h->r->n_ops + C.names[h->r->cn].size() : 0) + (mrnm ? mrnm->size() : 0);
  char stage[6144]; const bool staged = bound <= sizeof stage;
  if (!staged) { const size_t o = out.size(); out.resize(o + bound); }
  char* p = staged ? stage : &out[out.size() - bound];
  auto commit = [&](char* e) { if (staged) out.append(stage, (size_t)(e - stage)); else out.resize((size_t)(e - out.data())); };
  // colour space: the read as csfasta text, primer letter + colours ('.' for a skipped cycle), for the CS:Z tag (ref: output.c:451,730)
  auto put_csfasta = [&](char* q) { if (rd.text) return put_str(q, rd.text, (size_t)read_len + 1);     // verbatim, as the reference prints re->seq
    *q++ = "ACGT"[rd.primer & 3]; for (int i = 0; i < read_len; i++) { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; *q++ = (c < 4) ? (char)('0' + c) : '.'; } return q; };
  p = put_str(p, rd.name, rd.name_len); *p++ = '\t';
  if (!h) {
    p = put_int(p, mate ? pair_flags | 0x4 : 4); p = put_str(p, "\t*\t0\t0\t*\t", 9);
    if (mrnm) p = put_str(p, mrnm->data(), mrnm->size()); else *p++ = '*';
    *p++ = '\t'; p = put_uint(p, (unsigned)gstart_mp); p = put_str(p, "\t0\t", 3);
    if (cs) {                                                                         // ref: output.c:353-355,441-451
      p = put_str(p, "*\t*\tCQ:Z:", 9); if (qual) p = put_str(p, qual, (size_t)read_len); else *p++ = '*';
      p = put_str(p, "\tCS:Z:", 6); p = put_csfasta(p);
    } else {
      if (rd.text) for (int i = 0; i < read_len; i++) *p++ = seq_from_text(rd.text[i]);
      else {      // (the reference prints the file's own letters here: a U stays a U; its paired records know the other codes only as N)
        const char* L = mate ? "ACGTUNNNNNNNNNNN" : "ACGTUMRWSYKVHDBN";
        for (int i = 0; i < read_len; i++) *p++ = L[(rw[i >> 3] >> ((i & 7) * 4)) & 0xf];
      }
      if (qual) { *p++ = '\t'; p = put_str(p, qual, (size_t)read_len); }               // ref: output.c:419-421 (verbatim)
      else p = put_str(p, "\t*", 2);
    }
    commit(p); sam_tail(P, out, mate_seq, nullptr, nullptr, nullptr);
    return;
  }
  const GmFullRes& r = *h->r; const std::string& rname = C.names[r.cn];
  const bool rev = r.gen_st == 1, proper = mh && !mate->improper;
  const int read_start = r.read_start + 1, read_end = read_start + r.rmapped - 1;
  int gstart, gend; hit_ends(C.contig_off, h, &gstart, &gend);
  p = put_int(p, pair_flags | (proper ? 0x2 : 0) | (rev ? 0x10 : 0)); *p++ = '\t';
  p = put_str(p, rname.data(), rname.size()); *p++ = '\t';
  p = put_uint(p, (unsigned)gstart); *p++ = '\t';
  p = put_int(p, h->mqv); *p++ = '\t';
  p = put_cigar(p, cs, *h, read_len, rd.ops_stride); *p++ = '\t';
  int isize = 0;                                                                      // TLEN: from 5' end to 5' end on one contig (ref: output.c:640-655)
  if (!mh) *p++ = '*';
  else if (rname == *mrnm) { *p++ = '='; isize = (rev_mp ? gend_mp : gstart_mp - 1) - (rev ? gend : gstart - 1); }
  else p = put_str(p, mrnm->data(), mrnm->size());
  *p++ = '\t'; p = put_uint(p, (unsigned)gstart_mp); *p++ = '\t'; p = put_int(p, isize); *p++ = '\t';
  if (cs) {   // SEQ = the aligned letters post_sw called (ref: output.c:485-537)
    auto up = [](char c) { if (c >= 'a') c -= 32; return (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N') ? c : 'N'; };
    const int na = (int)h->qr.size();
    if (!rev) { for (int i = 0; i < na; i++) if (h->qr[i] != '-') *p++ = up(h->qr[i]); }
    else for (int i = na - 1; i >= 0; i--) if (h->qr[i] != '-') *p++ = rc_char(up(h->qr[i]));
  } else if (!rd.text || (read_start == 1 && read_end == read_len)) {
    // SEQ: read bases in input orientation (aligned part from qralign == the read's own letters), revcomp on '-'.  Every base from its code: eight to a word, the
    // reverse strand through the complement's letters
    static const char RC2SEQ[17] = "TGCANNNNNNNNNNNN";                             // rc_char(CODE2SEQ[c])
    if (!rev) { for (int i = 0; i < read_len; i += 8) { uint32_t x = rw[i >> 3]; const int m = std::min(8, read_len - i); for (int k = 0; k < m; k++) { *p++ = CODE2SEQ[x & 15u]; x >>= 4; } } }
    else { for (int i = read_len - 1; i >= 0;) { const uint32_t x = rw[i >> 3]; for (int k = i & 7; k >= 0; k--, i--) *p++ = RC2SEQ[(x >> (4 * k)) & 15u]; } }
  } else {
    // text input: the clipped ends -- local mode only -- keep the file's letters (ref: output.c:326-351,482-533; on the reverse strand the reference's reverse()
    // knows no 'X' / 'U' and exits there, those print as N here)
    auto seq_at = [&](int i) -> char { const int c = (rw[i >> 3] >> ((i & 7) * 4)) & 0xf; return (i < read_start - 1 || i >= read_end) ? seq_from_text(rd.text[i]) : CODE2SEQ[c]; };
    if (!rev) for (int i = 0; i < read_len; i++) *p++ = seq_at(i);
    else for (int i = read_len - 1; i >= 0; i--) { const char c = seq_at(i); *p++ = c == '.' ? '.' : rc_char(c); }
  }
  *p++ = '\t';
  if (cs && qual && !h->qual.empty()) {                                               // post_sw's base qualities, ref: output.c:613-621 (none in local mode: no post_sw there)
    const int nq = (int)h->qual.size();
    if (!rev) p = put_str(p, h->qual.data(), (size_t)nq); else for (int i = nq - 1; i >= 0; i--) *p++ = h->qual[i];
  } else if (!cs && qual) {                                                           // reversed with the read, re-based to PHRED+33 (ref: output.c:539-570)
    const int dq = 33 - rd.qual_delta;
    if (!rev) for (int i = 0; i < read_len; i++) *p++ = (char)(qual[i] + dq);
    else for (int i = read_len - 1; i >= 0; i--) *p++ = (char)(qual[i] + dq);
  } else *p++ = '*';
  p = put_str(p, "\tAS:i:", 6); p = put_int(p, h->score_full);
  auto z = [&](const char* tag, double v) { p = put_str(p, tag, 6); p = put_int(p, double_to_neglog(v)); };
  if (!gm_mqv_on(P) || P.all_contigs) {}                                               // no Z tags without mapping qualities or with --all-contigs (ref: output.c:691-696)
  else if (!mate) { z("\tZ0:i:", h->z0); z("\tZ1:i:", h->z1); }
  else if (proper) { z("\tZ2:i:", h->z2); z("\tZ3:i:", h->z3); z("\tZ4:i:", h->pr_top_random); z("\tZ6:i:", h->insert_size_denom); }
  else { z("\tZ0:i:", h->z0); z("\tZ1:i:", h->z1); z("\tZ4:i:", h->pr_top_random); z("\tZ5:i:", h->pr_missed_mp); }
  p = put_str(p, "\tNM:i:", 6); p = put_int(p, (cs ? h->cs_mismatch : r.n_mismatch) + r.n_del + r.n_ins);
  if (cs) {                                                                           // the colour-space tags (ref: output.c:717-730)
    if (qual) { p = put_str(p, "\tCQ:Z:", 6); p = put_str(p, qual, (size_t)read_len); }
    p = put_str(p, "\tCS:Z:", 6); p = put_csfasta(p);
    p = put_str(p, "\tCM:i:", 6); p = put_int(p, h->cs_xover);
    p = put_str(p, "\tXX:Z:", 6); p = put_str(p, h->qr.data(), h->qr.size());
  }
  commit(p);
  if (P.extra_sam_fields && !cs) { std::string db, qr; ls_alignment_strings(C, r, h->ops, std::min(r.n_ops, rd.ops_stride), rw, db, qr); sam_tail(P, out, mate_seq, h, &db, &qr); }
  else sam_tail(P, out, mate_seq, h, &h->db, &h->qr);
}
