// gm_host_files.inc -- the read loop's input side (SURVEY A22, 8(f)4): the reference's reads reader, its per-read preprocessing, and the file entry points, which stream
// a file in bounded chunks (ref: gmapper/gmapper.c:286-645 launch_scan_threads -- chunks of reads, trimming, QV checks, dropped reads; common/fasta.c:61-150 fasta_open,
// :242-283 extract_name, :315-552 fasta_get_next_read_with_range).  Included by gm_host.hip behind map_impl / map_pairs_impl.  Host code only.
//
// The reference reads 1 000 reads per thread and chunk; here a chunk is up to 1 M reads (what fills the device pipeline), read and preprocessed by a second thread while
// the chunk before it is being mapped; every chunk's records go to the caller's write function in the file's order, so neither the file nor the output is ever held whole.

// ---- per-read preprocessing (ref: gmapper.c:262-284 trim_read, :427-453 trimming and the Illumina "B" tail, :455-472 quality checks, :495-521 dropped reads) ----
// mate: 0 unpaired, 1 / 2 the mates of a pair.  seq holds the primer letter first in colour space.  *drop: the read gets no record at all (too long, mean QV too low).
static int gm_preprocess_read(const gm_params_t& P, bool have_q, int qual_delta, int mate, std::string& seq, std::string& qual, const std::string& name, bool* drop) {
  *drop = false;
  const bool cs = P.colour_space != 0, use_q = have_q && !P.ignore_qvs;
  const bool trim = P.trim_front > 0 || P.trim_end > 0;
  if (trim && (mate == 0 || (mate == 1 ? P.trim_first : P.trim_second))) {                       // ref: gmapper.c:427-438, trim_read :262-284
    const long keep = (long)seq.size() - P.trim_end - P.trim_front;
    if (keep <= 0) { seq.clear(); if (have_q) qual.clear(); }
    else { seq = seq.substr((size_t)P.trim_front, (size_t)keep); if (have_q) qual = qual.substr(std::min(qual.size(), (size_t)P.trim_front), (size_t)keep); }
  }
  if (!cs && P.trim_illumina && have_q) {                                                        // ref: gmapper.c:440-453 (letter space: a tail of 'B' quality values goes)
    size_t nb = 0; for (char c : qual) nb = c == 'B' ? nb + 1 : 0;
    if (nb > 0) { seq.resize(seq.size() - std::min(seq.size(), nb)); qual.resize(qual.size() - nb); }
  }
  const int read_len = (int)seq.size() - (cs ? 1 : 0);
  int avg_qv = 0;
  if (use_q && P.min_avg_qv >= 0) for (char c : qual) avg_qv += (int)c - qual_delta;             // ref: gmapper.c:456-462
  if (use_q && !P.no_qv_check) for (char c : qual) {                                             // ref: gmapper.c:463-472 (the binary exits here)
    const int qv = (int)c - qual_delta;
    if (qv < -10 || qv > 50) { gm_set_error("the quality offset might be set incorrectly: PHRED+%d gives a quality value of %d (read \"%s\"); set no_qv_check to go on (ref: gmapper.c:463-472)", qual_delta, qv, name.c_str()); return GM_E_ARG; }
  }
  if (read_len > 0) avg_qv /= read_len;                                                          // ref: gmapper.c:491-492 (integer mean)
  if (read_len < 1 || read_len > P.longest_read_len || (use_q && avg_qv < P.min_avg_qv)) *drop = true;      // ref: gmapper.c:495-521
  return GM_OK;
}
// The reference trims the FIRST mate of a pair after it has packed it (gmapper.c:427-438 runs at the second mate's turn, :474-475 packed the first one a turn earlier): its
// records then print a sequence that is shorter than its length field.  That combination is refused here instead of reproduced.
static int gm_check_pair_trim(const gm_params_t& P) {
  if ((P.trim_front > 0 || P.trim_end > 0) && P.trim_first) {
    gm_set_error("paired mode: trimming the first mate is not supported -- the reference trims it after packing it (ref: gmapper.c:427-438,474-475); use trim_first = 0, trim_second = 1 (--trim-second)");
    return GM_E_ARG; }
  return GM_OK;
}

struct FileRead { std::string name, seq, qual; };
// the reads reader, one read per call
struct ReadsFile {
  gzFile fp = nullptr; bool fastq = false, eof = false, have_pending = false, stopped = false; char mark = '>'; int colour_space = 0;
  std::string line, pending; std::vector<char> buf; size_t bpos = 0, blen = 0;      // a block of the (decompressed) file and the part of it already handed out
  ReadsFile() : buf(4u << 20) {}
  ~ReadsFile() { if (fp) gzclose(fp); }
  ReadsFile(const ReadsFile&) = delete; ReadsFile& operator=(const ReadsFile&) = delete;
  int open(const char* path, int cs, int fastq_flag) {
    colour_space = cs;
    fp = gzopen(path, "r");
    if (!fp) { gm_set_error("cannot open '%s' for reading", path); return GM_E_ARG; }
    gzbuffer(fp, 1 << 20);
    if (fastq_flag < 0) {                                            // ref: fasta.c:99-127
      int c = gzgetc(fp);
      while (c == '#' || c == ';') { while (c != -1 && c != '\n') c = gzgetc(fp); if (gzeof(fp)) break; if (c == -1) break; c = gzgetc(fp); }
      fastq_flag = 0;
      if (!gzeof(fp) && c != -1) {
        if (c == '@') fastq_flag = 1; else if (c == '>') fastq_flag = 0;
        else { gm_set_error("unrecognized character [%c] in input file [%s]", (char)c, path); return GM_E_ARG; }
        gzungetc(c, fp);
      }
    }
    fastq = fastq_flag != 0; mark = fastq ? '@' : '>';
    return GM_OK;
  }
  bool getline(std::string& l) {                                     // one line without its '\n' (blocks of 4 MB through gzread, the line ends by memchr: gzgets per line was the reader's time)
    l.clear();
    for (;;) {
      if (bpos == blen) {
        const int n = gzread(fp, buf.data(), (unsigned)buf.size());
        if (n <= 0) { eof = true; return !l.empty(); }
        bpos = 0; blen = (size_t)n;
      }
      const char* b = buf.data() + bpos;
      const char* e = (const char*)memchr(b, '\n', blen - bpos);
      if (e) { l.append(b, (size_t)(e - b)); bpos += (size_t)(e - b) + 1; return true; }
      l.append(b, blen - bpos); bpos = blen;
    }
  }
  // 1: a read; 0: the end of the file, or a malformed entry (the reference stops reading there); < 0: error
  int next(FileRead& R) {
    if (stopped) return 0;
    R.name.clear(); R.seq.clear(); R.qual.clear();
    // ---- name line ----
    bool got = false;
    for (;;) {
      if (have_pending) { line.swap(pending); have_pending = false; } else if (!getline(line)) break;
      if (line.empty()) { got = false; break; }
      if (line[0] == '#') continue;
      if (line[0] != mark) { got = false; line.clear(); break; }      // "Expecting ..." -- the reference stops reading here
      got = true; break;
    }
    if (!got || line.size() <= 1) { stopped = true; return 0; }
    R.name = gm_extract_name(line);
    // ---- sequence ----
    bool plus = false;
    for (;;) {
      if (!getline(line)) break;
      if (fastq && !line.empty() && line[0] == '+') { plus = true; break; }
      if (!fastq && !line.empty() && line[0] == '>') { pending = line; have_pending = true; break; }
      if (!line.empty() && line[0] == '#') continue;
      R.seq += line;
    }
    if (R.seq.empty()) { stopped = true; return 0; }
    if (fastq) {
      if (!plus) { stopped = true; return 0; }
      const size_t want = R.seq.size() - (colour_space ? 1 : 0);
      for (;;) {
        if (!getline(line)) break;
        R.qual += line;
        if (R.qual.size() >= want) break;
      }
      if (R.qual.size() != want) {
        if (R.qual.size() > want) { gm_set_error("read \"%s\": the quality string is longer than the sequence (ref: fasta.c:478-482)", R.name.c_str()); return GM_E_ARG; }
        stopped = true; return 0;
      }
      for (char& c : R.qual) c = std::max(c, '!');
    }
    if (eof && !have_pending) stopped = true;                          // (this read is the last one)
    return 1;
  }
};

static void gm_stats_add(gm_map_stats_t& total, const gm_map_stats_t& st) {
  uint64_t* a = (uint64_t*)&total; const uint64_t* b = (const uint64_t*)&st;                      // the counters: every field up to the stage times
  const size_t nu = offsetof(gm_map_stats_t, ms_lookup) / sizeof(uint64_t); for (size_t k = 0; k < nu; k++) a[k] += b[k];
  total.ms_lookup += st.ms_lookup; total.ms_anchors += st.ms_anchors; total.ms_pass1 += st.ms_pass1; total.ms_select += st.ms_select; total.ms_pass2 += st.ms_pass2; total.ms_host += st.ms_host;
}
// a buffer map_impl / map_pairs_impl handed out is freed here, not by the caller of the file entry
static void gm_release_group_text(char* p) { if (!p) return; { std::lock_guard<std::mutex> lk(g_outcache.m); if (p == g_outcache.live) g_outcache.live = nullptr; } free(p); }

// A chunk as the reader thread hands it over: the reads that survived the preprocessing, already sorted into groups of one length (the device pipeline takes batches of one
// length) with their texts joined and their codes packed -- the mapping thread only calls map_impl per group and puts the records back into the file's order.
struct ReadGroup { int L[2] = {0, 0}; uint32_t n = 0; std::string seqs[2], names[2], quals[2]; std::vector<uint32_t> packed[2]; std::vector<uint8_t> ibp[2]; };      // [1]: the second mates (pairs)
struct ReadChunk { std::vector<ReadGroup> groups; std::vector<uint32_t> group_of; int rc = GM_OK; std::string err; bool last = false; };      // group_of: per kept read / pair, in file order
static int gm_pack_group(ReadGroup& G, int m, int cs) {
  const int L = G.L[m], rwords = (L + 7) / 8, line = L + cs; const size_t n = G.n;
  G.packed[m].assign(n * rwords, 0); if (cs) G.ibp[m].assign(n, 0);
  std::atomic<int> bad_rc(GM_OK); std::mutex em; std::string emsg;
  const char* base = G.seqs[m].data(); uint32_t* pk = G.packed[m].data(); uint8_t* ib = cs ? G.ibp[m].data() : nullptr;
  gm_parallel_for(n, 8192, [&](size_t b0, size_t e0) {
    for (size_t i = b0; i < e0 && bad_rc.load(std::memory_order_relaxed) == GM_OK; i++) {
      int b = 0; const int r2 = gm_sequence_to_bitfield(cs, base + i * ((size_t)line + 1), line, pk + i * rwords, &b);
      if (r2) { std::lock_guard<std::mutex> lk(em); if (bad_rc == GM_OK) { bad_rc = r2; emsg = gm_last_error(); } return; }
      if (cs) ib[i] = (uint8_t)b;
    }
  });
  if (bad_rc != GM_OK) { gm_set_error("%s", emsg.c_str()); return bad_rc; }
  return GM_OK;
}
// the group of a read / pair by its length(s); the last one found first (files of one read length never look anything up)
struct GroupIndex {
  std::unordered_map<uint64_t, uint32_t> idx; uint64_t last_key = ~0ull; uint32_t last = 0;
  uint32_t find(ReadChunk& C, int L1, int L2) {
    const uint64_t key = ((uint64_t)(uint32_t)L1 << 32) | (uint32_t)L2;
    if (key == last_key) return last;
    auto it = idx.find(key);
    if (it == idx.end()) { it = idx.emplace(key, (uint32_t)C.groups.size()).first; C.groups.emplace_back(); C.groups.back().L[0] = L1; C.groups.back().L[1] = L2; }
    last_key = key; last = it->second; return last;
  }
};

// The reader thread runs up to two chunks ahead of the mapping thread (round 4: with one chunk of look-ahead and chunk sizes that doubled, reading chunk k + 1 took longer than
// mapping chunk k whenever the reader is not twice as fast as the device).  Chunk sizes: 2^17, 2^19, then chunk_reads -- few, large mapping calls.
struct ChunkFeed {
  std::mutex m; std::condition_variable cv; std::deque<ReadChunk> q; bool stop = false; std::thread th;
  template <class Load> void start(Load load) {
    th = std::thread([this, load]() mutable {
      for (;;) {
        ReadChunk C;
        try { C = load(); } catch (const std::exception& e) { C = ReadChunk(); C.rc = GM_E_NOMEM; C.err = std::string("reader thread: ") + e.what(); }      // (no exception leaves the thread)
        const bool last = C.last || C.rc != GM_OK;
        { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return q.size() < 2 || stop; }); if (stop) return; q.push_back(std::move(C)); }
        cv.notify_all();
        if (last) return;
      }
    });
  }
  ReadChunk take() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return !q.empty(); }); ReadChunk C = std::move(q.front()); q.pop_front(); lk.unlock(); cv.notify_all(); return C; }
  ~ChunkFeed() { { std::lock_guard<std::mutex> lk(m); stop = true; } cv.notify_all(); if (th.joinable()) th.join(); }
};
static size_t gm_next_chunk_size(size_t cur, size_t cap) { return std::min(cap, cur * 4); }      // 2^17, 2^19, then chunk_reads: every mapping call pays ~25 ms of pipeline fill and drain

// ---- unpaired -------------------------------------------------------------------------------------------------------------------------------------
static int map_reads_file_cb_impl(gm_session_t* s, const char* path, int fastq, int qual_delta, size_t chunk_reads, gm_write_fn write, void* ctx, gm_map_stats_t* stats) {
  if (!s || !path || !write) { gm_set_error("gm_map_reads_file_cb: bad arguments"); return GM_E_ARG; }
  const int cs = s->P.colour_space ? 1 : 0;
  if (cs && s->P.trim_front > 0) { gm_set_error("trim_front cannot be used in colour space (ref: gmapper.c:2134-2137)"); return GM_E_ARG; }
  if (chunk_reads == 0) chunk_reads = 1u << 20;
  ReadsFile F; int rc = F.open(path, cs, fastq); if (rc) return rc;
  if (cs && F.fastq && (s->P.trim_front > 0 || s->P.trim_end > 0)) { gm_set_error("colour space: trimming reads that carry quality values is not supported (the reference leaves one quality value too many, ref: gmapper.c:262-284)"); return GM_E_ARG; }
  if (cs && F.fastq && s->P.ignore_qvs) { gm_set_error("ignore_qvs is implemented for letter space only (colour space: sw_full_cs and post_sw without the reads' quality values, ref: gmapper.c:532,2962)"); return GM_E_ARG; }
  const gm_params_t P = s->P; const bool is_fastq = F.fastq;
  // (the first chunk is small: nothing overlaps the reading of the first one)
  size_t this_chunk = std::min<size_t>(chunk_reads, 1u << 17);
  FileRead R;                                                     // (one set of strings for every read: they keep their capacity)
  auto load = [&F, &R, P, is_fastq, qual_delta, chunk_reads, cs, &this_chunk]() -> ReadChunk {
    ReadChunk C; GroupIndex GI;
    const size_t want = this_chunk; this_chunk = gm_next_chunk_size(this_chunk, chunk_reads);
    C.group_of.reserve(want);
    while (C.group_of.size() < want) {
      const int g = F.next(R);
      if (g < 0) { C.rc = g; C.err = gm_last_error(); return C; }
      if (g == 0) { C.last = true; break; }
      bool drop = false;
      const int rc2 = gm_preprocess_read(P, is_fastq, qual_delta, 0, R.seq, R.qual, R.name, &drop);
      if (rc2) { C.rc = rc2; C.err = gm_last_error(); return C; }
      if (drop) continue;
      const uint32_t gi = GI.find(C, (int)R.seq.size() - cs, 0);
      ReadGroup& G = C.groups[gi];
      G.seqs[0] += R.seq; G.seqs[0] += '\n'; G.names[0] += R.name; G.names[0] += '\n'; if (is_fastq) { G.quals[0] += R.qual; G.quals[0] += '\n'; }
      G.n++; C.group_of.push_back(gi);
    }
    for (ReadGroup& G : C.groups) { const int rc3 = gm_pack_group(G, 0, cs); if (rc3) { C.rc = rc3; C.err = gm_last_error(); return C; } }
    return C;
  };
  ChunkFeed feed; feed.start(load);                                  // (its destructor stops and joins the reader on every way out)
  // One chunk: its groups through map_impl, the records back in the file's order -- either the single group's own buffer (*single, released by the caller) or `out`.
  auto map_chunk = [cs, is_fastq, qual_delta](gm_session* ss, ReadChunk& C, gm_map_stats_t& sum, std::string& out, char** single, size_t* single_len) -> int {
    const size_t ng = C.groups.size();
    std::vector<char*> gsam(ng, nullptr); std::vector<size_t> glen(ng, 0); std::vector<std::vector<uint32_t>> gbytes(ng);
    auto cleanup = [&]() { for (char*& p : gsam) { gm_release_group_text(p); p = nullptr; } };
    for (size_t g = 0; g < ng; g++) {
      ReadGroup& G = C.groups[g];
      gbytes[g].assign(G.n, 0);
      gm_map_stats_t st;
      const int rc = map_impl(ss, (int)G.n, G.L[0], G.packed[0].data(), nullptr, G.names[0].c_str(), 1, &gsam[g], &glen[g], &st, cs ? G.ibp[0].data() : nullptr, is_fastq ? G.quals[0].c_str() : nullptr, qual_delta,
                              G.seqs[0].c_str(), gbytes[g].data());
      if (rc) { cleanup(); return rc; }
      gm_stats_add(sum, st);
    }
    if (ng == 1) { *single = gsam[0]; *single_len = glen[0]; gsam[0] = nullptr; }
    else if (ng > 1) {
      size_t tot = 0; for (size_t g = 0; g < ng; g++) tot += glen[g];
      out.reserve(tot);
      std::vector<size_t> cur(ng, 0), nxt(ng, 0);
      for (const uint32_t g : C.group_of) { const uint32_t b = gbytes[g][nxt[g]++]; out.append(gsam[g] + cur[g], b); cur[g] += b; }
    }
    cleanup();
    return GM_OK;
  };
  // The chunks go alternately to this session and to its twin (made when the file turns out to hold more than one chunk), each mapped by a thread of its own: a mapping call
  // ends with a tail -- the last sub-batch's SW passes and the host's text work, ~30 ms with nothing on the lookup stream -- and with two calls in flight (GmDevTurn admits
  // two per device; each session owns its launch scratch) that tail runs under the other chunk's lookups.  Tickets keep the order: chunk t is written when chunks
  // 0 .. t - 1 have been.
  struct Shared { std::mutex take_m, m; std::condition_variable cv; size_t next_ticket = 0, write_turn = 0; bool done = false; int rc = GM_OK; std::string err; gm_map_stats_t total; } S;
  memset(&S.total, 0, sizeof S.total);
  std::thread helper;
  std::function<void(gm_session*, bool)> worker = [&](gm_session* ss, bool is_caller) {
    for (;;) {
      ReadChunk C; size_t ticket;
      { std::lock_guard<std::mutex> lk(S.take_m);
        if (S.done) return;
        C = feed.take();                                               // the next chunks are read, preprocessed, grouped and packed while this one is mapped
        ticket = S.next_ticket++;
        if (C.last || C.rc) S.done = true; }
      // the first chunk is not the last one: the twin session and its thread start now (a session that cannot be made -- memory -- is no error: one thread maps every chunk)
      if (is_caller && ticket == 0 && !C.last && !C.rc && !getenv("GM_FILE_ONE_SESSION")) {
        if (!s->twin) { gm_session_t* tw = nullptr; if (gm_session_create(&tw, s->ix, &s->P, s->max_batch) == GM_OK) s->twin = tw; }
        if (s->twin) { try { helper = std::thread(worker, s->twin, false); } catch (...) {} }
      }
      int my_rc = C.rc; std::string my_err = C.err;
      gm_map_stats_t sum; memset(&sum, 0, sizeof sum);
      std::string out; char* single = nullptr; size_t single_len = 0; bool stop = false;
      if (!my_rc) {
        try { my_rc = map_chunk(ss, C, sum, out, &single, &single_len); if (my_rc) my_err = gm_last_error(); }
        catch (const std::exception& e) { my_rc = GM_E_NOMEM; my_err = std::string("gm_map_reads_file_cb: ") + e.what(); }
      }
      { std::unique_lock<std::mutex> lk(S.m);
        S.cv.wait(lk, [&] { return S.write_turn == ticket; });
        if (S.rc == GM_OK && my_rc != GM_OK) { S.rc = my_rc; S.err = my_err; }
        if (S.rc == GM_OK) {
          const char* p = single ? single : out.data(); const size_t n = single ? single_len : out.size();
          if (n && write(ctx, p, n)) { S.rc = GM_E_ARG; S.err = "gm_map_reads_file_cb: the write function asked to stop"; }
          gm_stats_add(S.total, sum);
        }
        S.write_turn++; stop = S.rc != GM_OK; }
      S.cv.notify_all();
      gm_release_group_text(single);
      if (stop) { std::lock_guard<std::mutex> lk(S.take_m); S.done = true; }
    }
  };
  worker(s, true);
  if (helper.joinable()) helper.join();
  if (S.rc) { gm_set_error("%s", S.err.c_str()); return S.rc; }
  const gm_map_stats_t total = S.total;
  if (stats) *stats = total;
  return GM_OK;
}

// (no C++ exception crosses the C ABI: a failed thread start or allocation in the streaming entries comes back as an error code)
extern "C" int gm_map_reads_file_cb(gm_session_t* s, const char* path, int fastq, int qual_delta, size_t chunk_reads, gm_write_fn write, void* ctx, gm_map_stats_t* stats) {
  try { return map_reads_file_cb_impl(s, path, fastq, qual_delta, chunk_reads, write, ctx, stats); }
  catch (const std::bad_alloc&) { gm_set_error("gm_map_reads_file_cb: out of memory"); return GM_E_NOMEM; }
  catch (const std::exception& e) { gm_set_error("gm_map_reads_file_cb: %s", e.what()); return GM_E_ARG; }
}
struct GmTextSink { std::string text; };
static int gm_sink_append(void* ctx, const char* p, size_t n) { ((GmTextSink*)ctx)->text.append(p, n); return 0; }
static int gm_sink_to_caller(GmTextSink& K, char** sam, size_t* sam_len, const char* who) {
  char* outp = (char*)malloc(K.text.size() + 1); if (!outp) { gm_set_error("%s: out of memory", who); return GM_E_NOMEM; }
  memcpy(outp, K.text.data(), K.text.size()); outp[K.text.size()] = 0; *sam = outp; *sam_len = K.text.size();
  return GM_OK;
}
// the whole text in one buffer (small files; gm_free releases it): the callback form with a collecting write function
extern "C" int gm_map_reads_file(gm_session_t* s, const char* path, int fastq, int qual_delta, char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (!s || !path || !sam || !sam_len) { gm_set_error("gm_map_reads_file: bad arguments"); return GM_E_ARG; }
  *sam = nullptr; *sam_len = 0;
  GmTextSink K;
  const int rc = gm_map_reads_file_cb(s, path, fastq, qual_delta, 0, gm_sink_append, &K, stats);
  if (rc) return rc;
  return gm_sink_to_caller(K, sam, sam_len, "gm_map_reads_file");
}

// ---- pairs: `gmapper -1 a.fq -2 b.fq`, or one file with the mates adjacent (ref: gmapper.c:363-398 the two readers, :406-411,503-520 a pair is dropped whole) ----
static int map_pairs_file_cb_impl(gm_session_t* s, const char* path1, const char* path2, int fastq, int qual_delta, const gm_pair_opts_t* opts, size_t chunk_pairs,
                                  gm_write_fn write, void* ctx, gm_map_stats_t* stats) {
  if (!s || !path1 || !write) { gm_set_error("gm_map_pairs_file_cb: bad arguments"); return GM_E_ARG; }
  const int cs = s->P.colour_space ? 1 : 0;
  int rc = gm_check_pair_trim(s->P); if (rc) return rc;
  if (cs && s->P.trim_front > 0) { gm_set_error("trim_front cannot be used in colour space (ref: gmapper.c:2134-2137)"); return GM_E_ARG; }
  if (chunk_pairs == 0) chunk_pairs = 1u << 19;
  ReadsFile F1, F2;
  rc = F1.open(path1, cs, fastq); if (rc) return rc;
  if (path2) { rc = F2.open(path2, cs, fastq); if (rc) return rc; if (F1.fastq != F2.fastq) { gm_set_error("gm_map_pairs_file: one FASTA and one FASTQ file"); return GM_E_ARG; } }
  if (cs && F1.fastq && (s->P.trim_front > 0 || s->P.trim_end > 0)) { gm_set_error("colour space: trimming reads that carry quality values is not supported (ref: gmapper.c:262-284)"); return GM_E_ARG; }
  if (cs && F1.fastq && s->P.ignore_qvs) { gm_set_error("ignore_qvs is implemented for letter space only (ref: gmapper.c:532,2962)"); return GM_E_ARG; }
  const gm_params_t P = s->P; const bool is_fastq = F1.fastq, two = path2 != nullptr;
  size_t this_chunk = std::min<size_t>(chunk_pairs, 1u << 16);
  FileRead A, B;
  auto load = [&F1, &F2, &A, &B, P, is_fastq, qual_delta, chunk_pairs, two, cs, &this_chunk]() -> ReadChunk {
    ReadChunk C; GroupIndex GI;
    const size_t want = this_chunk; this_chunk = gm_next_chunk_size(this_chunk, chunk_pairs);
    C.group_of.reserve(want);
    while (C.group_of.size() < want) {
      const int g1 = F1.next(A); if (g1 < 0) { C.rc = g1; C.err = gm_last_error(); return C; }
      if (g1 == 0) { C.last = true; break; }
      const int g2 = two ? F2.next(B) : F1.next(B); if (g2 < 0) { C.rc = g2; C.err = gm_last_error(); return C; }
      if (g2 == 0) { C.last = true; break; }                            // an odd read at the end has no mate
      bool d1 = false, d2 = false;
      int rc2 = gm_preprocess_read(P, is_fastq, qual_delta, 1, A.seq, A.qual, A.name, &d1);
      if (!rc2 && !d1) rc2 = gm_preprocess_read(P, is_fastq, qual_delta, 2, B.seq, B.qual, B.name, &d2);        // (the mate of an ignored first read is not looked at, ref: gmapper.c:406-411)
      if (rc2) { C.rc = rc2; C.err = gm_last_error(); return C; }
      if (d1 || d2) continue;                                            // a pair is dropped whole (ref: gmapper.c:503-520)
      const uint32_t gi = GI.find(C, (int)A.seq.size() - cs, (int)B.seq.size() - cs);
      ReadGroup& G = C.groups[gi];
      const FileRead* M[2] = {&A, &B};
      for (int m = 0; m < 2; m++) { G.seqs[m] += M[m]->seq; G.seqs[m] += '\n'; G.names[m] += M[m]->name; G.names[m] += '\n'; if (is_fastq) { G.quals[m] += M[m]->qual; G.quals[m] += '\n'; } }
      G.n++; C.group_of.push_back(gi);
    }
    for (ReadGroup& G : C.groups) for (int m = 0; m < 2; m++) { const int rc3 = gm_pack_group(G, m, cs); if (rc3) { C.rc = rc3; C.err = gm_last_error(); return C; } }
    return C;
  };
  gm_map_stats_t total; memset(&total, 0, sizeof total);
  ChunkFeed feed; feed.start(load);
  for (;;) {
    ReadChunk C = feed.take();
    if (C.rc) { gm_set_error("%s", C.err.c_str()); return C.rc; }
    const size_t ng = C.groups.size();
    std::vector<char*> gsam(ng, nullptr); std::vector<size_t> glen(ng, 0); std::vector<std::vector<uint32_t>> gbytes(ng);
    auto cleanup = [&]() { for (char*& p : gsam) { gm_release_group_text(p); p = nullptr; } };
    auto fail = [&](int e) { cleanup(); return e; };
    for (size_t g = 0; g < ng; g++) {
      ReadGroup& G = C.groups[g];
      gbytes[g].assign(G.n, 0);
      gm_map_stats_t st;
      rc = map_pairs_impl(s, (int)G.n, G.L[0], G.packed[0].data(), G.L[1], G.packed[1].data(), G.names[0].c_str(), G.names[1].c_str(), opts, &gsam[g], &glen[g], &st,
                          is_fastq ? G.quals[0].c_str() : nullptr, is_fastq ? G.quals[1].c_str() : nullptr, qual_delta, cs ? G.ibp[0].data() : nullptr, cs ? G.ibp[1].data() : nullptr, gbytes[g].data());
      if (rc) return fail(rc);
      gm_stats_add(total, st);
    }
    if (ng == 1) { if (glen[0] && write(ctx, gsam[0], glen[0])) { gm_set_error("gm_map_pairs_file_cb: the write function asked to stop"); return fail(GM_E_ARG); } }
    else if (ng > 1) {
      std::string out; std::vector<size_t> cur(ng, 0), nxt(ng, 0);
      for (const uint32_t g : C.group_of) { const uint32_t b = gbytes[g][nxt[g]++]; out.append(gsam[g] + cur[g], b); cur[g] += b; }
      if (!out.empty() && write(ctx, out.data(), out.size())) { gm_set_error("gm_map_pairs_file_cb: the write function asked to stop"); return fail(GM_E_ARG); }
    }
    cleanup();
    if (C.last) break;
  }
  if (stats) *stats = total;
  return GM_OK;
}
extern "C" int gm_map_pairs_file_cb(gm_session_t* s, const char* path1, const char* path2, int fastq, int qual_delta, const gm_pair_opts_t* opts, size_t chunk_pairs,
                                    gm_write_fn write, void* ctx, gm_map_stats_t* stats) {
  try { return map_pairs_file_cb_impl(s, path1, path2, fastq, qual_delta, opts, chunk_pairs, write, ctx, stats); }
  catch (const std::bad_alloc&) { gm_set_error("gm_map_pairs_file_cb: out of memory"); return GM_E_NOMEM; }
  catch (const std::exception& e) { gm_set_error("gm_map_pairs_file_cb: %s", e.what()); return GM_E_ARG; }
}
extern "C" int gm_map_pairs_file(gm_session_t* s, const char* path1, const char* path2, int fastq, int qual_delta, const gm_pair_opts_t* opts,
                                 char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (!s || !path1 || !sam || !sam_len) { gm_set_error("gm_map_pairs_file: bad arguments"); return GM_E_ARG; }
  *sam = nullptr; *sam_len = 0;
  GmTextSink K;
  const int rc = gm_map_pairs_file_cb(s, path1, path2, fastq, qual_delta, opts, 0, gm_sink_append, &K, stats);
  if (rc) return rc;
  return gm_sink_to_caller(K, sam, sam_len, "gm_map_pairs_file");
}

// the preprocessing by itself (host only, no device): what the file entries do to one read before they map it.  seq / qual are edited in place (NUL-terminated, qual may be
// NULL for FASTA input); *drop = 1 when the read gets no record.  mate: 0 unpaired, 1 / 2 the mates of a pair.
extern "C" int gm_preprocess_read_text(const gm_params_t* params, int mate, char* seq, char* qual, int qual_delta, int* drop) {
  if (!params || !seq || !drop || mate < 0 || mate > 2) { gm_set_error("gm_preprocess_read_text: bad arguments"); return GM_E_ARG; }
  if (mate) { const int rc = gm_check_pair_trim(*params); if (rc) return rc; }
  std::string sq(seq), ql(qual ? qual : ""); bool d = false;
  const int rc = gm_preprocess_read(*params, qual != nullptr, qual_delta, mate, sq, ql, std::string("?"), &d);
  if (rc) return rc;
  memcpy(seq, sq.c_str(), sq.size() + 1); if (qual) memcpy(qual, ql.c_str(), ql.size() + 1);
  *drop = d ? 1 : 0;
  return GM_OK;
}
