// gm_index_io.inc -- the reference's on-disk index ("-S prefix" / "-L prefix"); included by gm_host.hip.
//   save_genome_map_seed / load_genome_map_seed   ref: gmapper/genome.c:15-176
//   save_genome_map / load_genome_map             ref: gmapper/genome.c:179-270,670-831
// Files: <prefix>.genome and <prefix>.seed.<n>, gzip streams of little-endian words:
//   .seed.n : u32 shrimp_mode (1 = letter space, 2 = colour space), u32 Hflag, seed_type {u64 mask, i32 span, i32 weight},
//             u32 lens[4^weight], u32 total, u32 positions[total]      (no `capacity` word, despite the reference's comment)
//   .genome : u32 mode, u32 Hflag, u32 num_contigs, u32 genome_len[], u32 contig_offsets[], {u32 namelen, name + NUL}...,
//             u32 total_words, forward bitfields, reverse-complement bitfields, in colour space also the colour bitfields
//             (genome_cs_contigs; the reference derives genome_cs_contigs_rc on load, ref: genome.c:757-770)
// so that an index built here can be handed to stock gmapper and vice versa.
#include <zlib.h>

static bool gz_put(gzFile f, const void* p, size_t n) {
  const char* c = (const char*)p;
  while (n) { const unsigned k = (unsigned)std::min<size_t>(n, 1u << 30); if (gzwrite(f, c, k) != (int)k) return false; c += k; n -= k; }
  return true;
}
static bool gz_get(gzFile f, void* p, size_t n) {
  char* c = (char*)p;
  while (n) { const unsigned k = (unsigned)std::min<size_t>(n, 1u << 30); if (gzread(f, c, k) != (int)k) return false; c += k; n -= k; }
  return true;
}

extern "C" int gm_index_save(const gm_index_t* ix, const char* prefix) {
  if (!ix || !prefix) return GM_E_ARG;
  GM_HIP(hipSetDevice(ix->device));
  { const int rc = gm_index_derive_rna(const_cast<gm_index*>(ix), nullptr); if (rc) return rc; }
  const uint32_t mode = ix->params.colour_space ? 2 : 1, hflag = ix->params.hash_seeds ? 1 : 0;   // shrimp_mode_t, ref: gmapper-definitions.h:31-32
  // ---- .genome ----
  std::vector<uint32_t> g(ix->genome_words);
  GM_HIP(hipMemcpy(g.data(), ix->d_genome, ix->genome_words * 4, hipMemcpyDeviceToHost));
  const std::string gname = std::string(prefix) + ".genome";
  gzFile fp = gzopen(gname.c_str(), "wb");
  if (!fp) { gm_set_error("cannot write %s", gname.c_str()); return GM_E_ARG; }
  bool ok = gz_put(fp, &mode, 4) && gz_put(fp, &hflag, 4);
  const uint32_t nc = (uint32_t)ix->n_contigs;
  ok = ok && gz_put(fp, &nc, 4);
  std::vector<uint32_t> lens(nc);
  for (uint32_t c = 0; c < nc; c++) lens[c] = ix->contig_off[c + 1] - ix->contig_off[c];
  ok = ok && gz_put(fp, lens.data(), nc * 4) && gz_put(fp, ix->contig_off.data(), nc * 4);
  uint32_t total = 0;
  for (uint32_t c = 0; c < nc; c++) {
    const uint32_t nl = (uint32_t)ix->names[c].size();
    ok = ok && gz_put(fp, &nl, 4) && gz_put(fp, ix->names[c].c_str(), nl + 1);
    total += (lens[c] + 7) / 8;
  }
  ok = ok && gz_put(fp, &total, 4);
  auto code_at = [&](uint64_t p) { return (g[p >> 3] >> ((p & 7) * 4)) & 0xfu; };
  static const uint8_t COMPL[16] = {3, 2, 1, 0, 0, 10, 9, 7, 8, 6, 5, 14, 13, 12, 11, 15};   // complement_base, ref: util.h:125-151 (same table as the kernels' 0xFBCDE56879A00123)
  for (int strand = 0; strand < 2 && ok; strand++)
    for (uint32_t c = 0; c < nc && ok; c++) {
      std::vector<uint32_t> w((lens[c] + 7) / 8, 0);
      const uint64_t off = ix->contig_off[c];
      for (uint32_t i = 0; i < lens[c]; i++) {
        uint32_t code = strand == 0 ? code_at(off + i) : COMPL[code_at(off + lens[c] - 1 - i)];
        if (strand == 1 && code == 3u && ix->rna_ready && ix->contig_rna[c]) code = 4u;      // an RNA contig's reverse complement holds U for A (ref: util.h:150, genome.c:1107)
        w[i >> 3] |= code << ((i & 7) * 4);
      }
      ok = gz_put(fp, w.data(), w.size() * 4);
    }
  if (ix->params.colour_space && ok) {   // genome_cs_contigs, ref: genome.c:259-263
    std::vector<uint32_t> gc(ix->genome_words);
    GM_HIP(hipMemcpy(gc.data(), ix->d_genome_cs, ix->genome_words * 4, hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < nc && ok; c++) {
      std::vector<uint32_t> w((lens[c] + 7) / 8, 0);
      const uint64_t off = ix->contig_off[c];
      for (uint32_t i = 0; i < lens[c]; i++) { const uint64_t p2 = off + i; w[i >> 3] |= ((gc[p2 >> 3] >> ((p2 & 7) * 4)) & 0xfu) << ((i & 7) * 4); }
      ok = gz_put(fp, w.data(), w.size() * 4);
    }
  }
  if (gzclose(fp) != Z_OK) ok = false;
  if (!ok) { gm_set_error("write error on %s", gname.c_str()); return GM_E_ARG; }
  // ---- .seed.n ----
  for (int sn = 0; sn < ix->n_seeds; sn++) {
    const GmSeedHost& sd = ix->seeds[sn];
    const uint64_t K = 1ull << sd.kbits; const int S = ix->n_slabs;
    std::vector<uint32_t> dir(sd.dir_words), pos(sd.n_pos);
    GM_HIP(hipMemcpy(dir.data(), sd.d_dir, sd.dir_words * 4, hipMemcpyDeviceToHost));
    if (sd.n_pos) GM_HIP(hipMemcpy(pos.data(), sd.d_pos, (size_t)sd.n_pos * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> ll(K);
    for (uint64_t k = 0; k < K; k++) ll[k] = dir[(k + 1) * S] - dir[k * S];
    const std::string sname = std::string(prefix) + ".seed." + std::to_string(sn);
    fp = gzopen(sname.c_str(), "wb");
    if (!fp) { gm_set_error("cannot write %s", sname.c_str()); return GM_E_ARG; }
    struct { uint64_t mask; int32_t span, weight; } st = {sd.mask, sd.span, sd.weight};
    const uint32_t tot = sd.n_pos;
    ok = gz_put(fp, &mode, 4) && gz_put(fp, &hflag, 4) && gz_put(fp, &st, 16) && gz_put(fp, ll.data(), K * 4) && gz_put(fp, &tot, 4) &&
         gz_put(fp, pos.data(), (size_t)tot * 4);
    if (gzclose(fp) != Z_OK) ok = false;
    if (!ok) { gm_set_error("write error on %s", sname.c_str()); return GM_E_ARG; }
  }
  return GM_OK;
}

extern "C" int gm_index_load(gm_index_t** out, int device, const char* prefix, const gm_params_t* params) {
  if (!out || !prefix) return GM_E_ARG;
  if (gm_device_count() <= device) { gm_set_error("no HIP device %d (the seed index lives in HBM; there is no CPU path)", device); return GM_E_NODEVICE; }
  GM_HIP(hipSetDevice(device));
  const std::string gname = std::string(prefix) + ".genome";
  gzFile fp = gzopen(gname.c_str(), "rb");
  if (!fp) { gm_set_error("cannot open %s", gname.c_str()); return GM_E_ARG; }
  uint32_t mode = 0, hflag = 0, nc = 0;
  bool ok = gz_get(fp, &mode, 4) && gz_get(fp, &hflag, 4) && gz_get(fp, &nc, 4);
  const uint32_t want_mode = (params && params->colour_space) ? 2u : 1u;
  const uint32_t want_h = (params && params->hash_seeds) ? 1u : 0u;
  if (!ok || mode != want_mode || hflag != want_h || nc == 0) {
    gzclose(fp); gm_set_error("%s: not a gmapper index of the requested mode (mode %u, wanted %u; Hflag %u, wanted %u)", gname.c_str(), mode, want_mode, hflag, want_h); return GM_E_ARG;   // ref: genome.c:705-715
  }
  { const int rc = gm_refuse_contig_count("gm_index_load", nc); if (rc != GM_OK) { gzclose(fp); return rc; } }
  std::vector<uint32_t> lens(nc), offs(nc);
  ok = gz_get(fp, lens.data(), nc * 4) && gz_get(fp, offs.data(), nc * 4);
  std::vector<std::string> names(nc);
  for (uint32_t c = 0; c < nc && ok; c++) {
    uint32_t nl = 0; ok = gz_get(fp, &nl, 4) && nl < (1u << 20);
    if (ok) { std::vector<char> b(nl + 1); ok = gz_get(fp, b.data(), nl + 1); names[c].assign(b.data(), nl); }
  }
  uint32_t total = 0; ok = ok && gz_get(fp, &total, 4);
  std::vector<std::vector<uint32_t>> fwd(nc);
  uint64_t chk = 0;
  for (uint32_t c = 0; c < nc && ok; c++) { fwd[c].resize((lens[c] + 7) / 8); chk += fwd[c].size(); ok = gz_get(fp, fwd[c].data(), fwd[c].size() * 4); }
  gzclose(fp);   // the reverse-complement (and colour) copies that follow are not needed: windows are reverse-complemented on load, colours re-derived on the device
  if (!ok || chk != total) { gm_set_error("%s: truncated or inconsistent", gname.c_str()); return GM_E_ARG; }
  gm_index* ix = new gm_index();
  ix->device = device;
  if (params) ix->params = *params; else gm_params_default(&ix->params);
  // seeds first (the cutoff depends on their weights)
  struct SeedFile { std::vector<uint32_t> lens, pos; };
  std::vector<SeedFile> sf;
  for (int sn = 0; sn < GM_MAX_SEEDS; sn++) {
    const std::string sname = std::string(prefix) + ".seed." + std::to_string(sn);
    fp = gzopen(sname.c_str(), "rb");
    if (!fp) break;
    struct { uint64_t mask; int32_t span, weight; } st;
    uint32_t m2 = 0, h2 = 0;
    ok = gz_get(fp, &m2, 4) && gz_get(fp, &h2, 4) && gz_get(fp, &st, 16) && m2 == want_mode && h2 == want_h && st.span >= 1;
    if (ok && st.span > 32) {   // (the reference writes spans up to 64; its mask does not say what lies above bit 63, so the seed is named by its number)
      gzclose(fp); delete ix; gm_set_error("%s: seed %d: span %d, the limit is 32 (the k-mer key is gathered through a 64-bit mask)", sname.c_str(), sn, (int)st.span); return GM_E_ARG;
    }
    std::string text;
    if (ok) for (int i = st.span - 1; i >= 0; i--) text.push_back(((st.mask >> i) & 1) ? '1' : '0');   // first character = highest bit (ref: seeds.c:9-43)
    if (ok && add_seed(ix, text.c_str()) != GM_OK) {      // weight above 14 without -H: the limit's own text, behind the file's name
      const std::string why = gm_last_error(); gzclose(fp); delete ix; gm_set_error("%s: %s", sname.c_str(), why.c_str()); return GM_E_ARG;
    }
    ok = ok && ix->seeds[ix->n_seeds - 1].weight == st.weight;
    SeedFile f;
    if (ok) {
      const uint64_t K = 1ull << ix->seeds[ix->n_seeds - 1].kbits;     // capacity, ref: genome.c:141
      f.lens.resize(K); uint32_t tot = 0;
      ok = gz_get(fp, f.lens.data(), K * 4) && gz_get(fp, &tot, 4);
      if (ok) { f.pos.resize(tot); ok = gz_get(fp, f.pos.data(), (size_t)tot * 4); }
    }
    gzclose(fp);
    if (!ok) { delete ix; gm_set_error("%s: truncated or not a seed file of the requested mode", sname.c_str()); return GM_E_ARG; }
    sf.push_back(std::move(f));
  }
  { const std::string sname = std::string(prefix) + ".seed." + std::to_string(GM_MAX_SEEDS);
    if ((fp = gzopen(sname.c_str(), "rb"))) { gzclose(fp); delete ix; gm_set_error("%s: more than %d seeds (GM_MAX_SEEDS)", sname.c_str(), GM_MAX_SEEDS); return GM_E_ARG; } }
  if (sf.empty()) { delete ix; gm_set_error("%s.seed.0 not found", prefix); return GM_E_ARG; }
  std::vector<const uint32_t*> cptr(nc); std::vector<const char*> nptr(nc);
  for (uint32_t c = 0; c < nc; c++) { cptr[c] = fwd[c].data(); nptr[c] = names[c].c_str(); }
  int rc = index_prepare(ix, (int)nc, cptr.data(), lens.data(), nptr.data());
  if (rc == GM_OK && ix->params.colour_space) rc = gm_index_colour_genome_device(ix, nullptr);
  for (uint32_t c = 0; c < nc && rc == GM_OK; c++) if (offs[c] != ix->contig_off[c]) { gm_set_error("%s: contig offsets are not cumulative", gname.c_str()); rc = GM_E_ARG; }
  for (int sn = 0; sn < ix->n_seeds && rc == GM_OK; sn++)
    rc = gm_index_from_lists_device(ix, sn, sf[sn].lens.data(), sf[sn].pos.data(), (uint32_t)sf[sn].pos.size());
  if (rc != GM_OK) { gm_index_free(ix); return rc; }
  *out = ix;
  return GM_OK;
}
