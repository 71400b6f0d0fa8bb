// gm_host.hip -- host side of libgmapper_hip.so: handles, batching, and the part of the per-read
// pipeline the reference keeps on the CPU next to its output code:
//   hit_run_post_sw (LS)            ref: gmapper/mapping.c:1609-1625
//   read_pass2 selection + dedup    ref: gmapper/mapping.c:1520-1606,1661-1750
//   compute_unpaired_mqv            ref: gmapper/output.c:777-793
//   hit_output (SAM record)         ref: gmapper/output.c:227-774, make_cigar :15-64
// No CPU fallback exists for the device stages: without a HIP device every entry point fails.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <mutex>
#include <optional>
#include <condition_variable>
#include <deque>
#include <functional>
#include <future>
#include <map>
#include <unordered_map>
#include <zlib.h>
#include "gm_common.h"
#include "gm_internal.h"
#include "gm_devmem.h"
#include "gm_textout.h"

// ---- errors -----------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void gm_set_error(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}
extern "C" const char* gm_last_error(void) { return g_err; }
extern "C" int gm_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
hipError_t gm_lds_at_least(const void* kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return hipSuccess;
  int dev = 0; hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  static std::mutex m; static std::map<std::pair<int, const void*>, size_t> raised;     // (device, kernel) -> the limit set there so far
  std::lock_guard<std::mutex> lk(m);
  size_t& cur = raised[{dev, kernel}];
  if (bytes <= cur) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) cur = bytes;
  return e;
}
static GmTextCacheT<> g_outcache;      // the text buffer parked between calls (gm_textout.h; gm_release_cache() drops it)
static void gm_text_pool_drop();
extern "C" void gm_release_cache(void) { g_outcache.drop(); gm_text_pool_drop(); }
extern "C" void gm_free(void* p) { if (p) g_outcache.give_back(p); }

extern "C" void gm_params_default(gm_params_t* p) {
  memset(p, 0, sizeof *p);
  p->match_score = 10; p->mismatch_score = -15;
  p->a_gap_open_score = -33; p->a_gap_extend_score = -7; p->b_gap_open_score = -33; p->b_gap_extend_score = -3;
  p->window_len = 140.0; p->window_overlap = 90.0; p->window_gen_threshold = 55.0;
  p->sw_vect_threshold = 50.0; p->sw_full_threshold = 50.0;     // LS: vect := full (ref: gmapper.c:2456-2458)
  p->match_mode = 2; p->num_outputs = 10; p->num_tmp_outputs = 30; p->anchor_width = 8;
  p->region_bits = 11; p->region_overlap = 50; p->list_cutoff = 0; p->hash_filter_calls = 1; p->tiebreak_rev = 1;
  p->sam_unaligned = 0; p->longest_read_len = 1000; p->strata = 0; p->max_alignments = 0;
  p->colour_space = 0; p->crossover_score = -20; p->indel_taboo_len = 0; p->pr_xover = 0.03; p->local_alignment = 0; p->ungapped = 0; p->hash_seeds = 0; p->output_format = 0; p->print_read_seq = 0; p->strand_only = 0;
  p->single_best_mapping = 0; p->all_contigs = 0; p->no_mapping_qualities = 0; p->no_improper_mappings = 0;
  p->extra_sam_fields = 0; p->sam_r2 = 0; memset(p->read_group, 0, sizeof p->read_group);
  p->trim_front = 0; p->trim_end = 0; p->trim_first = 1; p->trim_second = 1; p->trim_illumina = 0; p->min_avg_qv = 10; p->ignore_qvs = 0; p->no_qv_check = 0;      // ref: gmapper.h:63-67,75,81,104
}
extern "C" int gm_abi_sizeof(int which) {
  switch (which) { case 0: return (int)sizeof(gm_params_t); case 1: return (int)sizeof(gm_pair_opts_t); case 2: return (int)sizeof(gm_map_stats_t); case 3: return (int)sizeof(gm_merge_options_t); case 4: return (int)sizeof(gm_sw_full_rec_t); case 5: return (int)sizeof(gm_post_rec_t); }
  return -1;
}
// compute_mapping_qualities (ref: gmapper.c:2258,2325-2328): off with --no-mapping-qualities and in local mode -- then MAPQ 255, no Z tags, no post_sw (mapping.c:1648)
static inline bool gm_mqv_on(const gm_params_t& P) { return !P.local_alignment && !P.no_mapping_qualities; }
// the gmapper-cs binary's defaults (ref: gmapper.c:1748-1755, gmapper-defaults.h:52-58,64-66)
extern "C" void gm_params_default_cs(gm_params_t* p) {
  gm_params_default(p);
  p->colour_space = 1; p->mismatch_score = -24; p->sw_vect_threshold = 47.0; p->sw_full_threshold = 50.0;
}

static GmScoreDev make_score(const gm_params_t& P) {
  GmScoreDev s; memset(&s, 0, sizeof s);
  s.match = P.match_score;
  s.mismatch = P.colour_space ? P.match_score + P.crossover_score : P.mismatch_score;   // what f1_setup hands the vector filter (ref: gmapper.c:2933-2936)
  s.a_go = -P.a_gap_open_score; s.a_ge = -P.a_gap_extend_score; s.b_go = -P.b_gap_open_score; s.b_ge = -P.b_gap_extend_score;
  s.anchor_width = P.anchor_width; s.match_mode = P.match_mode; s.min_matches = P.match_mode;   // ref: gmapper.c:2625
  s.skip_strands = P.strand_only == 1 ? 2 : (P.strand_only == 2 ? 1 : 0);                       // -F: no strand 1; -C: no strand 0
  s.num_tmp_outputs = P.num_tmp_outputs; s.tiebreak_rev = P.tiebreak_rev; s.hash_filter_calls = P.hash_filter_calls; s.local = P.local_alignment ? 1 : 0; s.gapless = P.ungapped ? 1 : 0;
  auto frac = [](double thr, double* f, int* a) { if (thr < 0) { *f = -1.0; *a = (int)(-thr); } else { *f = thr / 100.0; *a = 0; } };
  frac(P.window_gen_threshold, &s.wgen_thr_frac, &s.wgen_abs);
  frac(P.sw_vect_threshold, &s.vect_thr_frac, &s.vect_abs);
  frac(P.sw_full_threshold, &s.full_thr_frac, &s.full_abs);
  return s;
}

// ---- index ------------------------------------------------------------------------------------
GmIndexDev GmIndexHost::dev_view() const {
  GmIndexDev d; memset(&d, 0, sizeof d);
  d.genome = d_genome; d.genome_cs = d_genome_cs; d.colour = params.colour_space ? 1 : 0; d.hflag = params.hash_seeds ? 1 : 0; d.total_len = total_len; d.n_contigs = n_contigs; d.contig_off = d_contig_off;
  d.contig_rna = d_contig_rna; d.genome_is_rna = genome_is_rna; d.read_rna = nullptr;
  d.n_seeds = n_seeds; d.min_seed_span = min_seed_span; d.max_seed_span = max_seed_span;
  d.slab_bits = slab_bits; d.n_slabs = n_slabs; d.region_bits = params.region_bits; d.region_overlap = params.region_overlap;
  d.list_cutoff = list_cutoff;
  for (int i = 0; i < n_seeds; i++) {
    d.seed[i].mask = seeds[i].mask; d.seed[i].span = seeds[i].span; d.seed[i].weight = seeds[i].weight;
    d.seed[i].dir = seeds[i].d_dir; d.seed[i].pos = seeds[i].d_pos; d.seed[i].bkt = seeds[i].d_bkt; d.seed[i].n_pos = seeds[i].n_pos;
    d.seed[i].sdir = strips_ready ? seeds[i].d_sdir : nullptr; d.seed[i].spos = strips_ready ? seeds[i].d_spos : nullptr;
  }
  return d;
}

// add_spaced_seed, ref: gmapper/seeds.c:9-43.  A refusal names the seed and the limit it broke in gm_last_error() (the limits: include/gmapper_hip.h, beside gm_index_build).
static int add_seed(GmIndexHost* ix, const char* s) {
  if (!s) { gm_set_error("seed %d: no seed string", ix->n_seeds); return GM_E_ARG; }
  const size_t len = strlen(s);
  if (ix->n_seeds >= GM_MAX_SEEDS) { gm_set_error("seed \"%.80s\": more than %d seeds (GM_MAX_SEEDS)", s, GM_MAX_SEEDS); return GM_E_ARG; }
  if (len < 1) { gm_set_error("seed %d: an empty seed", ix->n_seeds); return GM_E_ARG; }
  for (size_t i = 0; i < len; i++)
    if (s[i] != '0' && s[i] != '1') { gm_set_error("seed \"%.80s\": character %zu is neither '0' nor '1'", s, i); return GM_E_ARG; }
  if (len > 32) { gm_set_error("seed \"%.80s\": span %zu, the limit is 32 (the k-mer key is gathered through a 64-bit mask)", s, len); return GM_E_ARG; }
  GmSeedHost sd = ix->seeds[ix->n_seeds];
  sd.mask = 0; sd.span = (int)len; sd.weight = 0; sd.text = s;
  for (int i = 0; i < sd.span; i++) { sd.mask = (sd.mask << 1) | (uint64_t)(s[i] == '1'); sd.weight += (s[i] == '1'); }
  if (sd.weight < 1) { gm_set_error("seed \"%s\": weight 0, a seed needs a 1", s); return GM_E_ARG; }
  if (!ix->params.hash_seeds && sd.weight > 14) {   // MAX_SEED_WEIGHT, ref: gmapper-definitions.h:50, seeds.c:132-136
    gm_set_error("seed \"%s\": weight %d, the limit is 14 without hash_seeds (-H)", s, sd.weight); return GM_E_ARG;
  }
  sd.kbits = ix->params.hash_seeds ? 2 * GM_HASH_TABLE_POWER : 2 * sd.weight;
  ix->seeds[ix->n_seeds] = sd;
  ix->max_seed_span = std::max(ix->max_seed_span, sd.span);
  ix->min_seed_span = std::min(ix->min_seed_span, sd.span);
  ix->n_seeds++;
  return GM_OK;
}

static void choose_slabs(GmIndexHost* ix) {
  int bits = 12;
  while ((1ull << bits) < ix->total_len) bits++;
  int sb = std::min(bits, 29);
  if (const char* e = gm_tune("GM_SLAB_BITS")) sb = std::max(ix->params.region_bits + 2, std::min(31, atoi(e)));
  ix->slab_bits = sb;
  ix->n_slabs = (int)((ix->total_len + (1ull << sb) - 1) >> sb);
  if (ix->n_slabs < 1) ix->n_slabs = 1;
}

// more contigs than a window's 16-bit contig number can name (GM_MAX_CONTIGS): refused by every index entry before it builds anything
int gm_refuse_contig_count(const char* who, unsigned long long n_contigs) {
  if (n_contigs <= (unsigned long long)GM_MAX_CONTIGS) return GM_OK;
  gm_set_error("%s: %llu contigs, the limit is %d (a window carries its contig number in 16 bits)", who, n_contigs, GM_MAX_CONTIGS);
  return GM_E_RANGE;
}
// shared by gm_index_build, gm_index_load and gm_index_build_fasta: contig table (host and device), cutoff, slabs, size of the genome bitfield
static int index_tables(gm_index* ix, int n_contigs, const uint32_t* contig_len, const char* const* contig_names) {
  ix->n_contigs = n_contigs;
  ix->contig_off.resize(n_contigs + 1);
  uint64_t tot = 0;
  for (int c = 0; c < n_contigs; c++) {
    ix->contig_off[c] = (uint32_t)tot; tot += contig_len[c];
    char nm[64]; snprintf(nm, sizeof nm, "contig%d", c + 1);
    ix->names.push_back(contig_names && contig_names[c] ? contig_names[c] : nm);
  }
  if (tot >= (1ull << 32)) { gm_set_error("genome of %llu bp exceeds the reference's 32-bit global coordinates", (unsigned long long)tot); return GM_E_ARG; }
  ix->contig_off[n_contigs] = (uint32_t)tot;
  ix->total_len = tot;
  // automatic list cutoff (ref: gmapper.c:2811-2837): max(1000, 100*total/4^maxW)
  if (ix->params.list_cutoff == 0) {
    int maxw = 0; for (int i = 0; i < ix->n_seeds; i++) maxw = std::max(maxw, ix->seeds[i].weight);
    if (ix->params.hash_seeds) maxw = GM_HASH_TABLE_POWER;            // ref: gmapper.c:2820-2822
    uint32_t cutoff = 1000; unsigned long long p4 = 1ull << (2 * maxw);
    if ((uint32_t)((100ull * tot) / p4) > cutoff) cutoff = (uint32_t)((100ull * tot) / p4);
    ix->list_cutoff = cutoff;
  } else ix->list_cutoff = ix->params.list_cutoff;
  choose_slabs(ix);
  ix->genome_words = (tot + 7) / 8 + 64;
  GM_HIP(hipMalloc(&ix->d_contig_off, (size_t)(n_contigs + 1) * 4));
  GM_HIP(hipMemcpy(ix->d_contig_off, ix->contig_off.data(), (size_t)(n_contigs + 1) * 4, hipMemcpyHostToDevice));
  return GM_OK;
}
// gm_index_build and gm_index_load: the tables, then the genome re-packed into global coordinates on the host and uploaded
static int index_prepare(gm_index* ix, int n_contigs, const uint32_t* const* contigs, const uint32_t* contig_len, const char* const* contig_names) {
  { const int rc = index_tables(ix, n_contigs, contig_len, contig_names); if (rc != GM_OK) return rc; }
  // re-pack the per-contig bitfields into one bitfield in global coordinates
  std::vector<uint32_t> g(ix->genome_words, 0);
  for (int c = 0; c < n_contigs; c++) {
    const uint64_t off = ix->contig_off[c]; const uint32_t* src = contigs[c]; const uint64_t len = contig_len[c];
    const int sh = (int)(off & 7) * 4; uint64_t w0 = off >> 3; const uint64_t nw = (len + 7) / 8;
    for (uint64_t k = 0; k < nw; k++) {
      uint32_t w = src[k];
      if (k == nw - 1 && (len & 7)) w &= (1u << ((len & 7) * 4)) - 1u;
      g[w0 + k] |= w << sh;
      if (sh) g[w0 + k + 1] |= w >> (32 - sh);
    }
  }
  GM_HIP(hipMalloc(&ix->d_genome, ix->genome_words * 4));
  GM_HIP(hipMemcpy(ix->d_genome, g.data(), ix->genome_words * 4, hipMemcpyHostToDevice));
  return GM_OK;
}

extern "C" void gm_index_free(gm_index_t* ix);
static int index_seeds(gm_index* ix, int n_seeds, const char* const* seeds) {
  static const char* const DEFAULTS[3] = {"11110111101111", "1111011100100001111", "1111000011001101111"};   // load_default_seeds(0), letter space: ref gmapper-defaults.h:212-227
  if (n_seeds < 0 || (n_seeds > 0 && !seeds)) { gm_set_error("%d seeds and no seed strings", n_seeds); return GM_E_ARG; }
  if (n_seeds == 0) { n_seeds = 3; seeds = DEFAULTS; }
  for (int i = 0; i < n_seeds; i++) { const int rc = add_seed(ix, seeds[i]); if (rc != GM_OK) return rc; }      // (the first refusal's text stays in gm_last_error())
  return GM_OK;
}
extern "C" int gm_index_build(gm_index_t** out, int device, int n_contigs, const uint32_t* const* contigs,
                              const uint32_t* contig_len, const char* const* contig_names,
                              int n_seeds, const char* const* seeds, const gm_params_t* params) {
  if (!out || n_contigs < 1 || !contigs || !contig_len) { gm_set_error("gm_index_build: bad arguments"); return GM_E_ARG; }
  { const int rc = gm_refuse_contig_count("gm_index_build", (unsigned long long)n_contigs); if (rc != GM_OK) return rc; }
  if (gm_device_count() <= device) { gm_set_error("no HIP device %d (the seed index lives in HBM; there is no CPU path)", device); return GM_E_NODEVICE; }
  GM_HIP(hipSetDevice(device));
  gm_index* ix = new gm_index();
  ix->device = device;
  if (params) ix->params = *params; else gm_params_default(&ix->params);
  int rc = index_seeds(ix, n_seeds, seeds);
  if (rc != GM_OK) { delete ix; return rc; }
  rc = index_prepare(ix, n_contigs, contigs, contig_len, contig_names);
  if (rc != GM_OK) { gm_index_free(ix); return rc; }
  hipStream_t stream; GM_HIP(hipStreamCreate(&stream));
  rc = gm_index_build_device(ix, stream);
  (void)hipStreamDestroy(stream);
  if (rc != GM_OK) { gm_index_free(ix); return rc; }
  *out = ix;
  return GM_OK;
}

// S5 from the genome files themselves: the text is packed on the device (gm_fasta.hip), then the same tables and the same device build as gm_index_build
extern "C" int gm_index_build_fasta(gm_index_t** out, int device, int n_files, const char* const* paths,
                                    int n_seeds, const char* const* seeds, const gm_params_t* params) {
  if (!out || n_files < 1 || !paths) { gm_set_error("gm_index_build_fasta: bad arguments"); return GM_E_ARG; }
  if (gm_device_count() <= device) { gm_set_error("no HIP device %d (the seed index lives in HBM; there is no CPU path)", device); return GM_E_NODEVICE; }
  GM_HIP(hipSetDevice(device));
  const auto t0 = std::chrono::steady_clock::now();
  gm_index* ix = new gm_index();
  ix->device = device;
  if (params) ix->params = *params; else gm_params_default(&ix->params);
  int rc = index_seeds(ix, n_seeds, seeds);
  if (rc != GM_OK) { delete ix; return rc; }
  GmFastaGenome G;
  rc = gm_fasta_to_device(n_files, paths, &G);
  if (rc != GM_OK) { delete ix; return rc; }
  ix->d_genome = G.d_genome;                                       // (from here on gm_index_free releases it)
  std::vector<const char*> nptr(G.names.size());
  for (size_t c = 0; c < G.names.size(); c++) nptr[c] = G.names[c].c_str();
  rc = index_tables(ix, (int)G.lens.size(), G.lens.data(), nptr.data());
  if (rc == GM_OK && (ix->total_len != G.total || ix->genome_words != G.words)) { gm_set_error("gm_index_build_fasta: contig lengths do not add up to the bases packed"); rc = GM_E_ARG; }
  if (rc != GM_OK) { gm_index_free(ix); return rc; }
  const auto t1 = std::chrono::steady_clock::now();
  hipStream_t stream = nullptr;
  if (hipStreamCreate(&stream) != hipSuccess) { gm_index_free(ix); gm_set_error("hipStreamCreate failed"); return GM_E_NODEVICE; }
  rc = gm_index_build_device(ix, stream);
  (void)hipStreamDestroy(stream);
  if (rc != GM_OK) { gm_index_free(ix); return rc; }
  ix->fasta_to_bitfield_s = std::chrono::duration<double>(t1 - t0).count();
  ix->fasta_total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = ix;
  return GM_OK;
}
extern "C" int gm_index_n_contigs(const gm_index_t* ix) { return ix ? ix->n_contigs : GM_E_ARG; }
extern "C" int gm_index_contig(const gm_index_t* ix, int c, const char** name, uint32_t* len) {
  if (!ix || c < 0 || c >= ix->n_contigs) { gm_set_error("gm_index_contig: no contig %d", c); return GM_E_ARG; }
  if (name) *name = ix->names[c].c_str();
  if (len) *len = ix->contig_off[c + 1] - ix->contig_off[c];
  return GM_OK;
}
// the header gmapper prints before its records (ref: gmapper.c:2980-3008)
extern "C" int gm_sam_header(const gm_index_t* ix, const char* rg_id, const char* rg_sample, const char* command_line, char** text, size_t* len) {
  if (!ix || !text || !len) { gm_set_error("gm_sam_header: bad arguments"); return GM_E_ARG; }
  std::string h = "@HD\tVN:1.0\tSO:unsorted\n";
  for (int c = 0; c < ix->n_contigs; c++) h += "@SQ\tSN:" + ix->names[c] + "\tLN:" + std::to_string(ix->contig_off[c + 1] - ix->contig_off[c]) + "\n";
  if (rg_id) h += std::string("@RG\tID:") + rg_id + "\tSM:" + (rg_sample ? rg_sample : "") + "\n";
  if (command_line) h += std::string("@PG\tID:gmapper\tVN:2.2.3\tCL:") + command_line + "\n";
  char* p = (char*)malloc(h.size() + 1);
  if (!p) return GM_E_NOMEM;
  memcpy(p, h.c_str(), h.size() + 1);
  *text = p; *len = h.size();
  return GM_OK;
}
extern "C" int gm_index_build_timing(const gm_index_t* ix, double* to_bitfield_s, double* total_s) {
  if (!ix || ix->fasta_total_s <= 0) { gm_set_error("gm_index_build_timing: not an index built by gm_index_build_fasta"); return GM_E_ARG; }
  if (to_bitfield_s) *to_bitfield_s = ix->fasta_to_bitfield_s;
  if (total_s) *total_s = ix->fasta_total_s;
  return GM_OK;
}

extern "C" void gm_index_free(gm_index_t* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  (void)hipFree(ix->d_genome); (void)hipFree(ix->d_genome_cs); (void)hipFree(ix->d_contig_off); (void)hipFree(ix->d_contig_rna);
  for (int i = 0; i < ix->n_seeds; i++) { (void)hipFree(ix->seeds[i].d_dir); (void)hipFree(ix->seeds[i].d_pos); (void)hipFree(ix->seeds[i].d_bkt);
                                           (void)hipFree(ix->seeds[i].d_sdir); (void)hipFree(ix->seeds[i].d_spos); }
  delete ix;
}
extern "C" uint32_t gm_index_list_cutoff(const gm_index_t* ix) { return ix->list_cutoff; }
extern "C" int gm_index_n_slabs(const gm_index_t* ix) { return ix->n_slabs; }
extern "C" int gm_index_has_buckets(const gm_index_t* ix) { return ix->seeds[0].d_bkt != nullptr; }
extern "C" uint64_t gm_index_bytes(const gm_index_t* ix) {
  uint64_t b = ix->genome_words * 4 * (ix->d_genome_cs ? 2 : 1);
  for (int i = 0; i < ix->n_seeds; i++) b += (ix->seeds[i].dir_words + (uint64_t)ix->seeds[i].n_pos + (ix->seeds[i].d_bkt ? (16ull << ix->seeds[i].kbits) : 0ull) +
                                            (ix->seeds[i].d_sdir ? (1ull << ix->seeds[i].kbits) + 1 + ix->seeds[i].n_spos : 0ull)) * 4;
  return b;
}
extern "C" int gm_index_get_list(const gm_index_t* ix, int sn, uint32_t mapidx, uint32_t* len, uint32_t* positions, uint32_t cap) {
  if (sn < 0 || sn >= ix->n_seeds || mapidx >= (1u << ix->seeds[sn].kbits)) return GM_E_ARG;
  GM_HIP(hipSetDevice(ix->device));
  uint32_t be[2];
  GM_HIP(hipMemcpy(&be[0], ix->seeds[sn].d_dir + (size_t)mapidx * ix->n_slabs, 4, hipMemcpyDeviceToHost));
  GM_HIP(hipMemcpy(&be[1], ix->seeds[sn].d_dir + (size_t)(mapidx + 1) * ix->n_slabs, 4, hipMemcpyDeviceToHost));
  *len = be[1] - be[0];
  uint32_t n = std::min(*len, cap);
  if (n && positions) GM_HIP(hipMemcpy(positions, ix->seeds[sn].d_pos + be[0], (size_t)n * 4, hipMemcpyDeviceToHost));
  return GM_OK;
}
extern "C" int gm_index_device_array(const gm_index_t* ix, int kind, void** dev_ptr, uint64_t* bytes) {
  if (kind == 0) { *dev_ptr = ix->d_genome; *bytes = ix->genome_words * 4; return GM_OK; }
  if (kind == 1 + 3 * ix->n_seeds) { *dev_ptr = ix->d_genome_cs; *bytes = ix->d_genome_cs ? ix->genome_words * 4 : 0; return GM_OK; }   // colour translation of the genome
  const int sn = (kind - 1) / 3, what = (kind - 1) % 3; if (kind < 0 || sn < 0 || sn >= ix->n_seeds) return GM_E_ARG;
  if (what == 0) { *dev_ptr = ix->seeds[sn].d_dir; *bytes = (ix->seeds[sn].dir_words + 16) * 4; }
  else if (what == 1) { *dev_ptr = ix->seeds[sn].d_pos; *bytes = ((uint64_t)ix->seeds[sn].n_pos + 64) * 4; }
  else { *dev_ptr = ix->seeds[sn].d_bkt; *bytes = ix->seeds[sn].d_bkt ? (16ull << ix->seeds[sn].kbits) * 4 : 0; }
  return GM_OK;
}

// metadata blob: everything but the device arrays (fixed header + contig offsets + names + seed strings)
struct MetaHdr { uint64_t magic, total_len, genome_words; int32_t n_contigs, n_seeds, slab_bits, n_slabs; uint32_t list_cutoff, pad; gm_params_t params;
                 uint32_t n_pos[GM_MAX_SEEDS]; uint64_t dir_words[GM_MAX_SEEDS]; uint32_t has_bkt[GM_MAX_SEEDS]; };
extern "C" int gm_index_meta(const gm_index_t* ix, void* meta, uint64_t* meta_bytes) {
  std::string blob;
  MetaHdr h; memset(&h, 0, sizeof h);
  h.magic = 0x474D4958ull; h.total_len = ix->total_len; h.genome_words = ix->genome_words; h.n_contigs = ix->n_contigs; h.n_seeds = ix->n_seeds;
  h.slab_bits = ix->slab_bits; h.n_slabs = ix->n_slabs; h.list_cutoff = ix->list_cutoff; h.params = ix->params;
  for (int i = 0; i < ix->n_seeds; i++) { h.n_pos[i] = ix->seeds[i].n_pos; h.dir_words[i] = ix->seeds[i].dir_words; h.has_bkt[i] = ix->seeds[i].d_bkt != nullptr; }
  blob.append((const char*)&h, sizeof h);
  blob.append((const char*)ix->contig_off.data(), (size_t)(ix->n_contigs + 1) * 4);
  for (auto& n : ix->names) { blob += n; blob.push_back('\0'); }
  for (int i = 0; i < ix->n_seeds; i++) { blob += ix->seeds[i].text; blob.push_back('\0'); }
  if (meta && *meta_bytes >= blob.size()) memcpy(meta, blob.data(), blob.size());
  *meta_bytes = blob.size();
  return GM_OK;
}
extern "C" int gm_index_alloc_like(gm_index_t** out, int device, const void* meta, uint64_t meta_bytes) {
  if (meta_bytes < sizeof(MetaHdr)) return GM_E_ARG;
  MetaHdr h; memcpy(&h, meta, sizeof h);
  if (h.magic != 0x474D4958ull) return GM_E_ARG;
  if (gm_device_count() <= device) { gm_set_error("no HIP device %d", device); return GM_E_NODEVICE; }
  GM_HIP(hipSetDevice(device));
  gm_index* ix = new gm_index();
  ix->device = device; ix->params = h.params; ix->total_len = h.total_len; ix->genome_words = h.genome_words; ix->n_contigs = h.n_contigs;
  ix->slab_bits = h.slab_bits; ix->n_slabs = h.n_slabs; ix->list_cutoff = h.list_cutoff;
  const char* p = (const char*)meta + sizeof h;
  ix->contig_off.assign((const uint32_t*)p, (const uint32_t*)p + h.n_contigs + 1); p += (size_t)(h.n_contigs + 1) * 4;
  for (int c = 0; c < h.n_contigs; c++) { ix->names.push_back(p); p += strlen(p) + 1; }
  for (int i = 0; i < h.n_seeds; i++) { if (add_seed(ix, p) != GM_OK) { delete ix; return GM_E_ARG; } p += strlen(p) + 1; }
  GM_HIP(hipMalloc(&ix->d_genome, ix->genome_words * 4));
  if (ix->params.colour_space) GM_HIP(hipMalloc(&ix->d_genome_cs, ix->genome_words * 4));
  GM_HIP(hipMalloc(&ix->d_contig_off, (size_t)(h.n_contigs + 1) * 4));
  GM_HIP(hipMemcpy(ix->d_contig_off, ix->contig_off.data(), (size_t)(h.n_contigs + 1) * 4, hipMemcpyHostToDevice));
  for (int i = 0; i < h.n_seeds; i++) {
    ix->seeds[i].n_pos = h.n_pos[i]; ix->seeds[i].dir_words = h.dir_words[i];
    GM_HIP(hipMalloc(&ix->seeds[i].d_dir, (h.dir_words[i] + 16) * 4));
    GM_HIP(hipMalloc(&ix->seeds[i].d_pos, ((uint64_t)h.n_pos[i] + 64) * 4));
    if (h.has_bkt[i]) GM_HIP(hipMalloc(&ix->seeds[i].d_bkt, (16ull << ix->seeds[i].kbits) * 4));
  }
  *out = ix;
  return GM_OK;
}

// ---- session ----------------------------------------------------------------------------------
// One read set of a sub-batch: every device array K1..K4 need for reads of ONE length.  Unpaired
// mapping uses set[0]; paired mapping uses set[0] for the first mates and set[1] for the second.
struct DevSet {
  // capacities (grown on overflow)
  int cur_len = -1, scap = 0, scap2 = 0, hcap = 0, rcap_per_read = 8, ops_stride = 0, eff_batch = 0;
  int post_threads = 0;                                      // threads of k_post_sw_cs (each owns a column scratch)
  int p2_grid = 0;                                           // pass-2 grid for this read length: the session's, capped so that the back-pointer scratch stays within 2 GB
  int8_t* d_xover = nullptr; bool xover_on = false;        // colour space with QVs: per-position crossover scores [B][read_len]
  uint8_t* d_qv = nullptr; uint8_t* d_post_bq = nullptr;   // ... and the QVs themselves (clamped to 0..250) for post_sw on the device, which leaves the base qualities in d_post_bq [rcap][read_len]
  uint8_t* d_read_rna = nullptr;                             // letter space: 1 for a read with uracil and no thymine (re->is_rna, ref: fasta.c:528-542), set per sub-batch by k_read_rna_flags
  uint32_t* d_reads = nullptr; uint8_t* d_initbp = nullptr; uint64_t* d_surv = nullptr; uint32_t* d_surv_cnt = nullptr;   // d_initbp: colour space primer letters
  uint32_t* d_surv_seg = nullptr;                                          // [2B][S + 1] survivors after each slab (K1 emits slab by slab)
  uint64_t* d_surv2 = nullptr; uint32_t* d_surv_cnt2 = nullptr;            // survivors after the exact isolation prune (K1b) = input of K2
  GmHit* d_hits = nullptr; uint16_t* d_perm = nullptr; uint32_t* d_hit_cnt = nullptr; unsigned long long* d_slots = nullptr;
  uint32_t* d_heavy_list = nullptr; uint32_t* d_heavy_cnt = nullptr;   // read-strands beyond the LDS tier of K2
  int32_t* d_sel = nullptr; int32_t* d_sel_sidx = nullptr; uint32_t* d_sel_cnt = nullptr; uint32_t* d_sel_off = nullptr; uint32_t* d_work = nullptr; uint32_t* d_n_work = nullptr; uint32_t* d_p2_order = nullptr; uint32_t* d_p2_cls = nullptr;   // (pass 2's work items by kind, see k_p2cs_classify)
  GmFullRes* d_res = nullptr; uint8_t* d_ops = nullptr; uint8_t* d_back = nullptr; size_t back_stride = 0;
  GmPostRes* d_post = nullptr; double* d_post_fw = nullptr; uint32_t* d_post_info = nullptr;   // colour space: post_sw on the device (gm_post.hip), its per-thread scratch
  // paired mode only: mate range of every window (by sorted position) and the "saved" mark (by hit slot)
  int32_t* d_pmin = nullptr; int32_t* d_pmax = nullptr; uint8_t* d_saved = nullptr; uint32_t* d_saved_list = nullptr;
  int caps_pair_mode = 0;      // the paired match mode the capacities were chosen for
  uint32_t* d_mp_rows = nullptr; uint32_t* d_mp_cnt = nullptr; int mp_rows_for = 0;     // paired -n 3: the regions each read-strand marked twice (GmMpDev), for mp_rows_for read-strands
};

// Pinned host staging for one sub-batch's results: device-to-host copies run at link rate and the buffers are reused
// (three slots: one being filled while the host threads still work on the two sub-batches before it).
struct HostSlot {
  GmFullRes* res = nullptr; uint8_t* ops = nullptr; uint32_t* sel_cnt = nullptr; uint32_t* sel_off = nullptr; uint32_t* reads = nullptr;
  uint8_t* post_bq = nullptr; size_t post_bq_cap = 0; bool post_bq_on = false;   // base qualities of the device's post_sw (reads with QVs), read_len bytes per result
  GmPostRes* post = nullptr; size_t post_cap = 0; bool post_on = false;      // colour space: the device's post_sw results of this sub-batch (post_on: they are there)
  size_t res_cap = 0, ops_cap = 0, n_cap = 0, reads_cap = 0; uint32_t n_work = 0;
  bool want_reads = false;                                   // set by the caller: copy the sub-batch's packed reads back as well (reads handed over in device memory)
  unsigned long long* stats = nullptr; size_t stats_cap = 0;   // the sub-batch's stage counters as the device left them (pinned: their copy must not block the calling thread)
};
static int slot_reserve(void** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return GM_OK;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr; *cap = 0;
  const size_t want = bytes + bytes / 4 + 4096;
  GM_HIP(hipHostMalloc(p, want, hipHostMallocDefault));
  *cap = want;
  return GM_OK;
}
static void slot_free(HostSlot& h) {
  void* ptrs[] = {h.res, h.ops, h.sel_cnt, h.sel_off, h.reads, h.post, h.post_bq, h.stats};
  for (void* p : ptrs) if (p) (void)hipHostFree(p);
  h = HostSlot();
}

// A grow-only pinned host buffer that stands in for a std::vector as the target of a device-to-host copy (a copy into pageable memory is staged and blocks the caller)
template <class T> struct GmPinVec {
  T* p = nullptr; size_t cap = 0, n = 0;
  int resize(size_t k) { n = k; void* q = p; const int rc = slot_reserve(&q, &cap, k * sizeof(T)); p = (T*)q; return rc; }
  T* data() { return p; } const T* data() const { return p; } T& operator[](size_t i) { return p[i]; } const T& operator[](size_t i) const { return p[i]; } size_t size() const { return n; }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; n = 0; }
};
struct gm_session {
  GmPinVec<GmFullRes> pin_res[8]; GmPinVec<uint8_t> pin_ops[8];   // paired path: results of the pairs' pass 2 (0, 1: the mates) and of the half-paired rescue (2, 3); 4-7: the same for
                                                                  // odd sub-batches (the output stage of a sub-batch reads them on its own thread while the next one's copies arrive)
  gm_session* twin = nullptr;                     // a second session on the same index with the same parameters, made by the file entry the first time a file has more than one
                                                  // chunk: it maps every other chunk, so that a chunk's tail runs under the next chunk's lookups (freed with this one)
  const gm_index* ix = nullptr;
  gm_params_t P; GmScoreDev sc;
  double score_alpha = 0, score_beta = 0;
  double pr_mismatch = .01, pr_del_open = 0, pr_del_extend = 0, pr_ins_open = 0, pr_ins_extend = 0;   // post_sw_setup's arguments (ref: gmapper.c:2568-2571,2959-2963)
  double* d_qtab = nullptr;                       // colour space: log(1 - e(q)), log(e(q) / 3) for q = 0..250 as the host's libm computes them, for post_sw on the device with QVs
  int max_batch = 0, p2_grid = 16384;             // pass-2 waves in flight (GM_P2_GRID); each owns a back-pointer scratch, see DevSet::p2_grid
  hipStream_t stream = nullptr;                   // front of the pipeline (reads in, K1, K1b, K2); the only stream of the paired path
  hipStream_t stream_b = nullptr;                 // back of the pipeline (pass 1, selection, pass 2, results out): runs beside the next sub-batch's front
  hipStream_t stream_c = nullptr;                 // host -> device copies of the next sub-batch (never queued behind kernels)
  hipEvent_t ev[12] = {};                          // (null until created: gm_session_free also takes a session whose set-up stopped half-way)
  hipEvent_t pev[2][10] = {};                      // per buffer set: stage boundaries, front done, copies done
  hipEvent_t pkev[2][4] = {};                      // paired mode: begin / end of K1 for mate set 0 and 1 of buffer pair k
  unsigned long long* d_pstats[2] = {nullptr, nullptr};   // per buffer set: counters of one sub-batch
  uint32_t* h_pin = nullptr;                      // pinned words the front writes (heavy count per set); from word 16 on: K1's start flags
  uint32_t flag_epoch = 0, front_epoch[2] = {0, 0}; int front_flag_grid[2] = {0, 0};
  GmK1Scratch k1;                                 // K1 / K1b launch scratch: every launch that touches it is queued on `stream`
  DevSet set[2];
  DevSet set2[2];                                 // paired mode: the second pair of buffer sets of the two-stream pipeline
  HostSlot slot[3];
  uint32_t* d_pairs = nullptr; uint32_t* d_pair_cnt = nullptr; int pairs_cap = 0;   // paired mode: selected (mate 1, mate 2) window pairs
  unsigned long long* d_stats = nullptr;
  std::vector<uint32_t> h_genome;                 // host copy of the packed genome: only for the SHRiMP / pretty output formats, which print genome letters (fetched on first use)
  // last lookup timing
  double last_lookup_ms = 0; uint64_t last_lookup_bytes = 0; int last_lookup_launches = 0;
};

static void free_buffers(DevSet& D) {
  void* ptrs[] = {D.d_read_rna, D.d_xover, D.d_reads, D.d_initbp, D.d_surv, D.d_surv_cnt, D.d_surv_seg, D.d_surv2, D.d_surv_cnt2, D.d_hits, D.d_perm, D.d_hit_cnt, D.d_slots, D.d_heavy_list, D.d_heavy_cnt,
                  D.d_sel, D.d_sel_sidx, D.d_sel_cnt, D.d_sel_off, D.d_work, D.d_n_work, D.d_p2_order, D.d_p2_cls, D.d_res, D.d_ops, D.d_back,
                  D.d_pmin, D.d_pmax, D.d_saved, D.d_saved_list, D.d_post, D.d_post_fw, D.d_post_info, D.d_qv, D.d_post_bq, D.d_mp_rows, D.d_mp_cnt};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  D.d_post = nullptr; D.d_post_fw = nullptr; D.d_post_info = nullptr; D.d_qv = nullptr; D.d_post_bq = nullptr;
  D.d_read_rna = nullptr; D.d_xover = nullptr; D.d_reads = nullptr; D.d_initbp = nullptr; D.d_surv = nullptr; D.d_surv_cnt = nullptr; D.d_surv_seg = nullptr; D.d_surv2 = nullptr; D.d_surv_cnt2 = nullptr; D.d_hits = nullptr; D.d_perm = nullptr; D.d_hit_cnt = nullptr; D.d_slots = nullptr;
  D.d_heavy_list = nullptr; D.d_heavy_cnt = nullptr; D.d_sel = nullptr; D.d_sel_sidx = nullptr; D.d_sel_cnt = nullptr; D.d_sel_off = nullptr;
  D.d_work = nullptr; D.d_n_work = nullptr; D.d_p2_order = nullptr; D.d_p2_cls = nullptr; D.d_res = nullptr; D.d_ops = nullptr; D.d_back = nullptr;
  D.d_pmin = nullptr; D.d_pmax = nullptr; D.d_saved = nullptr; D.d_saved_list = nullptr;
  D.d_mp_rows = nullptr; D.d_mp_cnt = nullptr; D.mp_rows_for = 0;
  D.cur_len = -1;
}

static int pow2ceil(long long v) { int p = 1; while (p < v) p <<= 1; return p; }
// host threads of this process's share (a multi-rank job divides the cores itself: GM_HOST_THREADS)
// The hardware's processor count, and the container's CPU quota where there is one (cgroup v2 cpu.max / v1 cfs quota).  A one-GPU box of this pool shows 256 processors
// and grants 16 CPUs' worth of time per period.  The worker count does NOT follow the quota: the finalisation comes in bursts (a ~10 ms job per sub-batch), the quota is
// accounted per 100 ms, and 32 threads that finish a burst early beat 16 that never exceed it -- measured on such a box: 100 Mbp workload 9.2-9.5 M reads/s with 32 threads,
// 8.5 M with 16; colour space 4.27 against 4.00 M; the 3 Gbp workload, whose host work averages 7 cores, is the same.  gm_usable_cores() is for reporting.
static int gm_usable_cores() {
  static const int cached = [] {
    int n = (int)std::max(1u, std::thread::hardware_concurrency());
    long long quota = -1, period = -1;
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) { char q[64] = ""; if (fscanf(f, "%63s %lld", q, &period) == 2 && strcmp(q, "max") != 0) quota = atoll(q); fclose(f); }
    else {
      if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lld", &quota) != 1) quota = -1; fclose(g); }
      if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lld", &period) != 1) period = -1; fclose(g); }
    }
    if (quota > 0 && period > 0) n = std::min<long long>(n, std::max<long long>(1, (quota + period - 1) / period));
    return n;
  }();
  return cached;
}
static int gm_host_threads(int cap) {                         // (cap: 32 for the unpaired jobs and the parallel loops, 16 for the paired stages; the environment is read on every call)
  int n = (int)std::min<unsigned>((unsigned)cap, std::max(1u, std::thread::hardware_concurrency()));
  if (const char* e = getenv("GM_HOST_THREADS")) n = std::max(1, atoi(e));
  (void)&gm_usable_cores;
  return n;
}
// The host side's worker threads, kept for the life of the process (round 4: every sub-batch's finalisation started -- and joined -- up to 32 threads of its own, eight times
// per million reads).  gm_run_on_threads(n, f) runs f on n threads at once (n - 1 pool threads + the caller) and returns when all are done; calls from different threads
// (two finalisation jobs overlap) share the pool, which grows to the largest n asked for.
namespace {
struct GmThreadPool {
  // one call of run(): shared by the caller and the queue entries, so that whoever finishes last still finds it alive
  struct Call { const std::function<void()>* fn = nullptr; int left = 0; std::mutex m; std::condition_variable cv; };
  std::mutex m; std::condition_variable cv; std::deque<std::shared_ptr<Call>> q; std::vector<std::thread> workers; bool stop = false;
  ~GmThreadPool() { { std::lock_guard<std::mutex> lk(m); stop = true; } cv.notify_all(); for (auto& t : workers) if (t.joinable()) t.join(); }
  void loop() {
    for (;;) {
      std::shared_ptr<Call> c;
      { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return stop || !q.empty(); }); if (q.empty()) return; c = std::move(q.front()); q.pop_front(); }
      (*c->fn)();
      { std::lock_guard<std::mutex> lk(c->m); if (--c->left == 0) c->cv.notify_all(); }
    }
  }
  void run(int n, const std::function<void()>& fn) {
    if (n <= 1) { fn(); return; }
    auto c = std::make_shared<Call>(); c->fn = &fn; c->left = n - 1;
    { std::lock_guard<std::mutex> lk(m);
      while ((int)workers.size() < n - 1) workers.emplace_back([this] { loop(); });
      for (int t = 1; t < n; t++) q.push_back(c); }
    cv.notify_all();
    fn();
    std::unique_lock<std::mutex> lk(c->m); c->cv.wait(lk, [&] { return c->left == 0; });      // (fn stays valid until here: every worker has returned from it)
  }
};
GmThreadPool& gm_pool() { static GmThreadPool* p = new GmThreadPool(); return *p; }      // (never destroyed: no join at process exit while a caller may still hold the library)
}
static void gm_run_on_threads(int n, const std::function<void()>& fn) { gm_pool().run(n, fn); }
// Text buffers of the finalisation chunks, recycled across sub-batches and calls: a fresh std::string per chunk and job meant ~250 MB of first-touch page faults per million reads.
namespace {
struct GmTextPool {
  std::mutex m; std::vector<std::string> free_;
  std::string take() { std::lock_guard<std::mutex> lk(m); if (free_.empty()) return std::string(); std::string t = std::move(free_.back()); free_.pop_back(); t.clear(); return t; }
  void give(std::string&& t) { if (t.capacity() == 0 || t.capacity() > (16u << 20)) return; std::lock_guard<std::mutex> lk(m); if (free_.size() < 512) free_.push_back(std::move(t)); }
  void drop() { std::lock_guard<std::mutex> lk(m); free_.clear(); free_.shrink_to_fit(); }
};
GmTextPool& gm_text_pool() { static GmTextPool* p = new GmTextPool(); return *p; }
}
static void gm_text_pool_drop() { gm_text_pool().drop(); }
// fn(begin, end) over [0, n) in pieces of `grain`, on the host threads
template <class F> static void gm_parallel_for(size_t n, size_t grain, F fn) {
  const size_t pieces = (n + grain - 1) / std::max<size_t>(1, grain);
  const int nt = (int)std::min<size_t>((size_t)gm_host_threads(32), pieces);
  if (nt <= 1) { if (n) fn((size_t)0, n); return; }
  std::atomic<size_t> next(0);
  gm_run_on_threads(nt, [&]() { for (;;) { const size_t c = next.fetch_add(1); if (c >= pieces) break; fn(c * grain, std::min(n, (c + 1) * grain)); } });
}
static bool gm_fixed_lines(const char* text, size_t n, size_t want) {
  if (!n) return true;
  const size_t len = strlen(text), stride = want + 1;
  if (len != n * stride - 1 && len != n * stride) return false;
  std::atomic<bool> ok(true);
  gm_parallel_for(n, 16384, [&](size_t b, size_t e) {
    for (size_t i = b; i < e; i++) {
      const char* p = text + i * stride;
      if (memchr(p, '\n', want) != nullptr || (i + 1 < n && p[want] != '\n')) { ok = false; return; }
    }
  });
  return ok;
}

// -a: 0 .. 99, or -1 for no anchor band at all -- the threshold band in every full alignment (gm_sw.hip threshold_box); the reference exits on anything else (gmapper.c:2014-2016)
static int gm_check_anchor_width(const char* who, int anchor_width) {
  if (anchor_width >= -1 && anchor_width <= 99) return GM_OK;
  gm_set_error("%s: anchor_width %d outside [-1, 99] (ref: gmapper.c:2014-2016)", who, anchor_width); return GM_E_ARG;
}

static int window_len_of(const gm_params_t& P, int read_len) {   // ref: gmapper.c:530
  double w = P.window_len < 0 ? -P.window_len : read_len * (P.window_len / 100.0);
  return (int)(uint16_t)w;
}

static int alloc_buffers(gm_session* s, DevSet& D, int read_len, bool paired = false) {
  free_buffers(D);
  const gm_index* ix = s->ix;
  const int read_words = (read_len + 7) / 8;
  const int W = window_len_of(s->P, read_len);
  // sub-batch size under a device-memory budget (candidate windows dominate when hcap has grown)
  const double budget = 16e9;
  const double per_read = 2.0 * ((double)(D.scap + D.scap2) * 8 + (double)D.hcap * (sizeof(GmHit) + 2 + 8)) + (double)D.rcap_per_read * (sizeof(GmFullRes) + read_len + W + 16);
  D.eff_batch = (int)std::max(64.0, std::min((double)s->max_batch, budget / per_read));
  const int B = D.eff_batch, rs = 2 * B;
  (void)ix;
  D.ops_stride = ((read_len + W + 15) / 16) * 16;
  D.back_stride = (((size_t)read_len * W + 255) / 256) * 256;
  if (s->P.colour_space) { D.ops_stride *= 2; D.back_stride *= 12; }   // backtrace byte + letter codes per column; three words of back pointers per cell
  GM_HIP(hipMalloc(&D.d_reads, (size_t)B * read_words * 4 + 64));
  if (!s->P.colour_space) GM_HIP(hipMalloc(&D.d_read_rna, (size_t)B + 64));
  if (s->P.colour_space) { GM_HIP(hipMalloc(&D.d_initbp, (size_t)B + 64)); GM_HIP(hipMalloc(&D.d_xover, (size_t)B * read_len + 64)); GM_HIP(hipMalloc(&D.d_qv, (size_t)B * read_len + 64)); }
  GM_HIP(hipMalloc(&D.d_surv, (size_t)rs * D.scap * 8));
  GM_HIP(hipMalloc(&D.d_surv_cnt, (size_t)rs * 4));
  if (D.scap2 > 0) {
    GM_HIP(hipMalloc(&D.d_surv2, (size_t)rs * D.scap2 * 8)); GM_HIP(hipMalloc(&D.d_surv_cnt2, (size_t)rs * 4));
    GM_HIP(hipMalloc(&D.d_surv_seg, (size_t)rs * (ix->n_slabs + 1) * 4));
  }
  GM_HIP(hipMalloc(&D.d_hits, (size_t)rs * D.hcap * sizeof(GmHit)));
  GM_HIP(hipMalloc(&D.d_perm, (size_t)rs * D.hcap * 2));
  GM_HIP(hipMalloc(&D.d_hit_cnt, (size_t)rs * 4));
  GM_HIP(hipMalloc(&D.d_slots, (size_t)rs * D.hcap * 8));
  GM_HIP(hipMalloc(&D.d_heavy_list, (size_t)rs * 4));
  GM_HIP(hipMalloc(&D.d_heavy_cnt, 4));
  GM_HIP(hipMalloc(&D.d_sel, (size_t)B * GM_SEL_MAX * 4));
  GM_HIP(hipMalloc(&D.d_sel_cnt, (size_t)B * 4));
  GM_HIP(hipMalloc(&D.d_sel_off, (size_t)B * 4));
  const size_t rcap = (size_t)B * D.rcap_per_read;
  GM_HIP(hipMalloc(&D.d_work, (size_t)B * GM_SEL_MAX * 4));
  GM_HIP(hipMalloc(&D.d_n_work, 4));
  GM_HIP(hipMalloc(&D.d_p2_order, (size_t)B * GM_SEL_MAX * 4)); GM_HIP(hipMalloc(&D.d_p2_cls, 16));
  GM_HIP(hipMalloc(&D.d_res, rcap * sizeof(GmFullRes)));
  GM_HIP(hipMalloc(&D.d_ops, rcap * D.ops_stride));
  if (s->P.colour_space && !getenv("GM_POST_SW_HOST")) {     // post_sw on the device (gm_post.hip): one record per result, forward values + column descriptors per thread
    GM_HIP(hipMalloc(&D.d_post, rcap * sizeof(GmPostRes)));
    D.post_threads = GM_POST_THREADS;
    while (D.post_threads > 16384 && (size_t)D.post_threads * (size_t)(read_len + 1) * 140 > ((size_t)2 << 30)) D.post_threads /= 2;      // (long reads: at most 2 GB of scratch a buffer set)
    if (const char* e = gm_tune("GM_POST_THREADS")) D.post_threads = std::max(4096, std::min(1 << 20, atoi(e) & ~63));
    GM_HIP(hipMalloc(&D.d_post_fw, (size_t)D.post_threads * (size_t)(read_len + 1) * 17 * 8));
    GM_HIP(hipMalloc(&D.d_post_info, (size_t)D.post_threads * (size_t)(read_len + 1) * 4));
    GM_HIP(hipMalloc(&D.d_post_bq, rcap * (size_t)read_len + 64));
  }
  D.p2_grid = (int)std::max<size_t>(256, std::min<size_t>((size_t)s->p2_grid, ((size_t)2 << 30) / D.back_stride));
  GM_HIP(hipMalloc(&D.d_back, (size_t)D.p2_grid * D.back_stride));
  if (paired) {
    GM_HIP(hipMalloc(&D.d_sel_sidx, (size_t)B * GM_SEL_MAX * 4));
    GM_HIP(hipMalloc(&D.d_pmin, (size_t)rs * D.hcap * 4)); GM_HIP(hipMalloc(&D.d_pmax, (size_t)rs * D.hcap * 4));
    GM_HIP(hipMalloc(&D.d_saved, (size_t)rs * D.hcap)); GM_HIP(hipMalloc(&D.d_saved_list, (size_t)B * GM_SEL_MAX * 4));
  }
  D.cur_len = read_len;
  return GM_OK;
}

// pair_mode: the paired match mode when called for pairs (0: unpaired).  Modes 3 and 2 have no prune rules (a single k-mer match can open a window) and K2 takes
// the lookup's rows directly: its LDS tier holds 4096 keys; mode 2 keeps every list entry
static void choose_caps(const gm_session* s, DevSet& D, int read_len, int pair_mode = 0) {
  const gm_index* ix = s->ix;
  const int max_n_kmers = std::max(0, read_len - ix->min_seed_span + 1);
  double lists = 0, avg_len = 0;
  for (int i = 0; i < ix->n_seeds; i++) {
    lists += std::max(0, read_len - ix->seeds[i].span + 1);
    avg_len += (double)ix->seeds[i].n_pos / (double)(1ull << ix->seeds[i].kbits) / ix->n_seeds;
  }
  const double entries = lists * avg_len;
  const double region = (double)(1 << ix->params.region_bits) + ix->params.region_overlap;
  double expected = entries * std::min(1.0, entries * region / std::max(1.0, (double)ix->total_len)) + lists;
  if (pair_mode ? pair_mode == 2 : s->P.match_mode == 1) expected = entries + lists;                        // -n 1 (paired: -n 2): every list entry is kept
  // scap = capacity of the LDS tier of K2 (16 B of LDS per entry); read-strands beyond it take the heavy tier
  // chance partial matches echo on neighbouring offsets / other seeds, so the survivors come out ~1.6x the independence estimate
  D.scap = std::min(16384, std::max(256, pow2ceil((long long)(2.2 * expected) + 128)));
  D.hcap = 64;
  // K1b (exact isolation prune) shrinks K2's input; its LDS tier is sized for what typically remains
  // K1b's bounds assume the window-generation threshold: not in -U mode
  // (a read that maps keeps one survivor per list at its true place -- 251 at 100 bases -- before any chance survivor: a tier of 256 sent 2 % of the read-strands of the
  // 100 Mbp workload through the heavy tier, whose host round trips then cost a quarter of the step; the tier holds one and a half times the lists)
  D.scap2 = (s->P.match_mode == 2 && !s->P.ungapped && !gm_tune("GM_NO_PRUNE")) ? std::max(std::min(D.scap, std::max(256, pow2ceil((long long)(1.5 * lists)))), D.scap / 8) : 0;
  if (pair_mode == 2 || pair_mode == 3) { D.scap = std::min(D.scap, 4096); D.scap2 = 0; }
  if (const char* e = gm_tune("GM_SCAP")) D.scap = std::min(16384, std::max(64, pow2ceil(atoi(e))));
  if (const char* e = gm_tune("GM_SCAP2")) { if (D.scap2) D.scap2 = std::min(D.scap, std::max(64, pow2ceil(atoi(e)))); }
  if (const char* e = gm_tune("GM_HCAP")) D.hcap = std::min(32768, std::max(4, pow2ceil(atoi(e))));
  (void)max_n_kmers;
}

// log(1 - e(q)), log(e(q) / 3) for q = 0..250 with the host's libm: the per-colour error rates post_sw derives from quality values (ref: sw-post.c:486-491, pr_err_from_qv
// util.h:285-293), for every QV the formula distinguishes -- the device kernels read the very doubles the host routine computes.  sanger: PHRED, else Solexa-style odds.
static std::vector<double> cs_qv_table(bool sanger) {
  std::vector<double> qt(2 * 251);
  for (int q = 0; q <= 250; q++) {
    double e = q <= 0 ? .99999999 : (q >= 250 ? 1E-25 : pow(10.0, -(double)q / 10.0));
    if (!sanger) e /= (1 + e);
    if (e > .75) e = .75;
    qt[2 * q] = log(1 - e); qt[2 * q + 1] = log(e / 3.0);
  }
  return qt;
}

extern "C" void gm_session_free(gm_session_t* s);
extern "C" int gm_session_create(gm_session_t** out, const gm_index_t* ix, const gm_params_t* params, int max_batch_reads) {
  if (!out || !ix) return GM_E_ARG;
  GM_HIP(hipSetDevice(ix->device));
  gm_session* s = new gm_session();
  s->ix = ix; s->P = params ? *params : ix->params;
  // (the parameters are checked before anything is allocated; every failure further down goes through gm_session_free, which releases what exists by then)
  if (s->P.strand_only < 0 || s->P.strand_only > 2) { delete s; gm_set_error("strand_only %d: 0 (both), 1 (-F) or 2 (-C)", params ? params->strand_only : 0); return GM_E_ARG; }
  if (s->P.match_mode != 1 && s->P.match_mode != 2) { delete s; gm_set_error("match_mode %d: 1 or 2 (ref: gmapper.c:2624; 3 and 4 are paired-mode settings with mate-pair region counts)", s->P.match_mode); return GM_E_ARG; }
  if (gm_check_anchor_width("gm_session_create", s->P.anchor_width)) { delete s; return GM_E_ARG; }
  if (s->P.ungapped && !s->P.local_alignment) { delete s; gm_set_error("ungapped mode needs local alignment (ref: gmapper.c:2330-2333)"); return GM_E_ARG; }
  if ((s->P.colour_space != 0) != (ix->params.colour_space != 0)) { delete s; gm_set_error("session and index disagree on colour space"); return GM_E_ARG; }
  s->sc = make_score(s->P);
#define GM_HIP_S(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { gm_set_error("%s: %s", #call, hipGetErrorString(e_)); gm_session_free(s); return GM_E_NODEVICE; } } while (0)
  // score -> probability derivation (ref: gmapper.c:2557-2572)
  if (s->P.colour_space) {   // pr_xover => alpha => pr_mismatch
    s->score_alpha = (double)s->P.crossover_score / (log(s->P.pr_xover / 3) / log(2.0));
    s->pr_mismatch = 1.0 / (1.0 + 1.0 / 3.0 * pow(2.0, ((double)s->P.match_score - (double)s->P.mismatch_score) / s->score_alpha));
  } else {                   // pr_mismatch => alpha
    s->pr_mismatch = .01;
    s->score_alpha = ((double)s->P.match_score - (double)s->P.mismatch_score) / (log((1 - s->pr_mismatch) / (s->pr_mismatch / 3.0)) / log(2.0));
  }
  s->score_beta = (double)s->P.match_score - 2 * s->score_alpha - s->score_alpha * log(1 - s->pr_mismatch) / log(2.0);
  s->pr_del_open = pow(2.0, (double)s->P.a_gap_open_score / s->score_alpha);
  s->pr_ins_open = pow(2.0, (double)s->P.b_gap_open_score / s->score_alpha);
  s->pr_del_extend = pow(2.0, (double)s->P.a_gap_extend_score / s->score_alpha);
  s->pr_ins_extend = pow(2.0, ((double)s->P.b_gap_extend_score - s->score_beta) / s->score_alpha);
  if (s->P.colour_space && !getenv("GM_POST_SW_HOST")) {
    // The per-colour error rates post_sw derives from quality values (ref: sw-post.c:486-491, pr_err_from_qv util.h:285-293; Sanger QVs, the binary's default),
    // tabulated here with the host's libm for every QV the formula distinguishes: the device kernel reads the very doubles the host routine computes.
    const std::vector<double> qt = cs_qv_table(true);
    GM_HIP_S(hipMalloc(&s->d_qtab, qt.size() * 8));
    GM_HIP_S(hipMemcpy(s->d_qtab, qt.data(), qt.size() * 8, hipMemcpyHostToDevice));
  }
  s->max_batch = std::max(64, std::min(max_batch_reads > 0 ? max_batch_reads : 131072, 1 << 20));
  if (const char* e = gm_tune("GM_P2_GRID")) s->p2_grid = std::max(64, std::min(65536, atoi(e)));
  // The front stream gets the higher queue priority: K1's fall-back kernels (a few workgroups that each want most of a CU's LDS) otherwise wait for milliseconds
  // behind the back stream's thousands of small pass-1 workgroups, which refill every CU the moment the persistent K1 grid has left it.
  { int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (getenv("GM_STREAM_PRIO_OFF") || hi == lo) { GM_HIP_S(hipStreamCreate(&s->stream)); }
    else GM_HIP_S(hipStreamCreateWithPriority(&s->stream, hipStreamDefault, hi)); }
  GM_HIP_S(hipStreamCreateWithFlags(&s->stream_b, hipStreamNonBlocking));
  GM_HIP_S(hipStreamCreateWithFlags(&s->stream_c, hipStreamNonBlocking));
  for (auto& e : s->ev) GM_HIP_S(hipEventCreate(&e));
  for (auto& row : s->pev) for (auto& e : row) GM_HIP_S(hipEventCreate(&e));
  for (auto& row : s->pkev) for (auto& e : row) GM_HIP_S(hipEventCreate(&e));
  GM_HIP_S(hipMalloc(&s->d_stats, (size_t)GS_STRIPES * GS_STRIDE * 8));
  for (auto& d : s->d_pstats) GM_HIP_S(hipMalloc(&d, (size_t)GS_STRIPES * GS_STRIDE * 8));
  GM_HIP_S(hipHostMalloc((void**)&s->h_pin, (16 + 1024) * 4, hipHostMallocDefault));
  memset(s->h_pin, 0, (16 + 1024) * 4);
  { const int rc = gm_index_derive_rna(const_cast<gm_index*>(ix), s->stream); if (rc) { gm_session_free(s); return rc; } }      // which contigs are RNA (once per index)
  // k_lookup_v5 streams large indexes with the help of per-list strip lists, derived once per index (not stored in the index files)
  if (k1_strips_wanted(ix->n_slabs, ix->params.region_bits, gm_k1_tune())) {
    const int rc = gm_index_derive_strips(const_cast<gm_index*>(ix), s->stream);
    if (rc) { gm_session_free(s); return rc; }
  }
  *out = s;
  return GM_OK;
#undef GM_HIP_S
}
extern "C" void gm_session_free(gm_session_t* s) {
  if (!s) return;
  if (s->twin) { gm_session_free(s->twin); s->twin = nullptr; }
  (void)hipSetDevice(s->ix->device);
  for (auto& v : s->pin_res) v.release();
  for (auto& v : s->pin_ops) v.release();
  free_buffers(s->set[0]); free_buffers(s->set[1]); free_buffers(s->set2[0]); free_buffers(s->set2[1]);
  s->k1.release();
  for (auto& h : s->slot) slot_free(h);
  if (s->d_qtab) (void)hipFree(s->d_qtab);
  if (s->d_pairs) (void)hipFree(s->d_pairs);
  if (s->d_pair_cnt) (void)hipFree(s->d_pair_cnt);
  if (s->d_stats) (void)hipFree(s->d_stats);
  for (auto& d : s->d_pstats) if (d) (void)hipFree(d);
  if (s->h_pin) (void)hipHostFree(s->h_pin);
  for (auto& e : s->ev) if (e) (void)hipEventDestroy(e);
  for (auto& row : s->pev) for (auto& e : row) if (e) (void)hipEventDestroy(e);
  for (auto& row : s->pkev) for (auto& e : row) if (e) (void)hipEventDestroy(e);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  if (s->stream_b) (void)hipStreamDestroy(s->stream_b);
  if (s->stream_c) (void)hipStreamDestroy(s->stream_c);
  delete s;
}

#include "gm_host_finalize.inc"
#include "gm_host_records.inc"

// Heavy tier of K2: the few read-strands whose survivors exceed the LDS tier (low-complexity reads,
// repeats).  Sizes are known now, so every array is allocated exactly, the keys are re-emitted by K1
// and sorted by one segmented radix sort; then K2 runs on global arrays.  Rare by construction.
// the view a kernel that reads the reads of set D gets: with that set's RNA flags (letter space; null in colour space)
static inline GmIndexDev gm_view_of(const GmIndexDev& dv, const DevSet& D) { GmIndexDev v = dv; v.read_rna = D.d_read_rna; return v; }

static int run_heavy_tier(gm_session* s, DevSet& D, const GmIndexDev& dv, int n, int read_len, int read_words, int W, int n_heavy,
                          unsigned long long* d_stats = nullptr, const GmScoreDev* sc = nullptr) {
  if (!sc) sc = &s->sc;
  hipStream_t q = s->stream;
  if (!d_stats) d_stats = s->d_stats;
  std::vector<uint32_t> list(n_heavy), cnt_all((size_t)n * 2);
  GM_HIP(hipMemcpyAsync(list.data(), D.d_heavy_list, (size_t)n_heavy * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipMemcpyAsync(cnt_all.data(), D.d_surv_cnt, cnt_all.size() * 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipStreamSynchronize(q));
  std::sort(list.begin(), list.end());
  std::vector<uint64_t> off(n_heavy + 1); std::vector<uint32_t> segn(n_heavy), b32(n_heavy), e32(n_heavy);
  uint64_t tot = 0;
  for (int i = 0; i < n_heavy; i++) {
    const uint32_t c = cnt_all[list[i]];
    off[i] = tot; segn[i] = c; b32[i] = (uint32_t)tot; e32[i] = (uint32_t)(tot + c);
    tot += (uint64_t)std::max(64, pow2ceil(c));       // room for the padded window sort
  }
  off[n_heavy] = tot;
  if (tot >= (1ull << 32)) { gm_set_error("heavy tier: %llu keys in one sub-batch", (unsigned long long)tot); return GM_E_OVERFLOW; }
  uint32_t *d_list = nullptr, *d_segn = nullptr, *d_b32 = nullptr, *d_e32 = nullptr, *d_aux = nullptr, *d_nxt = nullptr, *d_ord = nullptr;
  uint64_t *d_off = nullptr, *d_kin = nullptr, *d_ks = nullptr; GmDevMem mem;      // (mem's scope ends behind the synchronise below)
  GM_HIP(mem.get(&d_list, (size_t)n_heavy * 4)); GM_HIP(mem.get(&d_segn, (size_t)n_heavy * 4)); GM_HIP(mem.get(&d_b32, (size_t)n_heavy * 4)); GM_HIP(mem.get(&d_e32, (size_t)n_heavy * 4));
  GM_HIP(mem.get(&d_off, (size_t)(n_heavy + 1) * 8));
  GM_HIP(mem.get(&d_kin, tot * 8)); GM_HIP(mem.get(&d_ks, tot * 8)); GM_HIP(mem.get(&d_aux, tot * 4)); GM_HIP(mem.get(&d_nxt, tot * 4)); GM_HIP(mem.get(&d_ord, tot * 4));
  GM_HIP(hipMemcpyAsync(d_list, list.data(), (size_t)n_heavy * 4, hipMemcpyHostToDevice, q));
  GM_HIP(hipMemcpyAsync(d_segn, segn.data(), (size_t)n_heavy * 4, hipMemcpyHostToDevice, q));
  GM_HIP(hipMemcpyAsync(d_b32, b32.data(), (size_t)n_heavy * 4, hipMemcpyHostToDevice, q));
  GM_HIP(hipMemcpyAsync(d_e32, e32.data(), (size_t)n_heavy * 4, hipMemcpyHostToDevice, q));
  GM_HIP(hipMemcpyAsync(d_off, off.data(), (size_t)(n_heavy + 1) * 8, hipMemcpyHostToDevice, q));
  GM_HIP(hipMemsetAsync(d_ks, 0xff, tot * 8, q));
  int rc = gm_launch_lookup_redo(gm_view_of(dv, D), D.d_reads, n, read_len, read_words, n_heavy, d_list, d_off, d_kin, d_stats, q);
  if (rc == GM_OK)
    rc = gm_launch_anchors_heavy(dv, *sc, n, read_len, W, n_heavy, d_list, d_off, d_segn, d_b32, d_e32, tot, d_kin, d_ks, d_aux, d_nxt, d_ord,
                                 D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, d_stats, q);
  GM_HIP(hipStreamSynchronize(q));      // (also behind a launch that failed)
  return rc;
}

// tight-cluster bound of the prune rules (gm_prune.hip): smallest window-generation threshold over all contigs, in survivors' x extent
static int prune_e_max(const gm_session* s, int read_len, int W) {
  int e_max = -1;
  if (gm_tune("GM_PRUNE_NO_RULE2")) return e_max;
  if (s->sc.match > 0 && s->sc.b_go >= 0 && s->sc.b_ge >= 0) {
    long long min_clen = 1ll << 40;
    for (int c = 0; c < s->ix->n_contigs; c++) min_clen = std::min<long long>(min_clen, (long long)s->ix->contig_off[c + 1] - s->ix->contig_off[c]);
    const int w_len = (int)std::min<long long>(W, min_clen);
    const int base = std::min(read_len, w_len) * s->sc.match;
    const int thr = s->sc.wgen_thr_frac < 0 ? s->sc.wgen_abs : (int)((double)base * s->sc.wgen_thr_frac);
    e_max = (thr + s->sc.match - 1) / s->sc.match - s->ix->max_seed_span - 1;
  }
  return e_max;
}

// K1 with K1b's prune fused where the chosen kernel can (k_lookup_v5); *fused tells launch_prune_anchors to skip K1b
static int launch_lookup(gm_session* s, DevSet& D, const GmIndexDev& dv, int n, int read_len, int read_words, int W, unsigned long long* d_stats, int* fused) {
  GmFusePrune f; f.d_surv2 = D.d_surv2; f.d_surv_cnt2 = D.d_surv_cnt2; f.scap2 = D.scap2; f.window_len = W; f.e_max = D.scap2 > 0 ? prune_e_max(s, read_len, W) : -1; f.fused = fused;
  *fused = 0;
  return gm_launch_lookup(gm_view_of(dv, D), D.d_reads, n, read_len, read_words, D.d_surv, D.d_surv_cnt, D.scap, D.d_heavy_list, D.d_heavy_cnt, 2 * D.eff_batch, d_stats, s->stream, &s->k1, D.d_surv_seg, &f);
}

// K1b + K2 on the survivors of K1
static int launch_prune_anchors(gm_session* s, DevSet& D, const GmIndexDev& dv, int n, int read_len, int W, unsigned long long* d_stats = nullptr, int fused = 0) {
  hipStream_t q = s->stream;
  if (!d_stats) d_stats = s->d_stats;
  if (D.scap2 > 0) {
    if (!fused) {
      const int e_max = prune_e_max(s, read_len, W);
      int rc = gm_launch_prune(n, read_len, W, e_max, s->ix->n_slabs, s->ix->slab_bits, D.d_surv, D.d_surv_cnt, D.d_surv_seg, D.scap, D.d_surv2, D.d_surv_cnt2, D.scap2, D.d_heavy_list, D.d_heavy_cnt, 2 * D.eff_batch, d_stats, q, &s->k1);
      if (rc) return rc;
    }
    return gm_launch_anchors(dv, s->sc, n, read_len, W, D.d_surv2, D.d_surv_cnt2, D.scap2, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, d_stats, q);
  }
  return gm_launch_anchors(dv, s->sc, n, read_len, W, D.d_surv, D.d_surv_cnt, D.scap, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, d_stats, q);
}

// One sub-batch on the device, in two halves that run on different streams so that the back of sub-batch i (pass 1 and 2: VALU-bound,
// 56-64 VGPRs, ~1 KB of LDS per wave) shares the CUs with the front of sub-batch i + 1 (K1: one 1 024-thread workgroup per CU that waits on
// memory most of the time and leaves 96 VGPRs per SIMD and 26 KB of LDS free).  Each half uses the buffer set k of its sub-batch only.
//
// the index as the kernels see it, with the session's per-call switches: -n 1 keeps every list entry (use_region_counts off, ref: gmapper.c:2610-2616)
static GmIndexDev session_view(const gm_session* s, const DevSet* D = nullptr) {
  GmIndexDev dv = s->ix->dev_view(); dv.no_region_counts = s->P.match_mode == 1 ? 1 : 0;
  if (D) dv.read_rna = D->d_read_rna;                        // (letter space: the flags k_read_rna_flags left for this sub-batch's reads)
  return dv;
}

// Front, stream A: K1, K1b, K2; nothing here waits on the host (the heavy count lands in pinned memory, event pev[k][6] marks the end).
static int pipeline_front(gm_session* s, int k, int n, int read_len) {
  DevSet& D = s->set[k];
  const GmIndexDev dv = session_view(s);
  const int read_words = (read_len + 7) / 8;
  const int W = window_len_of(s->P, read_len);
  hipStream_t q = s->stream;
  unsigned long long* d_stats = s->d_pstats[k];
  GM_HIP(hipMemsetAsync(d_stats, 0, (size_t)GS_STRIPES * GS_STRIDE * 8, q));
  GM_HIP(hipEventRecord(s->pev[k][0], q));
  if (D.d_read_rna) { const int rc0 = gm_launch_read_rna_flags(D.d_reads, n, read_len, read_words, D.d_read_rna, q); if (rc0) return rc0; }      // which reads are RNA (ref: fasta.c:528-542)
  s->k1.start_flags = s->h_pin + 16; s->k1.flag_cap = 1024; s->k1.epoch = ++s->flag_epoch;
  int fused = 0;
  int rc = launch_lookup(s, D, dv, n, read_len, read_words, W, d_stats, &fused);
  s->front_epoch[k] = s->flag_epoch; s->front_flag_grid[k] = rc ? 0 : s->k1.flag_grid;
  s->k1.start_flags = nullptr; s->k1.flag_cap = 0;     // (the paired path's lookups raise no flags)
  if (rc) return rc;
  GM_HIP(hipEventRecord(s->pev[k][1], q));
  rc = launch_prune_anchors(s, D, dv, n, read_len, W, d_stats, fused);
  if (rc) return rc;
  GM_HIP(hipMemcpyAsync(&s->h_pin[k], D.d_heavy_cnt, 4, hipMemcpyDeviceToHost, q));
  GM_HIP(hipEventRecord(s->pev[k][2], q));
  GM_HIP(hipEventRecord(s->pev[k][6], q));
  return GM_OK;
}

// the folded device counters of one sub-batch (hs[GS_N]) into the call's statistics: unpaired and paired mode alike
static void add_device_stats(gm_map_stats_t* st, const unsigned long long* hs) {
  st->lookups += hs[GS_LOOKUPS]; st->list_entries += hs[GS_ENTRIES]; st->list_bytes += 12ull * hs[GS_LOOKUPS] + 4ull * hs[GS_ENTRIES];
  st->survivors += hs[GS_SURVIVORS]; st->anchors += hs[GS_ANCHORS]; st->windows += hs[GS_WINDOWS];
  st->vec_calls += hs[GS_VEC_CALLS]; st->vec_cells += hs[GS_VEC_CELLS]; st->vec_bypassed += hs[GS_VEC_BYPASSED];
  st->full_calls += hs[GS_FULL_CALLS]; st->full_cells += hs[GS_FULL_CELLS]; st->exact_order_reads += hs[GS_EXACT_ORDER]; st->survivors_pruned += hs[GS_PRUNED];
}

// the striped stage counters as the device leaves them (raw[GS_STRIPES][GS_STRIDE]) into one row hs[GS_N]
static void fold_stats(const unsigned long long* raw, unsigned long long* hs) { for (int c = 0; c < GS_N; c++) { hs[c] = 0; for (int t = 0; t < GS_STRIPES; t++) hs[c] += raw[(size_t)t * GS_STRIDE + c]; } }
// sw_full_cs_setup's arguments (ref: gmapper.c:2944-2947)
static void cs_setup_args(const gm_params_t& P, int* cs9) {
  const int c9[9] = {P.match_score, P.mismatch_score, P.crossover_score, -P.a_gap_open_score, -P.a_gap_extend_score, -P.b_gap_open_score, -P.b_gap_extend_score, P.anchor_width, P.indel_taboo_len};
  memcpy(cs9, c9, sizeof c9);
}
// set 0 for unpaired reads of this length: kept when it has that length and unpaired capacities, else chosen and allocated anew
static int prepare_unpaired_set(gm_session* s, int read_len) {
  DevSet& D = s->set[0];
  if (D.cur_len == read_len && (D.caps_pair_mode == 0 || D.caps_pair_mode == 4)) return GM_OK;
  choose_caps(s, D, read_len); D.caps_pair_mode = 0;
  return alloc_buffers(s, D, read_len);
}
static double gm_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static const int GM_REDO = 1;     // a stage's answer besides GM_OK and the error codes: the sub-batch is run again from its front

namespace {
// Back, stream B, of the sub-batch whose front ran on set k: its stages in the order they are called, and what they share.  Each returns GM_OK or an error; grow also
// GM_REDO (the buffers of set k were re-allocated: the caller re-submits the sub-batch from the front).  Between copy_out and finish_back nothing of this set that the
// FRONT writes is read any more, so the caller may queue the front of the sub-batch after next onto it there (ReadRun::back).
struct BackStages {
  gm_session* s; int k; HostSlot& H; int n, read_len; gm_map_stats_t* st;
  DevSet& D = s->set[k]; const GmIndexDev dv = session_view(s); int read_words = (read_len + 7) / 8, W = window_len_of(s->P, read_len);
  hipStream_t q = s->stream_b; unsigned long long* d_stats = s->d_pstats[k];
  uint32_t n_work = 0; unsigned long long hs[GS_N]; float ms[5];      // pass 2's work items, the folded counters, the five stage times
  std::vector<unsigned long long> hraw = std::vector<unsigned long long>((size_t)GS_STRIPES * GS_STRIDE);
  size_t rcap() const { return (size_t)D.eff_batch * D.rcap_per_read; }
  // the front's end and times, the heavy tier if any (stream A, rare); next_front_queued: the other set's front is in flight
  int wait_front(bool next_front_queued) {
    GM_HIP(hipEventSynchronize(s->pev[k][6]));
    const uint32_t n_heavy = s->h_pin[k];
    GM_HIP(hipEventElapsedTime(&ms[0], s->pev[k][0], s->pev[k][1]));      // (the front's times now: its events are recorded again when this set takes the sub-batch after next)
    GM_HIP(hipEventElapsedTime(&ms[1], s->pev[k][1], s->pev[k][2]));
    if (n_heavy) { int rc = run_heavy_tier(s, D, dv, n, read_len, read_words, W, (int)n_heavy, d_stats); if (rc) return rc; GM_HIP(hipEventRecord(s->pev[k][6], s->stream)); }
    GM_HIP(hipStreamWaitEvent(q, s->pev[k][6], 0));
    if (next_front_queued && s->front_flag_grid[k ^ 1] > 0) {
      // K1 of the next sub-batch becomes runnable at the same moment as this pass 1.  Its persistent workgroups need a whole CU's LDS each; pass-1 waves
      // that get there first keep them off the CUs until pass 1 is over.  So: wait (bounded) until all of them have raised their flag.
      volatile uint32_t* f = s->h_pin + 16; const uint32_t want = s->front_epoch[k ^ 1]; const int g = s->front_flag_grid[k ^ 1];
      const double t0 = gm_now_ms();
      for (int up = 0; up < g && gm_now_ms() - t0 <= 5.0;) { up = 0; for (int i = 0; i < g; i++) up += f[i] == want; }
    }
    return GM_OK;
  }
  int pass1_select() {
    const int overlap_abs = (int)(unsigned int)(s->P.window_overlap < 0 ? -s->P.window_overlap : W * (s->P.window_overlap / 100.0));   // ref: mapping.c:1289
    GM_HIP(hipEventRecord(s->pev[k][3], q));
    int rc = gm_launch_pass1(gm_view_of(dv, D), s->sc, D.d_reads, n, read_len, read_words, W, overlap_abs, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, D.d_slots, d_stats, q,
                             nullptr, nullptr, D.d_initbp, true); if (rc) return rc;
    GM_HIP(hipEventRecord(s->pev[k][4], q));
    rc = gm_launch_select(s->sc, n, read_len, D.d_hits, D.d_perm, D.d_hit_cnt, D.hcap, D.d_sel, D.d_sel_cnt, D.d_sel_off, D.d_work, D.d_n_work, q); if (rc) return rc;
    GM_HIP(hipEventRecord(s->pev[k][5], q));
    GM_HIP(hipMemcpyAsync(&n_work, D.d_n_work, 4, hipMemcpyDeviceToHost, q));
    GM_HIP(hipMemcpyAsync(hraw.data(), d_stats, hraw.size() * 8, hipMemcpyDeviceToHost, q));
    GM_HIP(hipStreamSynchronize(q));
    fold_stats(hraw.data(), hs);
    return GM_OK;
  }
  int grow() {
    bool retry = false;
    if (hs[GS_OVERFLOW_SURV]) { gm_set_error("heavy list overflow"); return GM_E_OVERFLOW; }
    if (hs[GS_OVERFLOW_HITS]) { if (D.hcap >= 32768) { gm_set_error("window list overflow at capacity %d", D.hcap); return GM_E_OVERFLOW; } D.hcap *= 4; retry = true; }
    if (n_work > rcap()) { if (D.rcap_per_read >= 32) { gm_set_error("pass-2 work overflow"); return GM_E_OVERFLOW; } D.rcap_per_read = std::min(32, D.rcap_per_read * 2); retry = true; }
    if (!retry) return GM_OK;
    // capacities grew: re-allocate and let the caller re-submit (the sub-batch size may have shrunk)
    if (st) st->retries++;
    GM_HIP(hipStreamSynchronize(s->stream));           // the other set's front may be in flight; nothing may touch freed buffers
    const int rc = alloc_buffers(s, D, read_len);
    return rc ? rc : GM_REDO;
  }
  int pass2() {
    int rc; if (s->P.colour_space) {
      int cs9[9]; cs_setup_args(s->P, cs9);
      rc = gm_launch_pass2_cs(dv, s->sc, cs9, D.d_reads, D.d_initbp, n, read_len, read_words, W, D.d_hits, D.hcap, D.d_sel, D.d_work, D.d_n_work,
                              D.d_res, D.d_ops, D.ops_stride, (uint32_t*)D.d_back, D.back_stride / 4, D.p2_grid, d_stats, q, D.xover_on ? D.d_xover : nullptr, nullptr, D.d_p2_order, D.d_p2_cls);
      // post_sw of every result on the device (with the reads' quality values where they have them: per-colour error rates from the host's table, base qualities back), unless
      // the alignment is local (no mapping qualities at all, ref: gmapper.c:2325-2328)
      H.post_on = rc == GM_OK && D.d_post && gm_mqv_on(s->P) && (!D.xover_on || s->d_qtab);
      H.post_bq_on = H.post_on && D.xover_on;
      if (H.post_on) {
        const CsPostConsts c = cs_post_consts(s);
        GmCsPostDev K; K.let_m = c.let_m; K.let_x = c.let_x; K.col_m[0] = c.col_m[0]; K.col_m[1] = c.col_m[1]; K.col_x[0] = c.col_x[0]; K.col_x[1] = c.col_x[1];
        K.pr_del_open = c.pr_del_open; K.pr_del_extend = c.pr_del_extend; K.pr_ins_open = c.pr_ins_open; K.pr_ins_extend = c.pr_ins_extend;
        K.qv = H.post_bq_on ? D.d_qv : nullptr; K.qtab = H.post_bq_on ? s->d_qtab : nullptr; K.bq = H.post_bq_on ? D.d_post_bq : nullptr;
        rc = gm_launch_post_sw_cs(K, D.d_reads, D.d_initbp, read_len, read_words, D.d_res, D.d_ops, D.ops_stride, D.d_n_work, (uint32_t)rcap(), D.d_post, D.d_post_fw, D.d_post_info,
                                  D.post_threads, q);
      }
    } else {
      rc = gm_launch_pass2(gm_view_of(dv, D), s->sc, D.d_reads, n, read_len, read_words, W, D.d_hits, D.d_perm, D.hcap, D.d_sel, D.d_sel_cnt, D.d_work, D.d_n_work,
                           D.d_res, D.d_ops, D.ops_stride, D.d_back, D.back_stride, D.p2_grid, d_stats, q, nullptr, 0, 0, D.d_p2_order, D.d_p2_cls);
      H.post_on = false;
    }
    if (rc) return rc;
    if (!H.post_on) H.post_bq_on = false;
    GM_HIP(hipEventRecord(s->pev[k][7], q));
    return GM_OK;
  }
  // the results to the host slot
  int copy_out() {
    int rc; size_t cap;
    cap = H.res_cap; rc = slot_reserve((void**)&H.res, &cap, (size_t)n_work * sizeof(GmFullRes)); H.res_cap = cap; if (rc) return rc;
    cap = H.ops_cap; rc = slot_reserve((void**)&H.ops, &cap, (size_t)n_work * D.ops_stride); H.ops_cap = cap; if (rc) return rc;
    cap = H.n_cap; rc = slot_reserve((void**)&H.sel_cnt, &cap, (size_t)n * 4); if (rc) return rc;
    cap = H.n_cap; rc = slot_reserve((void**)&H.sel_off, &cap, (size_t)n * 4); H.n_cap = cap; if (rc) return rc;
    H.n_work = n_work;
    if (H.post_on) { cap = H.post_cap; rc = slot_reserve((void**)&H.post, &cap, (size_t)n_work * sizeof(GmPostRes)); H.post_cap = cap; if (rc) return rc; }
    if (H.post_bq_on) { cap = H.post_bq_cap; rc = slot_reserve((void**)&H.post_bq, &cap, (size_t)n_work * read_len + 64); H.post_bq_cap = cap; if (rc) return rc; }
    // The stage counters first, then an event: from there on nothing of this set that the FRONT writes is read any more (the copies below take d_res / d_ops / d_sel_* /
    // d_post only), so the front of the sub-batch after next may be queued onto this set before the host waits for the results.
    cap = H.stats_cap; rc = slot_reserve((void**)&H.stats, &cap, hraw.size() * 8); H.stats_cap = cap; if (rc) return rc;
    GM_HIP(hipMemcpyAsync(H.stats, d_stats, hraw.size() * 8, hipMemcpyDeviceToHost, q));
    if (H.want_reads) {                                              // reads handed over in device memory: the host's finalisation needs this sub-batch's letters too
      cap = H.reads_cap; rc = slot_reserve((void**)&H.reads, &cap, (size_t)n * read_words * 4); H.reads_cap = cap; if (rc) return rc;
      GM_HIP(hipMemcpyAsync(H.reads, D.d_reads, (size_t)n * read_words * 4, hipMemcpyDeviceToHost, q));
    }
    GM_HIP(hipEventRecord(s->pev[k][9], q));
    if (n_work) {
      if (H.post_on) GM_HIP(hipMemcpyAsync(H.post, D.d_post, (size_t)n_work * sizeof(GmPostRes), hipMemcpyDeviceToHost, q));
      if (H.post_bq_on) GM_HIP(hipMemcpyAsync(H.post_bq, D.d_post_bq, (size_t)n_work * read_len, hipMemcpyDeviceToHost, q));
      GM_HIP(hipMemcpyAsync(H.res, D.d_res, (size_t)n_work * sizeof(GmFullRes), hipMemcpyDeviceToHost, q));
      GM_HIP(hipMemcpyAsync(H.ops, D.d_ops, (size_t)n_work * D.ops_stride, hipMemcpyDeviceToHost, q));
    }
    GM_HIP(hipMemcpyAsync(H.sel_cnt, D.d_sel_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, q));
    GM_HIP(hipMemcpyAsync(H.sel_off, D.d_sel_off, (size_t)n * 4, hipMemcpyDeviceToHost, q));
    return GM_OK;
  }
  int finish_back(float* lookup_ms) {
    GM_HIP(hipStreamSynchronize(q));
    fold_stats(H.stats, hs);
    GM_HIP(hipEventElapsedTime(&ms[2], s->pev[k][3], s->pev[k][4]));
    GM_HIP(hipEventElapsedTime(&ms[3], s->pev[k][4], s->pev[k][5]));
    GM_HIP(hipEventElapsedTime(&ms[4], s->pev[k][5], s->pev[k][7]));
    *lookup_ms = ms[0];
    if (st) { add_device_stats(st, hs); st->ms_lookup += ms[0]; st->ms_anchors += ms[1]; st->ms_pass1 += ms[2]; st->ms_select += ms[3]; st->ms_pass2 += ms[4]; }
    s->last_lookup_bytes += 12ull * hs[GS_LOOKUPS] + 4ull * hs[GS_ENTRIES];
    return GM_OK;
  }
  // the first five stages, as far as the queued result copies
  int through_copy_out(bool next_front_queued) {
    int rc = wait_front(next_front_queued); if (!rc) rc = pass1_select(); if (!rc) rc = grow(); if (!rc) rc = pass2();
    return rc ? rc : copy_out();
  }
};
}  // namespace

// both halves back to back on set 0 (stage dumps)
static int run_device_pipeline(gm_session* s, HostSlot& H, int n, int read_len, float* lookup_ms) {
  BackStages B{s, 0, H, n, read_len, nullptr};
  int rc = pipeline_front(s, 0, n, read_len); if (!rc) rc = B.through_copy_out(false);
  return rc ? rc : B.finish_back(lookup_ms);
}

// Admission of mapping calls per device: at most TWO in flight on a device (a single call already fills the GPU), e.g. the two sessions the file entry alternates its
// chunks between -- the tail of one call, its last back half and host work, then runs under the other's lookups.  A third call waits until one of them returns.
// Sessions on different devices run side by side.  (Each session owns its launch scratch, GmK1Scratch: the calls share no buffers.)
struct GmDevTurn {
  static std::mutex& m(int d) { static std::mutex a[16]; return a[d]; }
  static std::condition_variable& cv(int d) { static std::condition_variable a[16]; return a[d]; }
  static int& in_flight(int d) { static int a[16] = {}; return a[d]; }
  int dev;
  explicit GmDevTurn(const gm_session* s) : dev((int)((unsigned)s->ix->device & 15u)) {
    std::unique_lock<std::mutex> lk(m(dev));
    cv(dev).wait(lk, [&] { return in_flight(dev) < 2; });
    in_flight(dev)++;
  }
  ~GmDevTurn() { { std::lock_guard<std::mutex> lk(m(dev)); in_flight(dev)--; } cv(dev).notify_one(); }
  GmDevTurn(const GmDevTurn&) = delete; GmDevTurn& operator=(const GmDevTurn&) = delete;
};

// ---- per-call set-up that map_impl and map_pairs_impl (gm_host_pairs.inc) share ----
static const char* line_end(const char* p) { const char* e = strchr(p, '\n'); return e ? e : p + strlen(p); }
// The first n lines of a text block: ptr gets each line's start, len (or null) its length.  want >= 0: every line has that many characters, or the call fails with the
// caller's message -- bad_len_fmt takes the line's number, its length and want, in that order
static int split_lines(const char* text, int n, std::vector<const char*>& ptr, std::vector<int>* len, int want = -1, const char* bad_len_fmt = nullptr) {
  for (int i = 0; i < n; i++) {
    const char* p = text; const char* e = line_end(p);
    if (want >= 0 && (int)(e - p) != want) { gm_set_error(bad_len_fmt, i, (int)(e - p), want); return GM_E_ARG; }
    ptr.push_back(p); if (len) len->push_back((int)(e - p)); text = *e ? e + 1 : e;
  }
  return GM_OK;
}
// per-position crossover scores of n colour-space reads from their QUAL strings (ref: gmapper.c:532-544); qv (or null): also the clamped quality values
static void xover_from_quals(const gm_session* s, const char* const* quals, int n, int read_len, int qual_delta, int8_t* xover, uint8_t* qv_out) {
  for (int i = 0; i < n; i++) {
    const char* q = quals[i];
    for (int j = 0; j < read_len; j++) {
      const int qv = (int)q[j] - qual_delta;
      if (qv_out) qv_out[(size_t)i * read_len + j] = (uint8_t)std::min(250, std::max(0, qv));   // what post_sw's error-rate formula distinguishes (qv <= 0, qv >= 250, ref: util.h:285-293)
      const double pe = qv <= 0 ? .99999999 : (qv >= 250 ? 1E-25 : pow(10.0, -(double)qv / 10.0));   // pr_err_from_qv, ref: util.h:285-293
      int cx = (int)(s->score_alpha * log(pe / 3.0) / log(2.0));
      if (cx > -1) cx = -1; else if (cx < 2 * s->P.crossover_score) cx = 2 * s->P.crossover_score;
      xover[(size_t)i * read_len + j] = (int8_t)cx;
    }
  }
}
// the SHRiMP / pretty formats and the ZE:Z edit string print genome letters: one download per session
static int ensure_host_genome(gm_session* s) {
  if (!(s->P.output_format || s->P.extra_sam_fields) || !s->h_genome.empty()) return GM_OK;
  s->h_genome.resize(s->ix->genome_words);
  GM_HIP(hipMemcpy(s->h_genome.data(), s->ix->d_genome, s->ix->genome_words * 4, hipMemcpyDeviceToHost));
  return GM_OK;
}
// The front's own limit on the read length.  K1b's list-mode kernel (k_prune, gm_launch_prune) takes gm_prune_lds bytes of LDS for twice the survivor capacity choose_caps
// gives reads of this length; beyond a CU's LDS its launch fails in the middle of the front.  The same arithmetic here, before anything is uploaded: on a small index
// this binds long before the alignment kernel's LDS does.  0: the session's front runs no K1b (pair_mode as choose_caps takes it).
static size_t pass2_front_prune_lds(const gm_session* s, int read_len, int pair_mode = 0) {
  DevSet D; choose_caps(s, D, read_len, pair_mode);
  if (D.scap2 <= 0) return 0;
  return gm_prune_lds(D.scap, s->ix->n_slabs);      // (every buffer set has its d_surv_seg: the launcher's segments are the slabs)
}
static int check_read_len(const gm_session* s, int read_len, int pair_mode = 0) {
  if (read_len > s->P.longest_read_len || read_len >= 32768 / std::max(1, s->P.match_score)) { gm_set_error("read length %d out of range (ref: sw-vector.c:393-398)", read_len); return GM_E_RANGE; }
  const size_t prune_lds = pass2_front_prune_lds(s, read_len, pair_mode);
  if (prune_lds > GM_SWF_LDS_LIMIT) {
    gm_set_error("reads of %d positions: the front's prune kernel needs %zu bytes of LDS on this index and seed set, beyond the %zu of a CU", read_len, prune_lds, (size_t)GM_SWF_LDS_LIMIT);
    return GM_E_RANGE;
  }
  // the window of these reads (window_len_of, before its cut to 16 bits) against what pass 2 can take: nothing is uploaded for a window beyond it
  const double w = s->P.window_len < 0 ? -s->P.window_len : read_len * (s->P.window_len / 100.0);
  const int w_max = gm_pass2_max_window(s->P.colour_space ? 1 : 0, s->P.local_alignment ? 1 : 0, read_len);
  if (w > (double)w_max) { gm_set_error("window length %.0f for reads of %d: beyond the %d columns pass 2 has LDS for", w, read_len, w_max); return GM_E_RANGE; }
  return GM_OK;
}

namespace {                                                    // (the call's own types: nothing of them is exported)
// One gm_map_reads call: what init() settles before the first sub-batch and nothing changes after it (the job threads read it beside the calling thread).
struct ReadCall {
  gm_session* s = nullptr; int n_reads = 0, read_len = 0, read_words = 0; gm_map_stats_t* stats = nullptr;
  const uint32_t* reads_host = nullptr; const void* reads_dev = nullptr; const uint8_t* initbp = nullptr;      // the reads: in host memory (with the primer letters in colour space) or on the device
  std::vector<const char*> nptr, qptr, sptr; std::vector<int> nlen; bool named = false, quals = false, seq_text = false;      // name, QUAL and text line of every read
  int qual_delta = 33, emit_sam = 0, nthreads = 1, ops_stride = 0, ramp_min = 8192; uint32_t* per_read_bytes = nullptr;
  bool overlap = false, timeline = false; const char* guard_tol = nullptr;      // guard_tol: GM_POST_GUARD_TOL (tests: a huge tolerance sends every result through the redo path)
  static int check_args(const gm_session* s, int n_reads, int read_len, const uint8_t* initbp_host) {
    if (!s || n_reads < 0 || read_len < 1) { gm_set_error("gm_map_reads: bad arguments"); return GM_E_ARG; }
    if ((s->P.colour_space != 0) != (initbp_host != nullptr)) { gm_set_error(s->P.colour_space ? "colour-space session: use gm_map_reads_cs (colours + primer letters)" : "gm_map_reads_cs needs a colour-space session"); return GM_E_ARG; }
    return check_read_len(s, read_len);
  }
  int lines_of(const char* text, int want, std::vector<const char*>& ptr, const char* bad_len_fmt) const {      // one line of `want` characters per read
    if (!gm_fixed_lines(text, (size_t)n_reads, (size_t)want)) return split_lines(text, n_reads, ptr, nullptr, want, bad_len_fmt);
    ptr.resize(n_reads); for (int i = 0; i < n_reads; i++) ptr[i] = text + (size_t)i * ((size_t)want + 1);      // (the usual case: no search for the line ends)
    return GM_OK;
  }
  int match_sets(int from) const {                             // give the other set the capacities of set `from`
    DevSet& a = s->set[from]; DevSet& b = s->set[from ^ 1];
    if (a.cur_len == b.cur_len && a.scap == b.scap && a.scap2 == b.scap2 && a.hcap == b.hcap && a.rcap_per_read == b.rcap_per_read && a.eff_batch == b.eff_batch && b.d_pmin == nullptr) return GM_OK;
    b.scap = a.scap; b.scap2 = a.scap2; b.hcap = a.hcap; b.rcap_per_read = a.rcap_per_read;
    return alloc_buffers(s, b, read_len);
  }
  // the set-up, behind check_args and the device's turn (map_impl)
  int init(gm_session* s_, int n_reads_, int read_len_, const uint32_t* reads_host_, const void* reads_dev_, const char* names, int emit_sam_, gm_map_stats_t* stats_,
           const uint8_t* initbp_host, const char* quals_, int qual_delta_, const char* seq, uint32_t* per_read_bytes_) {
    s = s_; n_reads = n_reads_; read_len = read_len_; reads_host = reads_host_; reads_dev = reads_dev_; emit_sam = emit_sam_; stats = stats_; initbp = initbp_host;
    qual_delta = qual_delta_; per_read_bytes = per_read_bytes_; named = names != nullptr; quals = quals_ != nullptr; seq_text = seq != nullptr;
    GM_HIP(hipSetDevice(s->ix->device));
    if (stats) memset(stats, 0, sizeof *stats);
    read_words = (read_len + 7) / 8;
    int rc = prepare_unpaired_set(s, read_len); if (!rc) rc = ensure_host_genome(s); if (rc) return rc;
    s->last_lookup_ms = 0; s->last_lookup_bytes = 0; s->last_lookup_launches = 0;
    if (seq) { rc = lines_of(seq, read_len + (s->P.colour_space ? 1 : 0), sptr, "read %d: %d characters, expected %d"); if (rc) return rc; }   // letters, or primer + colours
    if (quals_) { rc = lines_of(quals_, read_len, qptr, "read %d: QUAL string of %d characters for %d bases"); if (rc) return rc; }
    if (names) split_lines(names, n_reads, nptr, &nlen);
    nthreads = gm_host_threads(32);                            // a multi-rank job divides the cores itself: GM_HOST_THREADS (bench.py: cores / ranks of this node)
    ops_stride = s->set[0].ops_stride; guard_tol = gm_tune("GM_POST_GUARD_TOL");
    // Two buffer sets: the front of sub-batch i + 1 (stream A) is queued before the host turns to the back of sub-batch i (stream B),
    // so K1 of the next sub-batch and pass 1 / pass 2 of this one share the CUs (see pipeline_front).  GM_OVERLAP=0: one set, in order.
    overlap = n_reads > s->set[0].eff_batch;
    if (const char* e = getenv("GM_OVERLAP")) overlap = overlap && atoi(e) != 0;
    if (overlap) { rc = match_sets(0); if (rc) return rc; if (s->set[1].eff_batch != s->set[0].eff_batch) overlap = false; }
    if (const char* e = gm_tune("GM_RAMP_MIN")) ramp_min = std::max(64, atoi(e));
    timeline = getenv("GM_TIMELINE") != nullptr;               // GM_TIMELINE=1: where the calling thread's time goes, per sub-batch (stderr)
    return GM_OK;
  }
  // Sub-batch sizes: while the two halves overlap, the first sub-batch's front and the last one's back (and its host work) have nothing to
  // run beside, so the sizes ramp up from 8 192 at the start and halve towards the end (results do not depend on the split).
  int size_at(int base, int eff) const {
    const int R = n_reads - base;
    int n = std::min(eff, R);
    if (!overlap || ramp_min >= eff) return n;
    n = std::min(n, std::max(ramp_min, base + ramp_min));
    n = std::min(n, std::max(ramp_min, R / 2));
    return R - n < ramp_min / 2 ? std::min(eff, R) : n;
  }
};
// The host work of one sub-batch (pass-2 selection, MAPQ, SAM text) on a thread of its own, while the GPU works on the next sub-batch
struct ReadJob {
  int idx = 0, base = 0, n = 0; HostSlot* hs = nullptr; const uint32_t* hreads = nullptr;
  std::vector<std::string> outs; std::vector<uint64_t> cm, cr; double ms = 0; bool failed = false; std::thread th;
  ~ReadJob() { if (th.joinable()) th.join(); }
};
// The call's state that changes from sub-batch to sub-batch, and the stages in the order map_impl calls them.
// Sub-batch i lives in set i & 1.  Its front is queued as early as the set allows: the first two at once, the front of i + 2 from the back of i -- behind pass 2
// and the copy of the counters, in front of the wait for the result copies (the device orders it behind event pev[.][9]).  Short fronts
// (the bucket kernel on a small genome: 6 ms a sub-batch) then follow each other without the gap of a host round trip.
struct ReadRun : ReadCall {
  int q_base = 0, q_idx = 0;                                  // next sub-batch whose front is not queued yet: its first read, its number
  int fr_n[2] = {0, 0};                                       // reads of the sub-batch whose front is queued on set k
  std::vector<int8_t> xbuf; std::vector<uint8_t> qvbuf;       // colour space with QVs: a sub-batch's crossover scores and quality values on their way up
  std::atomic<uint64_t> post_redo{0};
  size_t joined = 0; double tl_join = 0, tl_spawn = 0;        // jobs joined so far; GM_TIMELINE: the last start_job's wait for a job, and its spawn
  // The SAM text is assembled as the jobs finish, in input order (each job appends after its predecessor)
  GmTextOut out;
  std::vector<std::unique_ptr<ReadJob>> jobs;                 // (last: their threads read the ReadCall part, post_redo and out, and are joined before anything here goes away)
  explicit ReadRun(size_t n_reads_) : out(g_outcache, n_reads_) {}
  // copies of one sub-batch into set k; host memory goes through stream C so that the call never waits behind queued kernels
  int queue_inputs(int k, int base, int n) {
    DevSet& S = s->set[k];
    S.xover_on = false;
    if (!reads_host) { GM_HIP(hipMemcpyAsync(S.d_reads, (const uint32_t*)reads_dev + (size_t)base * read_words, (size_t)n * read_words * 4, hipMemcpyDeviceToDevice, s->stream)); return GM_OK; }
    hipStream_t c = s->stream_c;
    GM_HIP(hipMemcpyAsync(S.d_reads, reads_host + (size_t)base * read_words, (size_t)n * read_words * 4, hipMemcpyHostToDevice, c));
    if (initbp) GM_HIP(hipMemcpyAsync(S.d_initbp, initbp + base, (size_t)n, hipMemcpyHostToDevice, c));
    if (initbp && quals) {                                   // per-position crossover scores from the QVs, ref: gmapper.c:532-544
      xbuf.resize((size_t)n * read_len); qvbuf.resize((size_t)n * read_len);
      xover_from_quals(s, qptr.data() + base, n, read_len, qual_delta, xbuf.data(), qvbuf.data());
      GM_HIP(hipMemcpyAsync(S.d_xover, xbuf.data(), xbuf.size(), hipMemcpyHostToDevice, c));
      GM_HIP(hipMemcpyAsync(S.d_qv, qvbuf.data(), qvbuf.size(), hipMemcpyHostToDevice, c));
      GM_HIP(hipStreamSynchronize(c));                      // xbuf is reused by the next sub-batch
      S.xover_on = true;
    }
    GM_HIP(hipEventRecord(s->pev[k][8], c));
    GM_HIP(hipStreamWaitEvent(s->stream, s->pev[k][8], 0));
    return GM_OK;
  }
  int queue_front(bool behind_back) {                         // queues the front of sub-batch q_idx, if there is one
    if (q_base >= n_reads) return GM_OK;
    const int k = overlap ? (q_idx & 1) : 0;
    const int n = size_at(q_base, s->set[k].eff_batch);
    if (behind_back) { GM_HIP(hipStreamWaitEvent(s->stream, s->pev[k][9], 0)); GM_HIP(hipStreamWaitEvent(s->stream_c, s->pev[k][9], 0)); }
    int rc = queue_inputs(k, q_base, n); if (!rc) rc = pipeline_front(s, k, n, read_len); if (rc) return rc;
    fr_n[k] = n; q_base += n; q_idx++;
    return GM_OK;
  }
  // The back of the sub-batch on set k.  go_ahead: the front of the sub-batch after next is queued onto this set in front of the wait for the result copies -- only when
  // the capacities are settled (a re-allocation frees the set's buffers), i.e. not for the first sub-batches
  int back(int k, HostSlot& H, int n, bool have_next, bool go_ahead, float* lookup_ms) {
    BackStages B{s, k, H, n, read_len, stats};
    int rc = B.through_copy_out(have_next); if (!rc && go_ahead) rc = queue_front(true);
    return rc ? rc : B.finish_back(lookup_ms);
  }
  // capacities of set `cur` grew: same for the other set, then again from the front of sub-batch idx (its first read: base)
  int redo(int cur, int base, int idx) {
    GM_HIP(hipStreamSynchronize(s->stream));
    if (overlap) { const int rc = match_sets(cur); if (rc) return rc; }
    q_base = base; q_idx = idx;
    return GM_OK;
  }
  void finalize(ReadJob* J) {
    auto t0 = std::chrono::steady_clock::now();
    const int n = J->n; const int chunk = std::max(256, std::min(4096, n / (2 * nthreads)));   // small sub-batches (the ramp) still use every thread
    const int nchunks = (n + chunk - 1) / chunk;
    J->outs.assign(nchunks, std::string()); J->cm.assign(nchunks, 0); J->cr.assign(nchunks, 0);
    std::atomic<int> next(0);
    HitScorer F; F.s = s; F.read_len = read_len; F.read_words = read_words;
    if (s->P.colour_space) { F.reads = J->hreads; F.initbp = initbp + J->base; F.ops_half = ops_stride / 2; F.csk = cs_post_consts(s); if (J->hs->post_on) { F.res_base = J->hs->res; F.post_base = J->hs->post; if (J->hs->post_bq_on) F.bq_base = J->hs->post_bq; } }
    F.redo_ctr = &post_redo; if (guard_tol) F.guard_tol = atof(guard_tol);
    if (quals) { F.qual_ptr = qptr.data() + J->base; F.qual_delta = qual_delta; }
    const RecCtx C{s->P, s->ix->names, s->ix->contig_off, s->h_genome.data()};
    auto worker = [&]() {
      std::vector<FHit> fh; std::vector<FHit*> p2;
      for (;;) {
        int c = next.fetch_add(1); if (c >= nchunks) break;
        std::string& o = J->outs[c]; o = gm_text_pool().take(); if (emit_sam) o.reserve((size_t)chunk * (read_len + 120));
        for (int rd = c * chunk; rd < std::min(n, (c + 1) * chunk); rd++) {
          const uint32_t cnt = J->hs->sel_cnt[rd], off = J->hs->sel_off[rd];
          const size_t before = o.size();
          const int g = J->base + rd;                           // the read's place in the call: its name ("r<g>" when the call gave none) and lines
          char nbuf[32]; nbuf[0] = 'r';
          const RecRead R{named ? nptr[g] : nbuf, named ? (size_t)nlen[g] : (size_t)(put_int(nbuf + 1, g) - nbuf), J->hreads + (size_t)rd * read_words, read_len,
                          initbp ? (int)initbp[g] : -1, quals ? qptr[g] : nullptr, qual_delta, seq_text ? sptr[g] : nullptr, ops_stride};
          int k = F.finalize_read(C, R, cnt ? &J->hs->res[off] : nullptr, J->hs->ops, (int)cnt, o, fh, p2);
          if (per_read_bytes) per_read_bytes[J->base + rd] = (uint32_t)(o.size() - before);
          if (!p2.empty()) J->cm[c]++;  J->cr[c] += k;
          if (!emit_sam) o.clear();
        }
      }
    };
    gm_run_on_threads(nthreads, worker);
    J->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (emit_sam) out.append(J->idx, J->outs, (size_t)n, std::min(nthreads, 4), gm_run_on_threads, [J](size_t c) { gm_text_pool().give(std::move(J->outs[c])); J->outs[c] = std::string(); });
  }
  // a job thread's body: no exception leaves it, and on every path the output turn passes to the next job
  void run_job(ReadJob* J) {
    try { finalize(J); } catch (...) { J->failed = true; if (emit_sam) out.fail(J->idx); }
    for (auto& o : J->outs) gm_text_pool().give(std::move(o));          // (what the copy did not hand back already)
  }
  // the host job of the sub-batch in slot H: at most two outstanding
  void start_job(HostSlot& H, int base, int n) {
    std::unique_ptr<ReadJob> J(new ReadJob());
    J->base = base; J->n = n; J->idx = (int)jobs.size(); J->hs = &H; J->hreads = reads_host ? reads_host + (size_t)base * read_words : H.reads;
    const double t0 = gm_now_ms();
    while (jobs.size() - joined >= 2) { jobs[joined]->th.join(); joined++; }
    const double t1 = gm_now_ms();
    jobs.reserve(jobs.size() + 1);                             // (nothing throws between the thread's start and its owner's place in jobs)
    J->th = std::thread([this, jp = J.get()]() { run_job(jp); });
    jobs.push_back(std::move(J));
    tl_join = t1 - t0; tl_spawn = gm_now_ms() - t1;
  }
  // join, totals, statistics, the text to the caller
  int finish(double tl0, char** sam, size_t* sam_len) {
    const double tl_f = gm_now_ms();
    bool job_failed = false; uint64_t matched = 0, records = 0;
    for (auto& j : jobs) if (j->th.joinable()) j->th.join();
    if (timeline) { fprintf(stderr, "[timeline] t %8.2f  final join %6.2f; host jobs:", tl_f - tl0, gm_now_ms() - tl_f); for (auto& j : jobs) fprintf(stderr, " %.1f", j->ms); fprintf(stderr, "\n"); }
    for (auto& j : jobs) {
      for (size_t c = 0; c < j->cm.size(); c++) { matched += j->cm[c]; records += j->cr[c]; }
      if (stats) stats->ms_host += j->ms;
      job_failed = job_failed || j->failed;
    }
    if (job_failed) { gm_set_error("gm_map_reads: out of memory in the output stage"); return GM_E_NOMEM; }
    if (stats) { stats->reads = n_reads; stats->reads_matched = matched; stats->sam_records = records; stats->post_sw_host_redo = post_redo.load(); }
    size_t len = 0;
    if (sam) { *sam = emit_sam ? out.hand_over(&len) : nullptr; if (emit_sam && !*sam) return GM_E_NOMEM; }
    if (sam_len) *sam_len = len;
    return GM_OK;
  }
};
}  // namespace

// Sub-batches are pipelined: while the GPU works on sub-batch i+1, host threads finish sub-batch i (pass-2 selection, MAPQ, SAM text).  Output stays in input order.
static int map_impl(gm_session* s, int n_reads, int read_len, const uint32_t* reads_host, const void* reads_dev, const char* names, int emit_sam, char** sam, size_t* sam_len,
                    gm_map_stats_t* stats, const uint8_t* initbp_host = nullptr, const char* quals = nullptr, int qual_delta = 33, const char* seq_text = nullptr, uint32_t* per_read_bytes = nullptr) {
  if (int rc = ReadCall::check_args(s, n_reads, read_len, initbp_host)) return rc;
  const double tl_in = gm_now_ms();
  GmDevTurn dev_turn(s);
  const double tl_turn = gm_now_ms();
  try {
    ReadRun R((size_t)n_reads);                                // (inside the try block: its job threads are joined before an exception is answered)
    int rc = R.init(s, n_reads, read_len, reads_host, reads_dev, names, emit_sam, stats, initbp_host, quals, qual_delta, seq_text, per_read_bytes); if (rc) return rc;
    const double tl0 = gm_now_ms();
    if (R.timeline) fprintf(stderr, "[timeline] before the first sub-batch: %.2f ms waiting for the device's turn, %.2f ms set-up\n", tl_turn - tl_in, tl0 - tl_turn);
    int base = 0, idx = 0;
    while (base < n_reads) {
      const int cur = R.overlap ? (idx & 1) : 0; float lk = 0;
      const double tl_a = gm_now_ms();
      while (!rc && R.q_idx <= idx + (R.overlap ? 1 : 0) && R.q_base < n_reads) rc = R.queue_front(false);      // (the start of the call, and after a re-allocation)
      const int n = R.fr_n[cur];
      const bool have_next = R.q_idx > idx + 1;
      HostSlot& HS = s->slot[R.jobs.size() % 3];
      HS.want_reads = reads_host == nullptr;
      const double tl_b = gm_now_ms();
      if (!rc) rc = R.back(cur, HS, n, have_next, R.overlap && idx >= 2, &lk);
      const double tl_c = gm_now_ms();
      if (rc == GM_REDO) { rc = R.redo(cur, base, idx); if (rc) return rc; continue; }
      if (rc) { (void)hipStreamSynchronize(s->stream); (void)hipStreamSynchronize(s->stream_b); return rc; }
      s->last_lookup_ms += lk; s->last_lookup_launches++;
      R.start_job(HS, base, n);
      if (R.timeline) fprintf(stderr, "[timeline] t %8.2f  n %7d  fronts %6.2f  back %6.2f  join-wait %6.2f  spawn %5.2f  (K1 %.2f ms, %u read-strands through the heavy tier)\n",
                              tl_a - tl0, n, tl_b - tl_a, tl_c - tl_b, R.tl_join, R.tl_spawn, lk, s->h_pin[cur]);
      base += n; idx++;
    }
    return R.finish(tl0, sam, sam_len);
  } catch (const std::exception& e) { gm_set_error("gm_map_reads: %s", e.what()); return GM_E_NOMEM; }
}

extern "C" int gm_map_reads(gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const char* names,
                            char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  return map_impl(s, n_reads, read_len, reads_packed, nullptr, names, 1, sam, sam_len, stats);
}
extern "C" int gm_map_reads_fastq(gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const char* names, const char* quals, int qual_delta,
                                  char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (!quals) { gm_set_error("gm_map_reads_fastq: no QUAL strings"); return GM_E_ARG; }
  if (s && s->P.colour_space) { gm_set_error("gm_map_reads_fastq: letter space only"); return GM_E_ARG; }
  return map_impl(s, n_reads, read_len, reads_packed, nullptr, names, 1, sam, sam_len, stats, nullptr, quals, qual_delta);
}
extern "C" int gm_map_reads_cs_fastq(gm_session_t* s, int n_reads, int n_colours, const uint32_t* colours_packed, const uint8_t* initbp, const char* names,
                                     const char* quals, int qual_delta, char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (!colours_packed || !initbp || !quals) { gm_set_error("gm_map_reads_cs_fastq: bad arguments"); return GM_E_ARG; }
  if (s && 2 * s->P.crossover_score < -128) { gm_set_error("crossover score %d: per-position scores are kept in 8 bits", s->P.crossover_score); return GM_E_RANGE; }
  for (int i = 0; i < n_reads; i++) if (initbp[i] > 3) { gm_set_error("read %d: primer letter code %d", i, (int)initbp[i]); return GM_E_ARG; }
  return map_impl(s, n_reads, n_colours, colours_packed, nullptr, names, 1, sam, sam_len, stats, initbp, quals, qual_delta);
}
extern "C" int gm_map_reads_cs(gm_session_t* s, int n_reads, int n_colours, const uint32_t* colours_packed, const uint8_t* initbp, const char* names,
                               char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (!colours_packed || !initbp) { gm_set_error("gm_map_reads_cs: bad arguments"); return GM_E_ARG; }
  for (int i = 0; i < n_reads; i++) if (initbp[i] > 3) { gm_set_error("read %d: primer letter code %d (the reference rejects such reads, fasta.c:636-645)", i, (int)initbp[i]); return GM_E_ARG; }
  return map_impl(s, n_reads, n_colours, colours_packed, nullptr, names, 1, sam, sam_len, stats, initbp);
}
extern "C" int gm_map_reads_device(gm_session_t* s, int n_reads, int read_len, const void* reads_dev, int emit_sam, char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  return map_impl(s, n_reads, read_len, nullptr, reads_dev, nullptr, emit_sam, sam, sam_len, stats);
}
// ---- A22: text -> 4-bit codes (ref: common/fasta.c:609-673; tables :151-200, fasta.h:26-42) --------------------------------------------------
// Host code (no device needed).  Letter space: A C G T U M R W S Y K V H D B N = 0..15, X and '.' = 15, either case.  Colour space: the first
// character is the primer letter (A/C/G/T, either case; anything else: the reference drops the read), then colours 0-3, and 4 / N / n / . / X / x = 15.
extern "C" int gm_sequence_to_bitfield(int colour_space, const char* seq, int seq_len, uint32_t* words, int* initbp) {
  if (!seq || seq_len < 1 || !words) { gm_set_error("gm_sequence_to_bitfield: bad arguments"); return GM_E_ARG; }
  static const signed char LS[128] = {
    -1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1, -1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,15,-1, -1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,-1,
    -1, 0,14, 1,13,-1,-1, 2,12,-1,-1,10,-1, 5,15,-1, -1,-1, 6, 8, 3, 4,11, 7,15, 9,-1,-1,-1,-1,-1,-1,  -1, 0,14, 1,13,-1,-1, 2,12,-1,-1,10,-1, 5,15,-1, -1,-1, 6, 8, 3, 4,11, 7,15, 9,-1,-1,-1,-1,-1,-1};
  int i = 0, idx = 0;
  if (colour_space) {
    int b;
    switch (seq[0]) { case 'A': case 'a': b = 0; break; case 'C': case 'c': b = 1; break; case 'G': case 'g': b = 2; break; case 'T': case 't': b = 3; break;
                      default: gm_set_error("colour-space read does not start with a primer letter (ref: fasta.c:626-634)"); return GM_E_ARG; }
    if (initbp) *initbp = b;
    i = 1;
  }
  const int n = seq_len - i;
  memset(words, 0, (size_t)((n + 7) / 8) * 4);
  for (; i < seq_len; i++, idx++) {
    const unsigned char ch = (unsigned char)seq[i]; int a = -1;
    if (colour_space) { if (ch >= '0' && ch <= '3') a = ch - '0'; else if (ch == '4' || ch == 'N' || ch == 'n' || ch == '.' || ch == 'X' || ch == 'x') a = 15; }
    else if (ch < 128) a = LS[ch];
    if (a < 0) { gm_set_error("invalid character 0x%x in a read (did you mix up letter space and colour space? ref: fasta.c:639-650)", ch); return GM_E_ARG; }
    words[idx >> 3] |= (uint32_t)a << ((idx & 7) * 4);
  }
  return GM_OK;
}

// Text entry point: n reads of one length as lines ('\n' separated): letters, or in a colour-space session primer + colours.  The library packs them
// (gm_sequence_to_bitfield) and keeps the characters for what the reference prints from the file's text: SEQ of unaligned reads and of clipped ends,
// the CS:Z tag.  quals (optional): FASTQ QUAL lines and their offset.
extern "C" int gm_map_reads_text(gm_session_t* s, int n_reads, int read_len, const char* seqs, const char* names, const char* quals, int qual_delta,
                                 char** sam, size_t* sam_len, gm_map_stats_t* stats) {
  if (!s || !seqs || n_reads < 0 || read_len < 1) { gm_set_error("gm_map_reads_text: bad arguments"); return GM_E_ARG; }
  const int cs = s->P.colour_space ? 1 : 0, line = read_len + cs, rwords = (read_len + 7) / 8;
  std::vector<uint32_t> packed((size_t)n_reads * rwords); std::vector<uint8_t> ibp(cs ? n_reads : 0);
  if (gm_fixed_lines(seqs, (size_t)n_reads, (size_t)line)) {      // packing on the host threads (one thread took 90 ms per million 100-base reads)
    std::atomic<int> bad_rc(GM_OK); std::mutex em; std::string emsg;
    gm_parallel_for((size_t)n_reads, 8192, [&](size_t b0, size_t e0) {
      for (size_t i = b0; i < e0 && bad_rc.load(std::memory_order_relaxed) == GM_OK; i++) {
        int b = 0; int rc = gm_sequence_to_bitfield(cs, seqs + i * ((size_t)line + 1), line, packed.data() + i * rwords, &b);
        if (rc) { std::lock_guard<std::mutex> lk(em); if (bad_rc == GM_OK) { bad_rc = rc; emsg = gm_last_error(); } return; }
        if (cs) ibp[i] = (uint8_t)b;
      }
    });
    if (bad_rc != GM_OK) { gm_set_error("%s", emsg.c_str()); return bad_rc; }
  } else {
  const char* p = seqs;
  for (int i = 0; i < n_reads; i++) {
    const char* e = line_end(p);
    if ((int)(e - p) != line) { gm_set_error("read %d: %d characters, expected %d", i, (int)(e - p), line); return GM_E_ARG; }
    int b = 0; const int rc = gm_sequence_to_bitfield(cs, p, line, packed.data() + (size_t)i * rwords, &b); if (rc) return rc;
    if (cs) ibp[i] = (uint8_t)b;
    p = *e ? e + 1 : e;
  }
  }
  return map_impl(s, n_reads, read_len, packed.data(), nullptr, names, 1, sam, sam_len, stats, cs ? ibp.data() : nullptr, quals, qual_delta, seqs);
}

// (the file entry points -- the reads reader, the per-read preprocessing, chunked streaming -- live in gm_host_files.inc, included below)

extern "C" int gm_last_lookup_timing(gm_session_t* s, double* ms, uint64_t* alg_bytes, int* launches) {
  if (!s) return GM_E_ARG;
  if (ms) *ms = s->last_lookup_ms; if (alg_bytes) *alg_bytes = s->last_lookup_bytes; if (launches) *launches = s->last_lookup_launches;
  return GM_OK;
}

#include "gm_host_pairs.inc"
#include "gm_host_files.inc"
#include "gm_index_io.inc"

// stage dump for parity tests: hits selected by pass 1, in ext-heap array order (before pass 2 / reverse_hit)
static int debug_tophits_impl(gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, const uint8_t* initbp, long long* rows, long cap, long* n_rows) {
  if (!s) return GM_E_ARG;
  if (initbp && !s->P.colour_space) { gm_set_error("gm_debug_tophits_cs: the session is not a colour-space one"); return GM_E_ARG; }
  GmDevTurn dev_turn(s);     // (admitted like the mapping entries)
  GM_HIP(hipSetDevice(s->ix->device));
  DevSet& D = s->set[0];
  if (int rc = prepare_unpaired_set(s, read_len)) return rc;
  const int read_words = (read_len + 7) / 8;
  float lk; int rc;
  do {
    if (n_reads > D.eff_batch) { gm_set_error("gm_debug_tophits: at most %d reads per call", D.eff_batch); return GM_E_ARG; }
    GM_HIP(hipMemcpyAsync(D.d_reads, reads_packed, (size_t)n_reads * read_words * 4, hipMemcpyHostToDevice, s->stream));
    if (initbp) GM_HIP(hipMemcpyAsync(D.d_initbp, initbp, (size_t)n_reads, hipMemcpyHostToDevice, s->stream));
    rc = run_device_pipeline(s, s->slot[0], n_reads, read_len, &lk);
  } while (rc == GM_REDO);
  if (rc) return rc;
  std::vector<int32_t> sel((size_t)n_reads * GM_SEL_MAX); std::vector<GmHit> hits((size_t)n_reads * 2 * D.hcap);
  GM_HIP(hipMemcpy(sel.data(), D.d_sel, sel.size() * 4, hipMemcpyDeviceToHost));
  GM_HIP(hipMemcpy(hits.data(), D.d_hits, hits.size() * sizeof(GmHit), hipMemcpyDeviceToHost));
  long w = 0;
  for (int rd = 0; rd < n_reads; rd++)
    for (uint32_t k = 0; k < s->slot[0].sel_cnt[rd]; k++) {
      if (w >= cap) { *n_rows = w; return GM_OK; }
      const int id = sel[(size_t)rd * GM_SEL_MAX + k]; const int st = id >> 16, hi = id & 0xFFFF;
      const GmHit& h = hits[((size_t)rd * 2 + st) * D.hcap + hi];
      long long r[12] = {rd, st, h.cn, h.g_off, h.w_len, h.score_vector, h.pct_score_vector, h.matches, h.ax, h.ay, h.alen, h.awidth};
      memcpy(rows + w * 12, r, sizeof r); w++;
    }
  *n_rows = w;
  return GM_OK;
}
extern "C" int gm_debug_tophits(gm_session_t* s, int n_reads, int read_len, const uint32_t* reads_packed, long long* rows, long cap, long* n_rows) {
  return debug_tophits_impl(s, n_reads, read_len, reads_packed, nullptr, rows, cap, n_rows);
}
// colour space: the reads' primer letters go up with their colours (gm_debug_tophits leaves the session's primer buffer as it is)
extern "C" int gm_debug_tophits_cs(gm_session_t* s, int n_reads, int n_colours, const uint32_t* colours_packed, const uint8_t* initbp, long long* rows, long cap, long* n_rows) {
  if (!initbp) { gm_set_error("gm_debug_tophits_cs: initbp is NULL"); return GM_E_ARG; }
  return debug_tophits_impl(s, n_reads, n_colours, colours_packed, initbp, rows, cap, n_rows);
}

#include "gm_host_windows.inc"
#include "gm_host_select.inc"
#include "gm_host_pass1.inc"
#include "gm_host_sam.inc"
#include "gm_host_seams.inc"
#include "gm_host_seams_ix.inc"
#include "gm_host_text.inc"
#include "gm_host_pass2.inc"
#include "gm_host_pass2_cs.inc"
#include "gm_host_pair_mappings.inc"
