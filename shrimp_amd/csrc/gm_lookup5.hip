// gm_lookup5.hip -- K1 v5: spaced-seed lookup + exact region filter + exact prune in ONE kernel (gfx950 only).
//
// Same contract as gm_lookup.hip (which keeps the bucket / slab-sweep / lane-per-list kernels and documents the
// reference lines replaced: read_get_mapidxs, read_get_region_counts, advance_index_in_genomemap,
// ref: gmapper/mapping.c:37-70,459-542,646-805) plus the exact prune of gm_prune.hip, for read-strands with many
// list entries (100 bp reads on a 3 Gbp genome: 251 lists of ~179 entries).  What is different from k_lookup_v4:
//
//  * One WAVE streams one list at a time: the list descriptor (pointer, length, y/seed) is wave-uniform (SGPRs),
//    lane l takes W = ceil(n / 64) consecutive entries of a chunk of n <= 256, read with one dwordx4.  No window
//    map, no prefix over the lists, no per-lane descriptor look-up.
//  * Pre-count in two 1-bit tables: seen[2^(lsw+5)] (region folded onto its low bits) and, an eighth of its size,
//    twice[]: the first mark of a counter sets its seen bit, every later one sets the twice bit.  Pass A marks,
//    pass B streams the lists again and keeps the entries whose twice bit is set -- a superset of the entries
//    whose region reaches the reference's count of 2 (a region's second mark always finds the seen bit set).
//  * The overlap strip (an entry in the first region_overlap bases of a region also counts for the region before,
//    ref: mapping.c:521-533,733-742) is not tested per entry: the index carries, per list, the few strip entries
//    again as a second short list (sdir / spos, derived on the device from dir / pos, 2.4 % of the entries), and
//    two small dense loops mark / test region - 1 for exactly those.
//  * The candidates (~13 % of the entries) stay in LDS -- pass B needs only twice[], so they are written over the
//    dead seen[] table -- and are resolved there: an open-addressing table keyed by region holds the exact mark
//    count (the reference's rule; exact because every entry of a region with count >= 2 is a candidate) and, per
//    region, the number and the min / max offset of the candidates inside it, from which the prune rules of
//    gm_prune.hip are evaluated with region-sized bins.  Judging the prune on candidates instead of survivors
//    only keeps more (both rules are monotone: more neighbours => keep), which is still exact.
//  * 6 workgroup barriers per read-strand (v4: ~25), no candidate scratch in global memory.
//
// Read-strands whose candidates do not fit (repeats) are redone by k_lookup<0> in list mode + k_prune in
// list mode (gm_lookup.hip / gm_prune.hip).
#include <algorithm>
#include <mutex>
#include "gm_common.h"
#include "gm_internal.h"
#include <rocprim/device/device_scan.hpp>

typedef uint32_t k5_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(3))) uint32_t k5_lds_u32;
// LDS word at an absolute LDS byte address (the tables of k_lookup_v5 start at the workgroup's LDS base, which the kernel checks to be 0:
// table offsets are then OR-ed, not added, into the address)
#define K5_LDS(off) ((k5_lds_u32*)(uintptr_t)(uint32_t)(off))
typedef __attribute__((address_space(3))) uint16_t k5_lds_u16;
#define K5_LDS16(off) ((k5_lds_u16*)(uintptr_t)(uint32_t)(off))
#define K5_LDS_OR(off, m) __hip_atomic_fetch_or(K5_LDS(off), (m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

#ifndef K5_Q
#define K5_Q 4            // list chunks in flight per wave (r03 sweep, ms per 262 144 reads: 1: 87.3, 2: 71.0, 3: 68.6, 4: 65.2, 5: see DESIGN, 6: 69.9, 10: 74.3)
#endif
enum { C_NCAND = 0, C_OVERFLOW, C_NMEMB, C_NKEEP, C_WLISTED /* tuning builds: items of the waves' lists */, C_NEDGE, C_NLISTS /* two words: read-strands alternate */, C_SINK = 8, C_NRAW = 9, C_WSPOT = 10 /* tuning builds: items taken on the spot */, C_NCAND0 = 11 /* rounds: the candidates of part 0 */, C_SPILL = 12 /* K5_MAX_ROUNDS - 1 words */, C_WORDS = 16 };

// Diagnostic build (-DK5_STAMPS): thread 0 of every workgroup adds the cycles between the phase boundaries of each read-strand to k5_stamps[]
// (0-5: setup, pass A, pass B, region table, rules + output, clears; 6, 7: candidates, fallbacks; 8-11: parts of set-up / the exact stages, taken out of
// the phase they sit in -- 10, a wave's own step (a) of stage 1, is the view of thread 0's wave: no barrier stands behind it); gm_debug_k5_stamps() reads and resets all 16.  No stamp executes in the normal build.
#ifdef K5_STAMPS
__device__ unsigned long long k5_stamps[16];
#define K5_STAMP(i) do { if (tid == 0) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); atomicAdd(&k5_stamps[i], t_ - t_prev); t_prev = t_; } } while (0)
extern "C" int gm_debug_k5_stamps(unsigned long long* out) {
  unsigned long long z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(k5_stamps), sizeof z) != hipSuccess) return GM_E_NODEVICE;
  if (hipMemcpyToSymbol(HIP_SYMBOL(k5_stamps), z, sizeof z) != hipSuccess) return GM_E_NODEVICE;
  return GM_OK;
}
#else
#define K5_STAMP(i) do { } while (0)
#endif

// Tuning builds: how many read-strands k_lookup_v5 took, and how many of them it handed on -- [1] to the fall-back kernels, [2] to k_prune alone (the prune_only tail) -- so that a
// test with small tables can tell whether its read-strands went through the exact stages at all.  gm_debug_k5_paths() reads and resets the three counts.
#ifdef GM_TUNING
__device__ unsigned long long k5_paths[3];
extern "C" int gm_debug_k5_paths(unsigned long long* out) {
  unsigned long long z[3] = {0, 0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(k5_paths), sizeof z) != hipSuccess) return GM_E_NODEVICE;
  if (hipMemcpyToSymbol(HIP_SYMBOL(k5_paths), z, sizeof z) != hipSuccess) return GM_E_NODEVICE;
  return GM_OK;
}
// The per-wave lists of exact stage 1: [0] items that went through a wave's list, [1] items taken on the spot because the list was full (GM_K5_WLIST caps a wave's list
// below what fits, 0: no list at all), added by thread 0 once per read-strand.  gm_debug_k5_wave_lists() reads and resets the two.
__device__ unsigned long long k5_wave_lists[2];
extern "C" int gm_debug_k5_wave_lists(unsigned long long* out) {
  unsigned long long z[2] = {0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(k5_wave_lists), sizeof z) != hipSuccess) return GM_E_NODEVICE;
  if (hipMemcpyToSymbol(HIP_SYMBOL(k5_wave_lists), z, sizeof z) != hipSuccess) return GM_E_NODEVICE;
  return GM_OK;
}
#endif

struct K5Args {
  const uint32_t* reads; int n_reads, read_len, read_words, max_n_kmers, NL;
  int lsw, ltw;             // log2(words) of seen[] and twice[]
  int cand_cap, hbits;      // candidate records and log2(slots of the region table), both inside the seen[] area
  int cand_limit;
  int xrec;                 // chunk records beyond one per list
  int wlist;                // tuning builds: the most words a wave's list of exact stage 1 may take (GM_K5_WLIST; the release build takes what fits)
  int rounds; uint32_t round_regs;      // the exact stages run `rounds` times, each over `round_regs` regions of the genome (+ one region either side)
  uint2* spill; int spill_cap;          // rounds > 1: (rounds - 1) rows of spill_cap candidates (position, y / seed) per workgroup
  uint64_t* out; uint32_t* out_cnt; int out_cap; uint32_t* surv_cnt;
  int prune; uint32_t D; int e_max;
  uint32_t* heavy_list; uint32_t* heavy_cnt; int heavy_cap;
  unsigned long long* stats;
  uint32_t* fb_list; uint32_t* fb_cnt; int fb_cap;
  uint32_t* start_flags; uint32_t start_epoch;
  // fused prune only: a read-strand that keeps more than out_cap survivors under the region-sized bins writes ALL its members to its raw row and goes to pl_list --
  // k_prune (256-base bins) prunes it from there; without this the lane-per-list kernel had to produce the members again
  uint64_t* raw_out; int raw_cap; uint32_t* surv_seg; int n_slabs; uint32_t* pl_list; uint32_t* pl_cnt; int pl_cap;
};

// lane * W for a wave-uniform W in 1..4 (the 24-bit multiply is a full-rate instruction)
__device__ __forceinline__ uint32_t k5_lane_times(int lane, uint32_t W) {
  uint32_t r; asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(lane), "s"(W)); return r;     // (the compiler turns __umul24 by a uniform factor into the quarter-rate v_mul_lo_u32)
}

#include "gm_region_table.h"

// LSWC: log2(words) of seen[] as a compile-time constant (the production size, 15), or 0 for the size in K5Args (small-table test variants, long reads):
// with constants the table masks are immediates and the base of seen[] folds into the LDS instructions' offset field.
// MULTI: long reads (2 x 150 bp on 3 Gbp: 72 k list entries, ~13 k candidates per read-strand) have more candidates than the LDS holds.  The marks of pass A are complete
// whatever comes next, so pass B and the exact stages run a.rounds times, each time over the candidates of one part of the genome: a.round_regs regions plus ONE region
// either side (a region's count takes the strip marks of the region behind it, its members look at the region before it, the prune rules at both neighbours -- with the
// halo all of that is complete for every region of the part itself), and only candidates of the part itself are emitted.
#define K5_KERNEL_HEAD template <int LSWC> __global__ void __launch_bounds__(1024) k_lookup_v5(GmIndexDev ix, K5Args a)
#define K5_KERNEL_MULTI false
#include "gm_lookup5_kernel.inc"
#undef K5_KERNEL_HEAD
#undef K5_KERNEL_MULTI
// (the variant with rounds carries a few more live values; five waves per SIMD as the allocator's target = 96 registers, so that -- like k_lookup_v5<15> -- its four waves per
// SIMD leave 128 registers to the other stream's kernels; what the allocator then keeps in scratch is stored and re-read per read-strand or per round, outside the streaming loops)
#define K5_KERNEL_HEAD __global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(5, 5))) k_lookup_v5_rounds(GmIndexDev ix, K5Args a)
#define K5_KERNEL_MULTI true
#define K5_KERNEL_LSWC 15
#include "gm_lookup5_kernel.inc"
#undef K5_KERNEL_HEAD
#undef K5_KERNEL_MULTI
#undef K5_KERNEL_LSWC
// The HALF-SIZE shape with rounds (round 4): 512 threads, tables of 2^19 + 2^16 bits -- 80 KB of LDS with the records, so that TWO workgroups share a CU and the phases of two
// read-strands (pass A: memory; pass B: L2 / vector issue; exact stages: LDS round trips) overlap instead of running one after the other.  The smaller seen[] table is a blocked
// Bloom filter (two bits per region, see the kernel body); the candidates (2 720 slots, region table of 4 096) go through the rounds of k_lookup_v5_rounds.
#define K5_KERNEL_HEAD __global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(5, 5))) k_lookup_v5_half(GmIndexDev ix, K5Args a)
#define K5_KERNEL_MULTI true
#define K5_KERNEL_LSWC 14
#define K5_KERNEL_BLOOM true
#include "gm_lookup5_kernel.inc"
#undef K5_KERNEL_HEAD
#undef K5_KERNEL_BLOOM
#ifdef GM_TUNING
// (the same without the Bloom bits: the measurement beside it, tuning builds only)
#define K5_KERNEL_HEAD __global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(5, 5))) k_lookup_v5_half_plain(GmIndexDev ix, K5Args a)
#define K5_KERNEL_BLOOM false
#include "gm_lookup5_kernel.inc"
#undef K5_KERNEL_HEAD
#undef K5_KERNEL_BLOOM
#endif
#undef K5_KERNEL_MULTI
#undef K5_KERNEL_LSWC

// ---------------------------------------------------------------------------------------------
// Strip lists: for every list k of a seed, its entries in the first region_overlap bases of a region > 0, in list
// order: spos[sdir[k] .. sdir[k + 1]).  Derived from dir / pos on the device (one flag pass, a scan over 64-entry
// groups, one scatter pass); not part of the index files.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool k5_strip(uint32_t p, int rb, uint32_t ovl) { return (p & ((1u << rb) - 1u)) < ovl && (p >> rb) > 0u; }

__global__ void __launch_bounds__(256) k_strip_count(const uint32_t* __restrict__ pos, uint32_t n_pos, int rb, uint32_t ovl, uint32_t* __restrict__ grp_cnt, uint32_t n_groups) {
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t g = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (; g < n_groups; g += stride) {
    const uint64_t i = g * 64 + lane;
    const bool f = i < n_pos && k5_strip(pos[i], rb, ovl);
    const unsigned long long b = __ballot(f);
    if (lane == 0) grp_cnt[g] = (uint32_t)__popcll(b);
  }
}
__global__ void __launch_bounds__(256) k_strip_scatter(const uint32_t* __restrict__ pos, uint32_t n_pos, int rb, uint32_t ovl, const uint32_t* __restrict__ grp_rank,
                                                       uint32_t n_groups, uint32_t* __restrict__ spos) {
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t g = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  for (; g < n_groups; g += stride) {
    const uint64_t i = g * 64 + lane;
    const uint32_t p = i < n_pos ? pos[i] : 0u;
    const bool f = i < n_pos && k5_strip(p, rb, ovl);
    const unsigned long long b = __ballot(f);
    if (f) spos[grp_rank[g] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = p;
  }
}
__global__ void __launch_bounds__(256) k_strip_dir(const uint32_t* __restrict__ dir, const uint32_t* __restrict__ pos, uint32_t n_pos, uint64_t K, int S, int rb, uint32_t ovl,
                                                   const uint32_t* __restrict__ grp_rank, uint32_t* __restrict__ sdir) {
  uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (; k <= K; k += stride) {
    const uint32_t i = dir[k * (uint64_t)S];                  // first entry of list k (dir[K * S] = n_pos)
    uint32_t r = grp_rank[i >> 6];
    for (uint32_t q = i & ~63u; q < i; q++) r += k5_strip(pos[q], rb, ovl) ? 1u : 0u;
    sdir[k] = r;
  }
}

static std::mutex g_strip_mutex;
int gm_index_derive_strips(GmIndexHost* ix, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(g_strip_mutex);
  if (ix->strips_ready) return GM_OK;
  const int rb = ix->params.region_bits; const uint32_t ovl = (uint32_t)ix->params.region_overlap;
  for (int sn = 0; sn < ix->n_seeds; sn++) {
    GmSeedHost& sd = ix->seeds[sn];
    const uint64_t K = 1ull << sd.kbits;
    const uint32_t n_groups = (uint32_t)(((uint64_t)sd.n_pos + 63) / 64) + 1u;      // + one empty group: rank of n_pos itself
    uint32_t *d_cnt = nullptr, *d_rank = nullptr; void* tmp = nullptr; size_t tmp_bytes = 0;
    GM_HIP(hipMalloc(&d_cnt, (size_t)n_groups * 4)); GM_HIP(hipMalloc(&d_rank, (size_t)n_groups * 4));
    hipLaunchKernelGGL(k_strip_count, dim3(256 * 16), dim3(256), 0, stream, sd.d_pos, sd.n_pos, rb, ovl, d_cnt, n_groups);
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_bytes, d_cnt, d_rank, 0u, (size_t)n_groups, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) { gm_set_error("exclusive_scan size query: %s", hipGetErrorString(e)); return GM_E_NODEVICE; }
    GM_HIP(hipMalloc(&tmp, tmp_bytes ? tmp_bytes : 16));
    e = rocprim::exclusive_scan(tmp, tmp_bytes, d_cnt, d_rank, 0u, (size_t)n_groups, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) { gm_set_error("exclusive_scan: %s", hipGetErrorString(e)); return GM_E_NODEVICE; }
    uint32_t total = 0;
    GM_HIP(hipMemcpyAsync(&total, d_rank + (n_groups - 1), 4, hipMemcpyDeviceToHost, stream));
    GM_HIP(hipStreamSynchronize(stream));
    sd.n_spos = total;
    GM_HIP(hipMalloc(&sd.d_spos, ((size_t)total + 64) * 4));
    GM_HIP(hipMemsetAsync(sd.d_spos, 0xff, ((size_t)total + 64) * 4, stream));
    GM_HIP(hipMalloc(&sd.d_sdir, (size_t)(K + 1 + 16) * 4));
    hipLaunchKernelGGL(k_strip_scatter, dim3(256 * 16), dim3(256), 0, stream, sd.d_pos, sd.n_pos, rb, ovl, d_rank, n_groups, sd.d_spos);
    hipLaunchKernelGGL(k_strip_dir, dim3(256 * 16), dim3(256), 0, stream, sd.d_dir, sd.d_pos, sd.n_pos, K, ix->n_slabs, rb, ovl, d_rank, sd.d_sdir);
    GM_HIP(hipGetLastError());
    GM_HIP(hipStreamSynchronize(stream));
    (void)hipFree(d_cnt); (void)hipFree(d_rank); (void)hipFree(tmp);
  }
  ix->strips_ready = true;
  return GM_OK;
}

// ---------------------------------------------------------------------------------------------
// launch, in the shape the plan gave (k5_shape, gm_lookup_plan.h): 1 when v5 was launched (0: its scratch could not be allocated, the caller takes the plan's
// next kernel; < 0: error)
// ---------------------------------------------------------------------------------------------
static_assert(K5_CTRL_WORDS == C_WORDS, "gm_lookup_plan.h restates the control words");
int gm_lookup5_launch(const K1Call& c, const K5Shape& sh, int wlist, uint64_t* d_out, uint32_t* d_out_cnt, int out_cap, GmK1Scratch* K) {
  const hipStream_t stream = c.stream;
  const int fb_cap = std::max(4096, 2 * c.n_reads);              // every read-strand may fall back (tiny tables in the tests, repeats)
  if (fb_cap > K->k5_cap) {
    if (K->k5_fb) { (void)hipStreamSynchronize(stream); (void)hipFree(K->k5_fb); (void)hipFree(K->k5_pl); K->k5_fb = nullptr; K->k5_pl = nullptr; K->k5_cap = 0; }
    if (hipMalloc(&K->k5_fb, (size_t)(fb_cap + 4) * 4) != hipSuccess) return 0;
    if (hipMalloc(&K->k5_pl, (size_t)(fb_cap + 4) * 4) != hipSuccess) return 0;
    K->k5_cap = fb_cap;
  }
  uint32_t* const fb_cnt_p = K->k5_fb + K->k5_cap; uint32_t* const pl_cnt_p = K->k5_pl + K->k5_cap;
  if (hipMemsetAsync(fb_cnt_p, 0, 4, stream) != hipSuccess || hipMemsetAsync(pl_cnt_p, 0, 4, stream) != hipSuccess) return GM_E_NODEVICE;
  if (gm_lds_at_least((const void*)k_lookup_v5<15>, sh.lds) != hipSuccess || gm_lds_at_least((const void*)k_lookup_v5<14>, sh.lds) != hipSuccess ||
      gm_lds_at_least((const void*)k_lookup_v5_rounds, sh.lds) != hipSuccess || gm_lds_at_least((const void*)k_lookup_v5_half, sh.lds) != hipSuccess ||
#ifdef GM_TUNING
      gm_lds_at_least((const void*)k_lookup_v5_half_plain, sh.lds) != hipSuccess ||
#endif
      gm_lds_at_least((const void*)k_lookup_v5<0>, sh.lds) != hipSuccess) return 0;
  K5Args a;
  a.reads = c.reads; a.n_reads = c.n_reads; a.read_len = c.read_len; a.read_words = c.read_words; a.max_n_kmers = c.g.max_n_kmers; a.NL = c.g.NL;
  a.lsw = sh.lsw; a.ltw = sh.ltw; a.cand_cap = sh.cand_cap; a.hbits = sh.hbits; a.cand_limit = sh.cand_limit; a.xrec = sh.xrec; a.rounds = sh.rounds; a.round_regs = sh.round_regs;
  a.out = d_out; a.out_cnt = d_out_cnt; a.out_cap = out_cap; a.surv_cnt = c.surv_cnt; a.prune = sh.prune ? 1 : 0; a.D = sh.D; a.e_max = sh.e_max;
  a.heavy_list = c.heavy_list; a.heavy_cnt = c.heavy_cnt; a.heavy_cap = c.heavy_cap; a.stats = c.stats;
  a.fb_list = K->k5_fb; a.fb_cnt = fb_cnt_p; a.fb_cap = fb_cap;
  // (the raw rows, their stride and the survivors-per-slab rows are read only with the prune rules)
  a.raw_out = sh.prune ? c.surv : nullptr; a.raw_cap = c.scap; a.surv_seg = c.surv_seg; a.n_slabs = c.ix.n_slabs; a.pl_list = K->k5_pl; a.pl_cnt = pl_cnt_p; a.pl_cap = fb_cap;
  a.spill = nullptr; a.spill_cap = sh.cand_cap;
  a.wlist = wlist;
  if (sh.rounds > 1) {
    const size_t need = (size_t)sh.grid * (size_t)(sh.rounds - 1) * (size_t)sh.cand_cap;
    if (need > K->k5_spill_n) {
      if (K->k5_spill) { (void)hipStreamSynchronize(stream); (void)hipFree(K->k5_spill); K->k5_spill = nullptr; K->k5_spill_n = 0; }
      if (hipMalloc(&K->k5_spill, need * sizeof(uint2)) != hipSuccess) return 0;
      K->k5_spill_n = need;
    }
    a.spill = K->k5_spill;
  }
  const bool use_flags = K->start_flags && sh.grid <= K->flag_cap;
  K->flag_grid = use_flags ? sh.grid : 0;
  a.start_flags = use_flags ? K->start_flags : nullptr; a.start_epoch = K->epoch;
  const dim3 grid(sh.grid), threads(sh.threads);
  if (sh.half) {
#ifdef GM_TUNING
    if (sh.half == 2) hipLaunchKernelGGL(k_lookup_v5_half_plain, grid, threads, sh.lds, stream, c.ix, a); else
#endif
    hipLaunchKernelGGL(k_lookup_v5_half, grid, threads, sh.lds, stream, c.ix, a);
  } else if (sh.rounds > 1) hipLaunchKernelGGL(k_lookup_v5_rounds, grid, threads, sh.lds, stream, c.ix, a);
  else if (sh.lsw == 15) hipLaunchKernelGGL((k_lookup_v5<15>), grid, threads, sh.lds, stream, c.ix, a);
  else if (sh.lsw == 14) hipLaunchKernelGGL((k_lookup_v5<14>), grid, threads, sh.lds, stream, c.ix, a);
  else hipLaunchKernelGGL((k_lookup_v5<0>), grid, threads, sh.lds, stream, c.ix, a);
  if (hipGetLastError() != hipSuccess) return GM_E_NODEVICE;
  return 1;
}
