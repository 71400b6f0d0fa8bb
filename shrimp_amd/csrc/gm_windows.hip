// gm_windows.hip -- export of K2's candidate windows (gm_read_windows): hcap-strided rows -> one tight array of gm_read_window_t (gfx950 only).
//
// K2 leaves, per read-strand rs, hit_cnt[rs] GmHit records in hits[rs * hcap ..] and their (contig, g_off) order in perm[rs * hcap ..].  Most read-strands hold
// 0-3 windows and hcap is 64 or more, so the rows are nearly empty: the export reads the counts, never the rows' padding.
//   k_win_scan:    exclusive scan of the 2 n counts (each clamped to hcap) into 64-bit offsets, off[2 n] = total.  One workgroup of 1 024 threads walks the
//                  counts in tiles of 16 384 (16 consecutive counts a thread, four uint4 loads in flight) with a running carry -- at most 16 tiles a
//                  sub-batch, one launch, no hand-off between workgroups.  One CU reads 1 MB and writes 2 MB at the most: 92 us per 262 144 counts (105 us at
//                  4 counts a thread), 1.3 % of the call it serves -- the price of having no second launch and no look-back.
//   k_win_scatter: a LANE a window.  Window j belongs to the read-strand rs with off[rs] <= j < off[rs + 1]: the workgroup's first two threads find the
//                  read-strands of its first and last window, every lane then searches between those (about nine steps where half the read-strands are empty).
//                  The lane reads its GmHit (40 bytes, five 8-byte loads) through perm and stores the 48-byte record as three 16-byte stores: a wave writes
//                  3 KB of consecutive bytes.
#include "gm_common.h"
#include <algorithm>
#include "gm_internal.h"

static_assert(sizeof(gm_read_window_t) == 48, "gm_read_window_t: 12 x 32 bits");
static_assert(sizeof(GmHit) == 40, "GmHit: ten 32-bit words");

#define WIN_SCAN_THREADS 1024
#define WIN_SCAN_VALS 16                                  // consecutive counts a thread (a multiple of 4: uint4 loads, 16-byte stores)
#define WIN_SCAN_TILE (WIN_SCAN_VALS * WIN_SCAN_THREADS)

__global__ __launch_bounds__(WIN_SCAN_THREADS) void k_win_scan(const uint32_t* __restrict__ cnt, int m, int hcap, unsigned long long* __restrict__ off) {
  __shared__ unsigned long long wave_sum[WIN_SCAN_THREADS / GM_WAVE];
  __shared__ unsigned long long carry_s;
  const int tid = threadIdx.x, lane = tid & (GM_WAVE - 1), wv = tid / GM_WAVE;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < m; base += WIN_SCAN_TILE) {
    const int i = base + WIN_SCAN_VALS * tid;
    const bool whole = i + WIN_SCAN_VALS <= m;
    uint32_t c[WIN_SCAN_VALS];
    if (whole) {
      uint4 v[WIN_SCAN_VALS / 4];
      for (int k = 0; k < WIN_SCAN_VALS / 4; k++) v[k] = *(const uint4*)(cnt + i + 4 * k);      // (all of the thread's loads in flight at once)
      for (int k = 0; k < WIN_SCAN_VALS / 4; k++) { c[4 * k] = v[k].x; c[4 * k + 1] = v[k].y; c[4 * k + 2] = v[k].z; c[4 * k + 3] = v[k].w; }
    } else for (int k = 0; k < WIN_SCAN_VALS; k++) c[k] = i + k < m ? cnt[i + k] : 0u;
    unsigned long long mine = 0;
    for (int k = 0; k < WIN_SCAN_VALS; k++) { c[k] = min(c[k], (uint32_t)hcap); mine += c[k]; }      // (K2 counts every window it found, also those beyond the row)
    unsigned long long incl = mine;
    for (int d = 1; d < GM_WAVE; d <<= 1) { const unsigned long long o = __shfl_up(incl, d); if (lane >= d) incl += o; }
    if (lane == GM_WAVE - 1) wave_sum[wv] = incl;
    __syncthreads();
    unsigned long long before = carry_s;
    for (int w = 0; w < wv; w++) before += wave_sum[w];
    unsigned long long o = before + incl - mine;
    if (whole) {
      for (int k = 0; k < WIN_SCAN_VALS; k += 2) { ulonglong2 a; a.x = o; a.y = o + c[k]; o = a.y + c[k + 1]; *(ulonglong2*)(off + i + k) = a; }
    } else for (int k = 0; k < WIN_SCAN_VALS; k++) { if (i + k < m) off[i + k] = o; o += c[k]; }
    __syncthreads();
    if (tid == WIN_SCAN_THREADS - 1) carry_s = before + incl;
    __syncthreads();
  }
  if (tid == 0) off[m] = carry_s;
}

// the last rs in [lo, hi] with off[rs] <= j (off[lo] <= j is given)
__device__ __forceinline__ int win_owner(const unsigned long long* __restrict__ off, int lo, int hi, unsigned long long j) {
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (off[mid] <= j) lo = mid; else hi = mid - 1; }
  return lo;
}

__global__ __launch_bounds__(256) void k_win_scatter(const GmHit* __restrict__ hits, const uint16_t* __restrict__ perm, const unsigned long long* __restrict__ off, int m, int hcap,
                                                     int read_base, gm_read_window_t* __restrict__ out) {
  __shared__ int range[2];
  const unsigned long long total = off[m];
  const unsigned long long j0 = (unsigned long long)blockIdx.x * blockDim.x, j = j0 + threadIdx.x;
  if (j0 >= total) return;
  if (threadIdx.x < 2) range[threadIdx.x] = win_owner(off, 0, m - 1, threadIdx.x == 0 ? j0 : min(j0 + blockDim.x - 1, total - 1));
  __syncthreads();
  if (j >= total) return;
  const int rs = win_owner(off, range[0], range[1], j);
  const uint32_t k = (uint32_t)(j - off[rs]);                           // < min(hit_cnt[rs], hcap)
  const size_t row = (size_t)rs * hcap;
  const uint32_t p = min((uint32_t)perm[row + k], (uint32_t)(hcap - 1));
  const uint2* h = (const uint2*)(hits + row + p);
  const uint2 a = h[0], b = h[1], c = h[2], e = h[4];                   // g_off ax | ay alen | awidth score_window_gen | (score_vector pct_score_vector) | cn w_len matches flags
  uint4 r0, r1, r2;
  r0.x = (uint32_t)(read_base + (rs >> 1)); r0.y = (uint32_t)(rs & 1); r0.z = e.x & 0xFFFFu; r0.w = a.x;       // read st cn g_off
  r1.x = e.x >> 16; r1.y = c.y; r1.z = e.y & 0xFFFFu; r1.w = a.y;                                                // w_len score_window_gen matches ax
  r2.x = b.x; r2.y = b.y; r2.z = c.x; r2.w = 0;                                                                  // ay alen awidth reserved
  uint4* o = (uint4*)(out + j);
  o[0] = r0; o[1] = r1; o[2] = r2;
}

int gm_launch_win_scan(const uint32_t* d_hit_cnt, int n_rs, int hcap, unsigned long long* d_off, hipStream_t stream) {
  if (n_rs <= 0 || hcap < 1) { gm_set_error("gm_launch_win_scan: nothing to scan"); return GM_E_ARG; }
  hipLaunchKernelGGL(k_win_scan, dim3(1), dim3(WIN_SCAN_THREADS), 0, stream, d_hit_cnt, n_rs, hcap, d_off);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_win_scatter(const GmHit* d_hits, const uint16_t* d_perm, const unsigned long long* d_off, int n_rs, int hcap, unsigned long long total, int read_base,
                          gm_read_window_t* d_out, hipStream_t stream) {
  if (total == 0) return GM_OK;
  if (n_rs <= 0 || hcap < 1 || total > (unsigned long long)n_rs * (unsigned long long)hcap) { gm_set_error("gm_launch_win_scatter: %llu windows in %d rows of %d", total, n_rs, hcap); return GM_E_ARG; }
  const unsigned long long blocks = (total + 255) / 256;                // <= 2 * 131 072 * 32 768 / 256 = 2^25
  hipLaunchKernelGGL(k_win_scatter, dim3((unsigned)blocks), dim3(256), 0, stream, d_hits, d_perm, d_off, n_rs, hcap, read_base, d_out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
