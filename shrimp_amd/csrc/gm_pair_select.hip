// gm_pair_select.hip -- the pair selection of paired pass 2 on the device (gm_pair_mappings, gfx950 only).  gm_map_pairs* keeps its host loop (pair_pass2,
// gm_host_pairs.inc); these kernels restate readpair_pass2's selection (ref: gmapper/mapping.c:2181-2314) on the records the paired pass 2 left on the device.
//
//   k_pair_sel_items:  a lane a window of the paired pass 2: the item the selection reads of it -- (cn, gen_st), the two sort keys of
//                      readpair_remove_duplicate_hits, score_max and sort_idx from the device's GmFullRes, score_full from the host's answer (hit_run_post_sw's double
//                      arithmetic stays with the host's libm).
//   k_sel_pair_pass2:  a WAVE a pair, a lane a candidate pair of the pair heap's list (at most 64).  A lane carries both windows' items.  Nothing is moved: a lane keeps
//                      its position in the list, a stable sort is a rank by counting over the 64 lanes (sel2_rank of gm_select.hip with a winner), and the first
//                      maximum of a run of equal keys is the lane no equal lane beats.  Steps, in the reference's order:
//                        1. both windows aligned (score_full != 0, :2243-2245) and the summed score at or above the threshold (:2246-2262): the integer threshold is
//                           read from a table the host filled with its own double expression, one entry per possible sum of the two score_max;
//                        2. readpair_push_dominant_single_hits four times (:2083-2110, :2113-2175): mate 0 by genome start, by genome end, mate 1 likewise -- every lane
//                           of a run of equal keys takes the window of the run's first maximum score_full; the pair's score, pct and key follow (compute_paired_hit);
//                        3. the stable sort by (sort_idx, sort_idx) (:2004-2050) and the removal of equal neighbours (common/util.c:1240-1255);
//                        4. the stable sort by descending key;
//                        5. num_outputs, strata (the leading run of equal score), max_alignments (:2264-2284).
//                      Output: out[pr * 64 + k] = (window of mate 0 << 8) | window of mate 1 of the k-th final pair, cnt[pr] their number.
// No atomics, no LDS, no double arithmetic: the outcome depends on the input alone.
#include "gm_common.h"
#include "gm_internal.h"

static_assert(sizeof(GmPairSelItem) == 24, "GmPairSelItem: 6 x 32 bits");

__global__ void k_pair_sel_items(int n, const GmFullRes* __restrict__ res, const int32_t* __restrict__ score_full, GmPairSelItem* __restrict__ items) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const GmFullRes r = res[i];
  GmPairSelItem it;
  it.grp = (int32_t)(r.cn * 2u) + (int32_t)r.gen_st;
  it.start = r.genome_start;                                             // cmp_gen_start, ref: mapping.c:1485-1494
  it.endkey = -r.genome_start - r.rmapped + r.n_del - r.n_ins;           // cmp_gen_end, ref: mapping.c:1496-1506
  it.score_full = score_full[i]; it.score_max = r.score_max; it.sort_idx = r.sort_idx;
  items[i] = it;
}

// one mate's window as a lane holds it
struct PsWin { int h, grp, start, endkey, sf, smax, sidx; };
__device__ __forceinline__ PsWin ps_shfl(const PsWin& w, int src) {
  PsWin o; o.h = __shfl(w.h, src); o.grp = __shfl(w.grp, src); o.start = __shfl(w.start, src); o.endkey = __shfl(w.endkey, src);
  o.sf = __shfl(w.sf, src); o.smax = __shfl(w.smax, src); o.sidx = __shfl(w.sidx, src);
  return o;
}
// position of a lane after a stable sort by (k1, k2) of the lanes alive, counted over the wave; *winner: the lane of the first maximum `val` among the alive lanes
// with equal (k1, k2) -- the largest val, and of equal ones the earliest position (the lane itself when no other beats it)
__device__ __forceinline__ int ps_rank(bool alive, int k1, int k2, int val, int pos, int lane, int* winner) {
  int rank = 0, wl = lane, wv = val, wp = pos;
  for (int j = 0; j < GM_WAVE; j++) {
    const int aj = __shfl((int)alive, j);
    if (!aj) continue;                                                   // (wave-uniform)
    const int k1j = __shfl(k1, j), k2j = __shfl(k2, j), vj = __shfl(val, j), pj = __shfl(pos, j);
    const bool lt = k1j < k1 || (k1j == k1 && k2j < k2), eq = k1j == k1 && k2j == k2;
    rank += (lt || (eq && pj < pos)) ? 1 : 0;
    if (eq && (vj > wv || (vj == wv && pj < wp))) { wl = j; wv = vj; wp = pj; }
  }
  *winner = wl;
  return rank;
}

__global__ __launch_bounds__(GM_WAVE) void k_sel_pair_pass2(int n_pairs, int abs_key, int num_outputs, int strata, int max_alignments,
                                                            const int* __restrict__ thr_tab, int thr_n,
                                                            const uint32_t* __restrict__ plist, const uint32_t* __restrict__ pcnt,
                                                            const GmPairSelItem* __restrict__ items0, const uint32_t* __restrict__ off0, const uint32_t* __restrict__ cnt0,
                                                            const GmPairSelItem* __restrict__ items1, const uint32_t* __restrict__ off1, const uint32_t* __restrict__ cnt1,
                                                            uint32_t* __restrict__ out, uint32_t* __restrict__ cnt) {
  const int pr = blockIdx.x, lane = threadIdx.x;
  if (pr >= n_pairs) return;
  const int np = min((int)pcnt[pr], GM_SEL_MAX);
  const int c0 = (int)cnt0[pr], c1 = (int)cnt1[pr];
  PsWin w[2]; bool alive = false;
  for (int m = 0; m < 2; m++) { w[m].h = 0; w[m].grp = 0; w[m].start = 0; w[m].endkey = 0; w[m].sf = 0; w[m].smax = 0; w[m].sidx = 0; }
  if (lane < np) {
    const uint32_t p = plist[(size_t)pr * GM_SEL_MAX + lane];
    const int a = (int)(p >> 8), b = (int)(p & 0xffu);
    if (a < c0 && b < c1) {                                              // (a pair that names a window outside its lists is passed over; the host checks the count)
      const GmPairSelItem x = items0[(size_t)off0[pr] + a], y = items1[(size_t)off1[pr] + b];
      w[0].h = a; w[0].grp = x.grp; w[0].start = x.start; w[0].endkey = x.endkey; w[0].sf = x.score_full; w[0].smax = x.score_max; w[0].sidx = x.sort_idx;
      w[1].h = b; w[1].grp = y.grp; w[1].start = y.start; w[1].endkey = y.endkey; w[1].sf = y.score_full; w[1].smax = y.score_max; w[1].sidx = y.sort_idx;
      const int smax = x.score_max + y.score_max;
      const int thr = (smax >= 0 && smax < thr_n) ? thr_tab[smax] : 0x7fffffff;
      alive = x.score_full != 0 && y.score_full != 0 && x.score_full + y.score_full >= thr;
    }
  }
  int pos = lane, wl;
  // readpair_remove_duplicate_hits: the four dominance passes
  for (int pass = 0; pass < 4; pass++) {
    const int nip = pass >> 1;
    const PsWin me = w[nip];
    pos = ps_rank(alive, me.grp, (pass & 1) ? me.endkey : me.start, me.sf, pos, lane, &wl);
    const PsWin win = ps_shfl(me, wl);                                   // (every lane shuffles; a lane that is its own winner keeps what it has)
    if (alive) w[nip] = win;
  }
  // (sort_idx, sort_idx), equal neighbours removed: the first of a run stays
  pos = ps_rank(alive, w[0].sidx, w[1].sidx, 0, pos, lane, &wl);
  alive = alive && wl == lane;
  // compute_paired_hit's score and key (ref: mapping.c:2053-2080)
  const int score = w[0].sf + w[1].sf, smax = w[0].smax + w[1].smax;
  const int key = abs_key ? score : (smax ? (1000 * 100 * score) / smax : 0);
  pos = ps_rank(alive, -key, 0, 0, pos, lane, &wl);                      // descending key, stable
  alive = alive && pos < num_outputs;
  if (strata) {                                                          // the leading run of equal score
    const unsigned long long top = __ballot(alive && pos == 0);
    if (top) {
      const int s0 = __shfl(score, __builtin_ctzll(top));
      int first_other = alive && score != s0 ? pos : 0x7fffffff;
      for (int d = 32; d > 0; d >>= 1) first_other = min(first_other, __shfl_xor(first_other, d));
      alive = alive && pos < first_other;
    }
  }
  int m = __popcll(__ballot(alive));
  if (max_alignments != 0 && m > max_alignments) { alive = false; m = 0; }
  if (alive && pos < GM_SEL_MAX) out[(size_t)pr * GM_SEL_MAX + pos] = ((uint32_t)w[0].h << 8) | (uint32_t)w[1].h;
  if (lane == 0) cnt[pr] = (uint32_t)m;
}

int gm_launch_pair_sel_items(int n, const GmFullRes* d_res, const int32_t* d_score_full, GmPairSelItem* d_items, hipStream_t stream) {
  if (n <= 0) return GM_OK;
  hipLaunchKernelGGL(k_pair_sel_items, dim3((n + 255) / 256), dim3(256), 0, stream, n, d_res, d_score_full, d_items);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_sel_pair_pass2(int n_pairs, int abs_key, int num_outputs, int strata, int max_alignments, const int* d_thr_tab, int thr_n, const uint32_t* d_plist,
                             const uint32_t* d_pcnt, const GmPairSelItem* d_items0, const uint32_t* d_off0, const uint32_t* d_cnt0, const GmPairSelItem* d_items1,
                             const uint32_t* d_off1, const uint32_t* d_cnt1, uint32_t* d_out, uint32_t* d_cnt, hipStream_t stream) {
  if (n_pairs <= 0 || thr_n < 1 || !d_thr_tab) { gm_set_error("gm_launch_sel_pair_pass2: %d pairs, a threshold table of %d", n_pairs, thr_n); return GM_E_ARG; }
  hipLaunchKernelGGL(k_sel_pair_pass2, dim3(n_pairs), dim3(GM_WAVE), 0, stream, n_pairs, abs_key, num_outputs, strata, max_alignments, d_thr_tab, thr_n, d_plist, d_pcnt,
                     d_items0, d_off0, d_cnt0, d_items1, d_off1, d_cnt1, d_out, d_cnt);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
