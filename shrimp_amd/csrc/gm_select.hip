// gm_select.hip -- the two selection seams on caller arrays (gm_select_pass1 / gm_select_pass2, gfx950 only).  The pipeline's own k_pass1 / k_select and the host
// finalisation are not touched: these kernels restate the same rules on tight arrays.
//
//   k_sel_pass1:  a WAVE a read: strand 0, then strand 1, 64 windows a step (ref: read_pass1_per_strand mapping.c:1261-1339, read_get_vector_hits :1376-1411,
//                 ext-heap heap.h:226-327).  The overlap rule is a chain among the windows at or above the threshold only -- a window below it never becomes
//                 last_good and cannot enter the heap whether it is skipped or not -- so a step ballots those lanes and walks them with ctz, (cn, g_off) of the
//                 last passing window carried in scalars across steps.  What survives goes through the heap, which lane 0 keeps in LDS (insert + percolate-up with
//                 a strict <, replace-min + percolate-down): typically a handful of windows a read.  Left behind: the heap's ARRAY order as window indices + the
//                 scores after the rule, K slots a read.
//   k_sel_pass1_f1: the same with the f1 call cache of the reference (gm_select_pass1_f1, gm_read_hits); a kernel of its own, k_sel_pass1 is what it was.
//   k_sel_emit:   a wave a read, a lane a selected hit: the 64-byte record, strand 1 turned as reverse_hit / anchor_reverse turn it (mapping.c:254-263, anchors.h:30-34),
//                 stored as four 16-byte stores at hit_off[read] + slot.
//   k_sel_pass2:  a wave a read, a lane a pass-2 item (at most 64): the two duplicate-removal passes, the score sort, the cut, strata and max_alignments
//                 (ref: read_pass2 mapping.c:1628-1750, read_remove_duplicate_hits :1552-1600).  Nothing is moved: an item carries its position, a stable sort
//                 is a rank by counting over the 64 lanes, and the first maximum of an equal run is the item no equal item beats.
#include "gm_common.h"
#include "gm_internal.h"

static_assert(sizeof(gm_read_window_t) == 48, "gm_read_window_t: 12 x 32 bits");
static_assert(sizeof(gm_pass1_hit_t) == 64, "gm_pass1_hit_t: 16 x 32 bits");
static_assert(sizeof(GmSel2Item) == 24, "GmSel2Item: 6 x 32 bits");

__device__ __forceinline__ int sel_thr_of(double frac, int absval, int base) { return frac < 0 ? absval : (int)((double)base * frac); }

__global__ __launch_bounds__(GM_WAVE) void k_sel_pass1(GmScoreDev sc, int n_reads, int read_len, int K, uint32_t W, uint32_t overlap_abs,
                                                       const gm_read_window_t* __restrict__ wins, const unsigned long long* __restrict__ off,
                                                       const int* __restrict__ scores, int32_t* __restrict__ sel_id, int32_t* __restrict__ sel_score,
                                                       uint32_t* __restrict__ sel_cnt) {
  __shared__ int hk[GM_SEL_MAX], hid[GM_SEL_MAX], hsc[GM_SEL_MAX];
  __shared__ int load_s;
  const int rd = blockIdx.x, lane = threadIdx.x;
  if (rd >= n_reads) return;
  const bool absthr = sc.vect_thr_frac < 0;
  int load = 0;                                                          // (lane 0's)
  for (int st = 0; st < 2; st++) {
    const unsigned long long a = off[2 * (size_t)rd + st], b = off[2 * (size_t)rd + st + 1];
    int last_cn = -1; uint32_t last_goff = 0;                            // last_good, reset at every read-strand (wave-uniform)
    for (unsigned long long base = a; base < b; base += GM_WAVE) {
      const unsigned long long i = base + lane;
      const bool have = i < b;
      int cn = -1, w_len = 1, matches = 0, score = 0; uint32_t goff = 0;
      if (have) { const uint4 w0 = *(const uint4*)(wins + i); const uint2 w1 = *(const uint2*)((const uint32_t*)(wins + i) + 4);
                  cn = (int)w0.z; goff = w0.w; w_len = (int)w1.x; matches = (int)((const uint32_t*)(wins + i))[6]; score = scores[i]; }
      const int score_max = (read_len < w_len ? read_len : w_len) * sc.match;
      const int thr = sel_thr_of(sc.vect_thr_frac, sc.vect_abs, score_max);
      const bool elig = have && matches >= sc.min_matches;               // ref: mapping.c:1275
      // a window that matters: it can become last_good (score >= thr) or, skipped and so counted with score 0, still reach the heap (only with thr <= 0)
      unsigned long long bal = __ballot(elig && (score >= thr || 0 >= thr));
      bool adm = false; int fin = score;
      while (bal) {
        const int l = __builtin_ctzll(bal); bal &= bal - 1;
        const int cn_l = __shfl(cn, l); const uint32_t goff_l = (uint32_t)__shfl((int)goff, l); const int pass_l = __shfl((int)(score >= thr), l);
        const bool skip = last_cn >= 0 && cn_l == last_cn && (unsigned long long)goff_l + overlap_abs <= (unsigned long long)(uint32_t)(last_goff + W);   // ref :1287-1293
        if (skip) { if (lane == l) { fin = 0; adm = 0 >= thr; } }
        else if (pass_l) { last_cn = cn_l; last_goff = goff_l; if (lane == l) adm = true; }     // ref :1332-1335
      }
      const int pct = score_max ? (1000 * 100 * fin) / score_max : 0;
      const int key = absthr ? fin : pct;
      unsigned long long ab = __ballot(adm);
      while (ab) {                                                       // ref: mapping.c:1391-1404, in list order
        const int l = __builtin_ctzll(ab); ab &= ab - 1;
        const int k = __shfl(key, l), f = __shfl(fin, l);
        if (lane == 0) {
          const int me = (int)(base + l);
          if (load < K) {                                                // extheap insert + percolate_up (strict <)
            hk[load] = k; hid[load] = me; hsc[load] = f; load++;
            int node = load, parent = node / 2;
            while (node > 1 && hk[node - 1] < hk[parent - 1]) {
              int t = hk[parent - 1]; hk[parent - 1] = hk[node - 1]; hk[node - 1] = t;
              t = hid[parent - 1]; hid[parent - 1] = hid[node - 1]; hid[node - 1] = t;
              t = hsc[parent - 1]; hsc[parent - 1] = hsc[node - 1]; hsc[node - 1] = t;
              node = parent; parent = node / 2;
            }
          } else if (k > hk[0]) {                                        // replace_min + percolate_down
            hk[0] = k; hid[0] = me; hsc[0] = f;
            int node = 1;
            for (;;) {
              const int left = node * 2, right = left + 1; int mn = node;
              if (left <= load && hk[left - 1] < hk[node - 1]) mn = left;
              if (right <= load && hk[right - 1] < hk[mn - 1]) mn = right;
              if (mn == node) break;
              int t = hk[mn - 1]; hk[mn - 1] = hk[node - 1]; hk[node - 1] = t;
              t = hid[mn - 1]; hid[mn - 1] = hid[node - 1]; hid[node - 1] = t;
              t = hsc[mn - 1]; hsc[mn - 1] = hsc[node - 1]; hsc[node - 1] = t;
              node = mn;
            }
          }
        }
      }
    }
  }
  if (lane == 0) load_s = load;
  __syncthreads();
  const int n = load_s;                                                  // <= K <= 64
  if (lane < n) { sel_id[(size_t)rd * K + lane] = hid[lane]; sel_score[(size_t)rd * K + lane] = hsc[lane]; }
  if (lane == 0) sel_cnt[rd] = (uint32_t)n;
}

// the ext-heap of k_sel_pass1 (lane 0's, in LDS) as a routine of the kernel below: insert + percolate-up with a strict <, or replace-min + percolate-down
__device__ __forceinline__ void sel_heap_offer(int* hk, int* hid, int* hsc, int& load, const int K, const int k, const int me, const int f) {
  if (load < K) {
    hk[load] = k; hid[load] = me; hsc[load] = f; load++;
    int node = load, parent = node / 2;
    while (node > 1 && hk[node - 1] < hk[parent - 1]) {
      int t = hk[parent - 1]; hk[parent - 1] = hk[node - 1]; hk[node - 1] = t;
      t = hid[parent - 1]; hid[parent - 1] = hid[node - 1]; hid[node - 1] = t;
      t = hsc[parent - 1]; hsc[parent - 1] = hsc[node - 1]; hsc[node - 1] = t;
      node = parent; parent = node / 2;
    }
  } else if (k > hk[0]) {
    hk[0] = k; hid[0] = me; hsc[0] = f;
    int node = 1;
    for (;;) {
      const int left = node * 2, right = left + 1; int mn = node;
      if (left <= load && hk[left - 1] < hk[node - 1]) mn = left;
      if (right <= load && hk[right - 1] < hk[mn - 1]) mn = right;
      if (mn == node) break;
      int t = hk[mn - 1]; hk[mn - 1] = hk[node - 1]; hk[node - 1] = t;
      t = hid[mn - 1]; hid[mn - 1] = hid[node - 1]; hid[node - 1] = t;
      t = hsc[mn - 1]; hsc[mn - 1] = hsc[node - 1]; hsc[node - 1] = t;
      node = mn;
    }
  }
}

// k_sel_pass1 with the f1 call cache (hash_filter_calls; ref: f1_run f1-wrapper.h:97-134, the tag advances once per read-strand, mapping.c:1268).  A window that gets
// past the matches check and the overlap check takes the score of the FIRST earlier window of its read-strand that was itself computed and has the same cache slot
// (one bypassed call), else keeps its own and becomes computed.  The taken score decides last_good, so the chain runs over EVERY eligible window in list order, not
// over those at the threshold only: a step ballots the eligible lanes and walks them with ctz.  comp[off[2 r + st] ..]: the (slot | score << 32) pairs of the
// read-strand's computed windows, written by lane 0 and searched 64 a ballot (as k_pass1 searches its list); a read-strand has at most as many as it has windows.
__global__ __launch_bounds__(GM_WAVE) void k_sel_pass1_f1(GmScoreDev sc, int n_reads, int read_len, int K, uint32_t W, uint32_t overlap_abs,
                                                          const gm_read_window_t* __restrict__ wins, const unsigned long long* __restrict__ off,
                                                          const int* __restrict__ scores, const uint32_t* __restrict__ slots, unsigned long long* comp,
                                                          int32_t* __restrict__ sel_id, int32_t* __restrict__ sel_score, uint32_t* __restrict__ sel_cnt,
                                                          uint32_t* __restrict__ byp) {
  __shared__ int hk[GM_SEL_MAX], hid[GM_SEL_MAX], hsc[GM_SEL_MAX];
  __shared__ int load_s;
  const int rd = blockIdx.x, lane = threadIdx.x;
  if (rd >= n_reads) return;
  const bool absthr = sc.vect_thr_frac < 0;
  int load = 0;                                                          // (lane 0's)
  uint32_t bypassed = 0;
  for (int st = 0; st < 2; st++) {
    const unsigned long long a = off[2 * (size_t)rd + st], b = off[2 * (size_t)rd + st + 1];
    int last_cn = -1; uint32_t last_goff = 0;                            // last_good, reset at every read-strand (wave-uniform)
    unsigned long long* SL = comp + a; int n_comp = 0;                   // a new tag: nothing of another read-strand is found
    for (unsigned long long base = a; base < b; base += GM_WAVE) {
      const unsigned long long i = base + lane;
      const bool have = i < b;
      int cn = -1, w_len = 1, matches = 0, score = 0; uint32_t goff = 0, slot = 0;
      if (have) { const uint4 w0 = *(const uint4*)(wins + i); const uint2 w1 = *(const uint2*)((const uint32_t*)(wins + i) + 4);
                  cn = (int)w0.z; goff = w0.w; w_len = (int)w1.x; matches = (int)((const uint32_t*)(wins + i))[6]; score = scores[i]; slot = slots[i]; }
      const int score_max = (read_len < w_len ? read_len : w_len) * sc.match;
      const int thr = sel_thr_of(sc.vect_thr_frac, sc.vect_abs, score_max);
      unsigned long long bal = __ballot(have && matches >= sc.min_matches);      // ref: mapping.c:1275
      bool adm = false; int fin = score;
      while (bal) {
        const int l = __builtin_ctzll(bal); bal &= bal - 1;
        const int cn_l = __shfl(cn, l); const uint32_t goff_l = (uint32_t)__shfl((int)goff, l);
        const bool skip = last_cn >= 0 && cn_l == last_cn && (unsigned long long)goff_l + overlap_abs <= (unsigned long long)(uint32_t)(last_goff + W);   // ref :1287-1293
        if (skip) { if (lane == l) { fin = 0; adm = 0 >= thr; } continue; }
        const uint32_t slot_l = (uint32_t)__shfl((int)slot, l); const int own_l = __shfl(score, l), thr_l = __shfl(thr, l);
        int found = -1;                                                  // f1_run's look-up, ref: f1-wrapper.h:105-114
        for (int c0 = 0; c0 < n_comp; c0 += GM_WAVE) {
          const int c = c0 + lane;
          const bool hit = c < n_comp && (uint32_t)__hip_atomic_load(&SL[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == slot_l;
          const unsigned long long hb = __ballot(hit);
          if (hb) { found = c0 + __builtin_ctzll(hb); break; }
        }
        int taken = own_l;
        if (found >= 0) { taken = (int)(uint32_t)(__hip_atomic_load(&SL[found], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32); bypassed++; }
        else {                                                           // computed: saved under its slot, ref :128-131
          if (lane == 0) __hip_atomic_store(&SL[n_comp], (unsigned long long)slot_l | ((unsigned long long)(uint32_t)own_l << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          n_comp++; __syncthreads();
        }
        const bool pass_l = taken >= thr_l;
        if (pass_l) { last_cn = cn_l; last_goff = goff_l; }              // ref: mapping.c:1332-1335
        if (lane == l) { fin = taken; adm = pass_l; }
      }
      const int pct = score_max ? (1000 * 100 * fin) / score_max : 0;
      const int key = absthr ? fin : pct;
      unsigned long long ab = __ballot(adm);
      while (ab) {                                                       // ref: mapping.c:1391-1404, in list order
        const int l = __builtin_ctzll(ab); ab &= ab - 1;
        const int k = __shfl(key, l), f = __shfl(fin, l);
        if (lane == 0) sel_heap_offer(hk, hid, hsc, load, K, k, (int)(base + l), f);
      }
    }
  }
  if (lane == 0) load_s = load;
  __syncthreads();
  const int n = load_s;                                                  // <= K <= 64
  if (lane < n) { sel_id[(size_t)rd * K + lane] = hid[lane]; sel_score[(size_t)rd * K + lane] = hsc[lane]; }
  if (lane == 0) { sel_cnt[rd] = (uint32_t)n; byp[rd] = bypassed; }
}

__global__ __launch_bounds__(GM_WAVE) void k_sel_emit(GmScoreDev sc, int n_reads, int read_len, int K, const gm_read_window_t* __restrict__ wins,
                                                      const uint32_t* __restrict__ contig_off, const int32_t* __restrict__ sel_id, const int32_t* __restrict__ sel_score,
                                                      const uint32_t* __restrict__ sel_cnt, const unsigned long long* __restrict__ hit_off, gm_pass1_hit_t* __restrict__ out) {
  const int rd = blockIdx.x, lane = threadIdx.x;
  if (rd >= n_reads || lane >= (int)sel_cnt[rd]) return;
  const int id = sel_id[(size_t)rd * K + lane], score = sel_score[(size_t)rd * K + lane];
  const uint4* w = (const uint4*)(wins + id);
  const uint4 a = w[0], b = w[1], c = w[2];                              // read st cn g_off | w_len score_window_gen matches ax | ay alen awidth reserved
  const int st = (int)a.y, cn = (int)a.z, w_len = (int)b.x;
  uint32_t goff = a.w; int ax = (int)b.w, ay = (int)c.x; const int alen = (int)c.y, awidth = (int)c.z;
  if (st) {                                                              // reverse_hit
    goff = (contig_off[cn + 1] - contig_off[cn]) - goff - (uint32_t)w_len;
    ax = -ax + (w_len - 1) - (alen - 1) - (awidth - 1);
    ay = -ay + (read_len - 1) - (alen - 1) + (awidth - 1);
  }
  const int score_max = (read_len < w_len ? read_len : w_len) * sc.match;
  uint4 r0, r1, r2, r3;
  r0.x = a.x; r0.y = a.y; r0.z = (uint32_t)id; r0.w = a.z;                                                        // read st win cn
  r1.x = (uint32_t)st; r1.y = goff; r1.z = b.x; r1.w = (uint32_t)score;                                           // gen_st g_off w_len score_vector
  r2.x = (uint32_t)(score_max ? (1000 * 100 * score) / score_max : 0); r2.y = (uint32_t)score_max; r2.z = b.z; r2.w = b.y;   // pct_score_vector score_max matches score_window_gen
  r3.x = (uint32_t)ax; r3.y = (uint32_t)ay; r3.z = c.y; r3.w = c.z;                                               // ax ay alen awidth
  uint4* o = (uint4*)(out + hit_off[rd] + lane);
  o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
}

// position of an item after a stable sort by (k1, k2) of the items alive, counted over the lanes; *beaten: an alive item with equal (k1, k2) has a larger key, or
// the same key and an earlier position -- the item is not the first maximum of its run
__device__ __forceinline__ int sel2_rank(bool alive, int k1, int k2, int key, int pos, bool* beaten) {
  int rank = 0; bool bt = false;
  for (int j = 0; j < GM_WAVE; j++) {
    const int aj = __shfl((int)alive, j);
    if (!aj) continue;                                                   // (wave-uniform)
    const int k1j = __shfl(k1, j), k2j = __shfl(k2, j), keyj = __shfl(key, j), posj = __shfl(pos, j);
    const bool lt = k1j < k1 || (k1j == k1 && k2j < k2), eq = k1j == k1 && k2j == k2;
    rank += (lt || (eq && posj < pos)) ? 1 : 0;
    bt = bt || (eq && (keyj > key || (keyj == key && posj < pos)));
  }
  *beaten = bt;
  return rank;
}

__global__ __launch_bounds__(GM_WAVE) void k_sel_pass2(int n_reads, int num_outputs, int strata, int max_alignments, const unsigned long long* __restrict__ hit_off,
                                                       const GmSel2Item* __restrict__ items, int32_t* __restrict__ order, uint32_t* __restrict__ cnt) {
  const int rd = blockIdx.x, lane = threadIdx.x;
  if (rd >= n_reads) return;
  const unsigned long long a = hit_off[rd];
  const int n = (int)(hit_off[rd + 1] - a);                              // <= 64 (the host checked)
  GmSel2Item it; it.grp = 0; it.start = 0; it.endkey = 0; it.key = 0; it.score_full = 0; it.keep = 0;
  if (lane < n) it = items[a + lane];
  bool alive = lane < n && it.keep != 0;                                 // the threshold (a double compare, made on the host; ref: mapping.c:1661)
  int pos = lane; bool beaten;
  pos = sel2_rank(alive, it.grp, it.start, it.key, pos, &beaten); alive = alive && !beaten;       // by (cn, gen_st, genome_start)
  pos = sel2_rank(alive, it.grp, it.endkey, it.key, pos, &beaten); alive = alive && !beaten;      // by (cn, gen_st, -genome_start - rmapped + deletions - insertions)
  pos = sel2_rank(alive, -it.key, 0, 0, pos, &beaten);                                             // descending key, stable (ref :1479-1482,1678)
  alive = alive && pos < num_outputs;
  if (strata) {                                                          // the leading run of equal score_full, ref :1706-1712
    const unsigned long long top = __ballot(alive && pos == 0);
    if (top) {
      const int sf0 = __shfl(it.score_full, __builtin_ctzll(top));
      int first_other = alive && it.score_full != sf0 ? pos : 0x7fffffff;
      for (int d = 32; d > 0; d >>= 1) first_other = min(first_other, __shfl_xor(first_other, d));
      alive = alive && pos < first_other;
    }
  }
  int m = __popcll(__ballot(alive));
  if (max_alignments != 0 && m > max_alignments) { alive = false; m = 0; }   // ref :1713-1722
  if (alive) order[a + pos] = lane;
  if (lane == 0) cnt[rd] = (uint32_t)m;
}

int gm_launch_sel_pass1(const GmScoreDev& sc, int n_reads, int read_len, int K, int window_len, int overlap_abs, const gm_read_window_t* d_wins,
                        const unsigned long long* d_off, const int* d_scores, int32_t* d_sel_id, int32_t* d_sel_score, uint32_t* d_sel_cnt, hipStream_t stream) {
  if (n_reads <= 0 || K < 1 || K > GM_SEL_MAX) { gm_set_error("gm_launch_sel_pass1: %d reads, %d slots", n_reads, K); return GM_E_ARG; }
  hipLaunchKernelGGL(k_sel_pass1, dim3(n_reads), dim3(GM_WAVE), 0, stream, sc, n_reads, read_len, K, (uint32_t)window_len, (uint32_t)overlap_abs, d_wins, d_off, d_scores,
                     d_sel_id, d_sel_score, d_sel_cnt);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_sel_pass1_f1(const GmScoreDev& sc, int n_reads, int read_len, int K, int window_len, int overlap_abs, const gm_read_window_t* d_wins,
                           const unsigned long long* d_off, const int* d_scores, const uint32_t* d_slots, unsigned long long* d_comp, int32_t* d_sel_id,
                           int32_t* d_sel_score, uint32_t* d_sel_cnt, uint32_t* d_byp, hipStream_t stream) {
  if (n_reads <= 0 || K < 1 || K > GM_SEL_MAX || !d_slots || !d_comp || !d_byp) { gm_set_error("gm_launch_sel_pass1_f1: %d reads, %d slots", n_reads, K); return GM_E_ARG; }
  hipLaunchKernelGGL(k_sel_pass1_f1, dim3(n_reads), dim3(GM_WAVE), 0, stream, sc, n_reads, read_len, K, (uint32_t)window_len, (uint32_t)overlap_abs, d_wins, d_off, d_scores,
                     d_slots, d_comp, d_sel_id, d_sel_score, d_sel_cnt, d_byp);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_sel_emit(const GmScoreDev& sc, int n_reads, int read_len, int K, const gm_read_window_t* d_wins, const uint32_t* d_contig_off, const int32_t* d_sel_id,
                       const int32_t* d_sel_score, const uint32_t* d_sel_cnt, const unsigned long long* d_hit_off, gm_pass1_hit_t* d_out, hipStream_t stream) {
  if (n_reads <= 0 || K < 1 || K > GM_SEL_MAX) { gm_set_error("gm_launch_sel_emit: %d reads, %d slots", n_reads, K); return GM_E_ARG; }
  hipLaunchKernelGGL(k_sel_emit, dim3(n_reads), dim3(GM_WAVE), 0, stream, sc, n_reads, read_len, K, d_wins, d_contig_off, d_sel_id, d_sel_score, d_sel_cnt, d_hit_off, d_out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_sel_pass2(int n_reads, int num_outputs, int strata, int max_alignments, const unsigned long long* d_hit_off, const GmSel2Item* d_items,
                        int32_t* d_order, uint32_t* d_cnt, hipStream_t stream) {
  if (n_reads <= 0) { gm_set_error("gm_launch_sel_pass2: no reads"); return GM_E_ARG; }
  hipLaunchKernelGGL(k_sel_pass2, dim3(n_reads), dim3(GM_WAVE), 0, stream, n_reads, num_outputs, strata, max_alignments, d_hit_off, d_items, d_order, d_cnt);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
