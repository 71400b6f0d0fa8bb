// gm_pass2.hip -- the small kernels of gm_read_mappings (gm_host_pass2.inc) that stand where a caller's host glue stood between the batch seams: the rule of
// hit_run_full_sw (ref: gmapper/mapping.c:332-402) on the pass-1 hits of a sub-batch, which never leave the device (gfx950 only).
//
//   k_p2_items     a lane a hit: the pass-2 item of the hit -- its window resolved on the index as ix_window resolves it (strand 1: the lowest forward base, read
//                  backwards and complemented), the hit's anchor box, revcmpl = gen_st && tiebreak_rev, thresh = (int)abs_or_pct(sw_full_threshold, score_max), and the
//                  ROW of the sub-batch's reads the hit's read is in.  thresh comes from a table the HOST made with its own double expression, one entry per
//                  min(read_len, w_len) (score_max is that times the match score, k_sel_emit): no double is evaluated here.
//   k_p2_compact   the place of every hit with sv >= thresh in the full-alignment work list, in hit order.  One workgroup of 16 waves, a contiguous stretch of hits
//                  a wave: a ballot over 64 hits and a popcount below the lane give each passing hit its place, the waves' totals are prefix-summed through LDS.
//                  No atomics: the list's order, and with it every ops offset, is the hits' order whatever the timing.  It reads two dense words a hit (sv, thresh)
//                  and writes one, so that the one workgroup is no bottleneck; k_p2_scatter, a lane a hit over the whole device, then copies the passing items to
//                  their places with maxscore = sv.  Work item k owns ops[k * ops_cap ..).
//   k_p2_records   a lane a hit: the record of the hit as the batch entries leave it (genome_start counted on the strand's contig), the zero record for a hit under
//                  the threshold (calloc + score = 0, ref: mapping.c:365,396-398), and the three integers the host's double functions read of it.
//   k_p2_sel_items a lane a hit: k_sel_pass2's item from the record, the hit and the host's answer (score_full, key, the threshold compare).
// Colour space (gm_read_mappings_cs, gm_host_pass2_cs.inc; ref: mapping.c:375-379, 1609-1625) has no second score and no work list -- every hit is aligned -- and post_sw
// behind the alignment:
//   k_p2_items_cs   a lane a hit: the item in its colour-space by-row form (the primer letter stays in initbp, the row rides in maxscore), hit i's operations at i * ops_cap.
//   k_p2_records_cs a lane a hit: the record as gm_sw_full_cs_batch_ix leaves it, the host's three integers, the read positions post_sw takes (scanned by k_win_scan).
//   k_p2_post_items a lane a hit: k_post_sw_batch's item from the device record, the read named by its row, qual_off from the scan.
//   k_p2_move       a wave a segment: bytes between two device buffers by a list -- the flagged items' operations packed for the host, its re-called letters back.
#include "gm_common.h"
#include <algorithm>
#include "gm_internal.h"

static_assert(sizeof(gm_pass1_hit_t) == 64, "gm_pass1_hit_t: 16 x 32 bits");
static_assert(sizeof(gm_sw_full_rec_t) == 64, "gm_sw_full_rec_t: ten ints, two 64-bit words, n_ops and its padding");

#define P2_COMPACT_THREADS 1024
#define P2_COMPACT_WAVES (P2_COMPACT_THREADS / GM_WAVE)

__global__ __launch_bounds__(256) void k_p2_items(int n, const gm_pass1_hit_t* __restrict__ hits, int read_base, int read_len, const uint32_t* __restrict__ contig_off,
                                                  const uint8_t* __restrict__ contig_rna, const int* __restrict__ thresh_tab, int tiebreak_rev, int ops_cap,
                                                  GmFullItem* __restrict__ items, int* __restrict__ thresh) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* h = (const uint4*)(hits + i);
  const uint4 a = h[0], b = h[1], d = h[3];                                // read st win cn | gen_st g_off w_len score_vector | ... | ax ay alen awidth
  const int cn = (int)a.w, gen_st = (int)b.x, w_len = (int)b.z;
  const uint32_t c0 = contig_off[cn], clen = contig_off[cn + 1] - c0;
  const uint32_t foff = gen_st ? clen - b.y - (uint32_t)w_len : b.y;      // the window's lowest forward base (ix_window)
  GmFullItem it;
  it.goff = (long long)c0 + (long long)foff; it.glen = w_len; it.rlen = read_len;
  const bool has_anchor = (int)d.z > 0;                                    // (a box of no length: the threshold band, as the batch entries take it)
  it.ax = has_anchor ? (long long)(int)d.x : 0; it.ay = has_anchor ? (long long)(int)d.y : 0;
  it.alen = has_anchor ? (int)d.z : 1; it.awidth = has_anchor ? (int)d.w : 1;
  it.thresh = thresh_tab[min(read_len, w_len)]; it.maxscore = 0;
  it.flags = (has_anchor ? 1 : 0) | ((gen_st && tiebreak_rev) ? 2 : 0) | (gen_st ? 4 : 0) | ((contig_rna && contig_rna[cn]) ? 8 : 0);
  it.initbp = (int)a.x - read_base;                                        // letter space, by-row form: the row of the read (GmFullItem)
  it.ops_cap = ops_cap; it.ops_off = 0; it.idx = i;
  items[i] = it; thresh[i] = it.thresh;
}

__global__ __launch_bounds__(P2_COMPACT_THREADS) void k_p2_compact(int n, const int* __restrict__ thresh, const int* __restrict__ sv, int* __restrict__ pos_of,
                                                                   uint32_t* __restrict__ n_work) {
  __shared__ uint32_t wave_cnt[P2_COMPACT_WAVES];
  const int lane = threadIdx.x & (GM_WAVE - 1), wv = threadIdx.x / GM_WAVE;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int per = (int)((((long long)n + P2_COMPACT_THREADS - 1) / P2_COMPACT_THREADS) * GM_WAVE);      // hits a wave: a multiple of 64
  const int a0 = (int)min((long long)n, (long long)wv * per), a1 = (int)min((long long)n, (long long)a0 + per);
  uint32_t c = 0;
  for (int i0 = a0; i0 < a1; i0 += GM_WAVE) {
    const int i = i0 + lane;
    const bool pass = i < a1 && sv[i] >= thresh[i];
    c += (uint32_t)__popcll(__ballot(pass));
  }
  if (lane == 0) wave_cnt[wv] = c;
  __syncthreads();
  uint32_t at = 0;
  for (int w = 0; w < wv; w++) at += wave_cnt[w];
  for (int i0 = a0; i0 < a1; i0 += GM_WAVE) {
    const int i = i0 + lane;
    const bool in = i < a1;
    const bool pass = in && sv[i] >= thresh[i];
    const unsigned long long bal = __ballot(pass);
    if (in) pos_of[i] = pass ? (int)(at + (uint32_t)__popcll(bal & below)) : -1;
    at += (uint32_t)__popcll(bal);
  }
  if (threadIdx.x == P2_COMPACT_THREADS - 1) *n_work = at;               // (the last wave's cursor: every wave before it is counted in)
}

__global__ __launch_bounds__(256) void k_p2_scatter(int n, const GmFullItem* __restrict__ items, const int* __restrict__ sv, const int* __restrict__ pos_of,
                                                    GmFullItem* __restrict__ work) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = pos_of[i];
  if (k < 0) return;
  GmFullItem it = items[i];
  it.maxscore = sv[i]; it.ops_off = (unsigned long long)k * (unsigned long long)it.ops_cap;
  work[k] = it;
}

__global__ __launch_bounds__(256) void k_p2_records(int n, const gm_pass1_hit_t* __restrict__ hits, const int* __restrict__ pos_of, const GmFullOut* __restrict__ out,
                                                    int ops_cap, gm_sw_full_rec_t* __restrict__ recs, GmP2In* __restrict__ p2in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const gm_pass1_hit_t* h = hits + i;
  gm_sw_full_rec_t R;
  R.score = 0; R.read_start = 0; R.rmapped = 0; R.gmapped = 0; R.matches = 0; R.mismatches = 0; R.insertions = 0; R.deletions = 0; R.crossovers = 0; R.status = 0;
  R.genome_start = 0; R.ops_off = 0; R.n_ops = 0;
  const int k = pos_of[i];
  if (k >= 0) {
    const GmFullOut o = out[i];
    R.ops_off = (unsigned long long)k * (unsigned long long)ops_cap;
    if (o.v[0] > 0) {
      R.score = o.v[0]; R.read_start = o.v[1]; R.rmapped = o.v[2]; R.genome_start = (int64_t)h->g_off + o.v[3]; R.gmapped = o.v[4];
      R.matches = o.v[5]; R.mismatches = o.v[6]; R.insertions = o.v[7]; R.deletions = o.v[8];
      R.n_ops = (uint32_t)min(o.v[10], ops_cap);
    } else { R.rmapped = 1; R.gmapped = 1; R.genome_start = (int64_t)h->g_off; }      // as sw_full_ls leaves a window without alignment
  }
  uint4* dst = (uint4*)(recs + i); const uint4* src = (const uint4*)&R;
  ((uint32_t*)&R)[15] = 0;                                                 // (the padding behind n_ops)
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
  GmP2In q; q.score = R.score; q.rmapped = R.rmapped; q.score_max = h->score_max;
  p2in[i] = q;
}

__global__ __launch_bounds__(256) void k_p2_sel_items(int n, const gm_pass1_hit_t* __restrict__ hits, const gm_sw_full_rec_t* __restrict__ recs,
                                                      const GmP2Host* __restrict__ ans, GmSel2Item* __restrict__ items) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const gm_pass1_hit_t* h = hits + i; const gm_sw_full_rec_t* R = recs + i; const GmP2Host a = ans[i];
  GmSel2Item it;
  it.grp = h->cn * 2 + h->gen_st; it.start = (int32_t)R->genome_start;
  it.endkey = (int32_t)(-R->genome_start - R->rmapped + R->deletions - R->insertions);
  it.score_full = a.score_full; it.key = a.key; it.keep = a.keep;
  items[i] = it;
}

// ---- colour space (gm_read_mappings_cs): every hit is aligned, so there is no second score and no work list; post_sw follows on the device -----------------------
// k_p2_items_cs: k_p2_items with the colour-space by-row form of the item -- the primer letter (| GM_SEAM_RNA) in initbp, the read's row in maxscore, hit i's operations
// at i * ops_cap.
__global__ __launch_bounds__(256) void k_p2_items_cs(int n, const gm_pass1_hit_t* __restrict__ hits, int read_base, int read_len, const uint32_t* __restrict__ contig_off,
                                                     const uint8_t* __restrict__ contig_rna, const int* __restrict__ thresh_tab, int tiebreak_rev, int ops_cap,
                                                     const uint8_t* __restrict__ initbp_rows, int is_rna, GmFullItem* __restrict__ items) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4* h = (const uint4*)(hits + i);
  const uint4 a = h[0], b = h[1], d = h[3];                                // read st win cn | gen_st g_off w_len score_vector | ... | ax ay alen awidth
  const int cn = (int)a.w, gen_st = (int)b.x, w_len = (int)b.z, row = (int)a.x - read_base;
  const uint32_t c0 = contig_off[cn], clen = contig_off[cn + 1] - c0;
  const uint32_t foff = gen_st ? clen - b.y - (uint32_t)w_len : b.y;
  GmFullItem it;
  it.goff = (long long)c0 + (long long)foff; it.glen = w_len; it.rlen = read_len;
  const bool has_anchor = (int)d.z > 0;
  it.ax = has_anchor ? (long long)(int)d.x : 0; it.ay = has_anchor ? (long long)(int)d.y : 0;
  it.alen = has_anchor ? (int)d.z : 1; it.awidth = has_anchor ? (int)d.w : 1;
  it.thresh = thresh_tab[min(read_len, w_len)]; it.maxscore = row;
  it.flags = (has_anchor ? 1 : 0) | ((gen_st && tiebreak_rev) ? 2 : 0) | (gen_st ? 4 : 0) | ((contig_rna && contig_rna[cn]) ? 8 : 0);
  it.initbp = (int)initbp_rows[row] | (is_rna ? GM_SEAM_RNA : 0);
  it.ops_cap = ops_cap; it.ops_off = (unsigned long long)i * (unsigned long long)ops_cap; it.idx = i;
  items[i] = it;
}

// k_p2_records_cs: the record of a hit as gm_sw_full_cs_batch_ix leaves it -- all zero where sw_full_cs found no alignment at or above thresh -- the three integers of
// the host's double functions, and the read positions post_sw takes of it
__global__ __launch_bounds__(256) void k_p2_records_cs(int n, const gm_pass1_hit_t* __restrict__ hits, const GmFullOut* __restrict__ out, int ops_cap,
                                                       gm_sw_full_rec_t* __restrict__ recs, GmP2In* __restrict__ p2in, uint32_t* __restrict__ len) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const gm_pass1_hit_t* h = hits + i;
  gm_sw_full_rec_t R;
  R.score = 0; R.read_start = 0; R.rmapped = 0; R.gmapped = 0; R.matches = 0; R.mismatches = 0; R.insertions = 0; R.deletions = 0; R.crossovers = 0; R.status = 0;
  R.genome_start = 0; R.ops_off = 0; R.n_ops = 0;
  const GmFullOut o = out[i];
  if (o.v[0] > 0) {
    R.score = o.v[0]; R.read_start = o.v[1]; R.rmapped = o.v[2]; R.genome_start = (int64_t)h->g_off + o.v[3]; R.gmapped = o.v[4];
    R.matches = o.v[5]; R.mismatches = o.v[6]; R.insertions = o.v[7]; R.deletions = o.v[8]; R.crossovers = o.v[9];
    R.n_ops = (uint32_t)min(o.v[10], ops_cap); R.ops_off = (unsigned long long)i * (unsigned long long)ops_cap;
  }
  ((uint32_t*)&R)[15] = 0;                                                 // (the padding behind n_ops)
  uint4* dst = (uint4*)(recs + i); const uint4* src = (const uint4*)&R;
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
  GmP2In q; q.score = R.score; q.rmapped = R.rmapped; q.score_max = h->score_max;
  p2in[i] = q;
  len[i] = R.score > 0 ? (uint32_t)max(R.rmapped, 0) : 0u;
}

// k_p2_post_items: post_sw's item of a hit from its device record (the host has checked the records against their windows before this is launched)
__global__ __launch_bounds__(256) void k_p2_post_items(int n, const gm_pass1_hit_t* __restrict__ hits, const gm_sw_full_rec_t* __restrict__ recs,
                                                       const unsigned long long* __restrict__ qoff, int read_base, int read_len, const uint32_t* __restrict__ contig_off,
                                                       const uint8_t* __restrict__ contig_rna, const uint8_t* __restrict__ initbp_rows, GmPostItem* __restrict__ items) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const gm_pass1_hit_t* h = hits + i; const gm_sw_full_rec_t* R = recs + i;
  const int row = h->read - read_base, cn = h->cn, gen_st = h->gen_st;
  const uint32_t c0 = contig_off[cn], clen = contig_off[cn + 1] - c0;
  GmPostItem it;
  it.ops_off = 0; it.qual_off = qoff[i]; it.genome_start = 0; it.n_ops = 0; it.read_start = 0; it.len = 0;
  it.gbase = (long long)c0 + (gen_st ? (long long)clen - 1 : 0);
  it.rlen = read_len; it.initbp = (int)initbp_rows[row]; it.idx = row;
  it.flags = (gen_st ? 1 : 0) | ((contig_rna && contig_rna[cn]) ? 2 : 0);
  if (R->score > 0) { it.ops_off = R->ops_off; it.n_ops = R->n_ops; it.genome_start = R->genome_start; it.read_start = R->read_start; it.len = R->rmapped; }
  items[i] = it;
}

// k_p2_move: a wave a segment, a byte a lane and step
__global__ __launch_bounds__(GM_WAVE) void k_p2_move(int n_segs, const GmP2Seg* __restrict__ segs, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
  for (int k = blockIdx.x; k < n_segs; k += gridDim.x) {
    const GmP2Seg s = segs[k];
    for (uint32_t j = threadIdx.x; j < s.len; j += GM_WAVE) dst[s.dst + j] = src[s.src + j];
  }
}

int gm_launch_p2_items_cs(int n, const gm_pass1_hit_t* d_hits, int read_base, int read_len, const uint32_t* d_contig_off, const uint8_t* d_contig_rna, const int* d_thresh_tab,
                          int tiebreak_rev, int ops_cap, const uint8_t* d_initbp_rows, int is_rna, GmFullItem* d_items, hipStream_t stream) {
  if (n <= 0) return GM_OK;
  hipLaunchKernelGGL(k_p2_items_cs, dim3((n + 255) / 256), dim3(256), 0, stream, n, d_hits, read_base, read_len, d_contig_off, d_contig_rna, d_thresh_tab, tiebreak_rev, ops_cap,
                     d_initbp_rows, is_rna, d_items);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_p2_records_cs(int n, const gm_pass1_hit_t* d_hits, const GmFullOut* d_out, int ops_cap, gm_sw_full_rec_t* d_recs, GmP2In* d_p2in, uint32_t* d_len, hipStream_t stream) {
  if (n <= 0) return GM_OK;
  hipLaunchKernelGGL(k_p2_records_cs, dim3((n + 255) / 256), dim3(256), 0, stream, n, d_hits, d_out, ops_cap, d_recs, d_p2in, d_len);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_p2_post_items(int n, const gm_pass1_hit_t* d_hits, const gm_sw_full_rec_t* d_recs, const unsigned long long* d_qoff, int read_base, int read_len,
                            const uint32_t* d_contig_off, const uint8_t* d_contig_rna, const uint8_t* d_initbp_rows, GmPostItem* d_items, hipStream_t stream) {
  if (n <= 0) return GM_OK;
  hipLaunchKernelGGL(k_p2_post_items, dim3((n + 255) / 256), dim3(256), 0, stream, n, d_hits, d_recs, d_qoff, read_base, read_len, d_contig_off, d_contig_rna, d_initbp_rows, d_items);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_p2_move(int n_segs, const GmP2Seg* d_segs, const uint8_t* d_src, uint8_t* d_dst, hipStream_t stream) {
  if (n_segs <= 0) return GM_OK;
  hipLaunchKernelGGL(k_p2_move, dim3(std::min(n_segs, 4096)), dim3(GM_WAVE), 0, stream, n_segs, d_segs, d_src, d_dst);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_p2_items(int n, const gm_pass1_hit_t* d_hits, int read_base, int read_len, const uint32_t* d_contig_off, const uint8_t* d_contig_rna, const int* d_thresh_tab,
                       int tiebreak_rev, int ops_cap, GmFullItem* d_items, int* d_thresh, hipStream_t stream) {
  if (n <= 0) return GM_OK;
  hipLaunchKernelGGL(k_p2_items, dim3((n + 255) / 256), dim3(256), 0, stream, n, d_hits, read_base, read_len, d_contig_off, d_contig_rna, d_thresh_tab, tiebreak_rev, ops_cap, d_items,
                     d_thresh);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_p2_compact(int n, const GmFullItem* d_items, const int* d_thresh, const int* d_sv, GmFullItem* d_work, int* d_pos_of, uint32_t* d_n_work, hipStream_t stream) {
  if (n <= 0) { gm_set_error("gm_launch_p2_compact: no hits"); return GM_E_ARG; }
  hipLaunchKernelGGL(k_p2_compact, dim3(1), dim3(P2_COMPACT_THREADS), 0, stream, n, d_thresh, d_sv, d_pos_of, d_n_work);
  hipLaunchKernelGGL(k_p2_scatter, dim3((n + 255) / 256), dim3(256), 0, stream, n, d_items, d_sv, d_pos_of, d_work);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_p2_records(int n, const gm_pass1_hit_t* d_hits, const int* d_pos_of, const GmFullOut* d_out, int ops_cap, gm_sw_full_rec_t* d_recs, GmP2In* d_p2in,
                         hipStream_t stream) {
  if (n <= 0) return GM_OK;
  hipLaunchKernelGGL(k_p2_records, dim3((n + 255) / 256), dim3(256), 0, stream, n, d_hits, d_pos_of, d_out, ops_cap, d_recs, d_p2in);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

int gm_launch_p2_sel_items(int n, const gm_pass1_hit_t* d_hits, const gm_sw_full_rec_t* d_recs, const GmP2Host* d_ans, GmSel2Item* d_items, hipStream_t stream) {
  if (n <= 0) return GM_OK;
  hipLaunchKernelGGL(k_p2_sel_items, dim3((n + 255) / 256), dim3(256), 0, stream, n, d_hits, d_recs, d_ans, d_items);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
