// gm_text.hip -- the text of n alignments of one gm_sw_full_*_batch call, made on the device (gm_sw_full_batch_text[_ix], gm_host.hip): dbalign / qralign as
// gm_sw_full_batch_strings builds them, the CIGAR (make_cigar / reverse_cigar, ref: gmapper/output.c:15-80) and the edit string (alignment_edit_string, ref:
// common/output.c:60-121; reverse_alignment_edit_string, ref: gmapper/output.c:83-122).
//
//   k_sw_text   one wave per item (a block is one wave), grid-stride over the items; lane k takes column k of each 64-column step.
//
// The host has checked every item against the caller's buffers (swf_rec_check): ops[ops_off .. + n_ops), the genome positions and the read positions of the
// alignment all lie inside what was uploaded.  The kernel runs twice: the sizing launch (write = 0) leaves the CIGAR and edit-string lengths of every item in lens[],
// the host scans them into offsets, the writing launch stores every byte.  Both launches run the same code, so the sizes cannot disagree with the bytes.
//
// Columns.  An operation byte makes a column: a gap in the read (qgap: letter space 'I', colour space type 1), a gap in the genome (dgap: 'D', types 2-5) or a pair.
// The genome / read position of a column is the start plus the count of earlier columns that hold one: a ballot and a popcount inside a step, a running base between.
// Colour space: the read letter of a column comes from one of four translations of the colour read (cstols chain, ref: util.h:157-180).  On letters 0-3 cstols is
// XOR, so translation k at read position j is ((k + initbp) & 3) ^ X(j), X = the XOR of the colours since the last reset (a colour 15, or the read's start), and N
// once a colour 4-14 has been met since then.  The read positions of a step are a contiguous stretch of at most 64: lane r takes the r-th of them, X comes from the
// ballots of the two colour bits, and the column's lane fetches it by its rank.  The carry between steps is (X, the N flag); the colours before read_start are folded
// into it first.
// CIGAR.  A run's last column knows its length: the distance to the last column of another type, found in the ballot of run starts, or the carried length plus the
// lane.  Carry: the open run's type and length.
// Edit string.  Only a column that is no plain match emits: a ')' it owes to an insertion group before it, the count of matches before it, its own characters.  All
// three follow from the PREVIOUS such column p and the m match columns between: the count is m (+ 1 when p was a crossover on a matching letter, which starts the
// count), the group is open iff p was an insertion, and it stays open only if this column is an insertion with m = 0.  A virtual column behind the last one flushes.
// Carry: m and p's kind.
// Bytes.  Per-lane byte counts are scanned across the wave, the step's bytes are laid down in LDS and stored by all lanes, consecutive bytes by consecutive lanes; the
// byte cursor is carried.  A reversed item (printed on the reverse strand) puts every token at the mirrored place of the item's slice instead.
#include "gm_common.h"
#include "gm_internal.h"

namespace {

__device__ __forceinline__ int ls_char(int code) {             // base_translate, ref: common/fasta.c:689-690
  constexpr uint64_t lo = pack8("ACGTUMRW"), hi = pack8("SYKVHDBN");
  return (int)(((code & 8) ? hi : lo) >> (8 * (code & 7))) & 0xff;
}
__device__ __forceinline__ int nib(const uint32_t* __restrict__ b, long long i) { return (int)((b[i >> 3] >> ((i & 7) * 4)) & 0xf); }
__device__ __forceinline__ void put_num(uint8_t* at, uint32_t v, int nd) { for (int k = nd - 1; k >= 0; k--) { at[k] = (uint8_t)('0' + v % 10u); v /= 10u; } }
__device__ __forceinline__ int top_bit(unsigned long long m) { return 63 - __clzll((long long)m); }      // m != 0
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int* total) {
  int x = v;
  for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(x, d); if (lane >= d) x += y; }
  *total = __shfl(x, 63);
  return x - v;
}
__device__ __forceinline__ bool is_lower(int c) { return c >= 'a' && c <= 'z'; }
__device__ __forceinline__ int to_upper(int c) { return is_lower(c) ? c - 32 : c; }
// what reverse_alignment_edit_string does to a character that is no digit
__device__ __forceinline__ int rev_char(int c) { return c == ')' ? '(' : c == '(' ? ')' : c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// X and the N flag of the r-th read position of a stretch of `cnt` (<= 64) positions, lane r holding colour `base` of it (lanes >= cnt: anything); *cx / *cn: the
// carry in front of the stretch, replaced by the carry behind it.  Returns X | N << 2 | (colour 15) << 3; wave-uniform control flow.
__device__ __forceinline__ int cs_stretch(int base, int cnt, int lane, int* cx, int* cn) {
  const bool in = lane < cnt;
  const unsigned long long reset = __ballot(in && base == 15), poison = __ballot(in && base > 3 && base != 15),
                           b0 = __ballot(in && base <= 3 && (base & 1)), b1 = __ballot(in && base <= 3 && (base & 2));
  auto at = [&](int r) {                                      // the state behind position r of the stretch (0 <= r < 64)
    const unsigned long long upto = (2ull << r) - 1ull, rs = reset & upto;
    const unsigned long long seg = rs ? upto & ~((2ull << top_bit(rs)) - 1ull) : upto;      // the positions behind the last reset
    int x = (__popcll(b0 & seg) & 1) | ((__popcll(b1 & seg) & 1) << 1); int n = (poison & seg) != 0;
    if (!rs) { x ^= *cx; n |= *cn; }
    return x | (n << 2);
  };
  const int mine = at(lane) | ((base == 15) << 3);
  if (cnt > 0) { const int last = at(cnt - 1); *cx = last & 3; *cn = (last >> 2) & 1; }
  return mine;
}

}  // namespace

template <bool IX>
__global__ void __launch_bounds__(64)
k_sw_text(const GmTextItem* __restrict__ items, int n_items, int colour, int what, int write, const uint8_t* __restrict__ ops, const uint32_t* __restrict__ genome,
          const uint32_t* __restrict__ reads, int read_words, int is_rna, const uint8_t* __restrict__ qin, int clip_char, uint32_t* __restrict__ lens,
          const unsigned long long* __restrict__ offs, uint8_t* __restrict__ db_out, uint8_t* __restrict__ qr_out, uint8_t* __restrict__ cig_out, uint8_t* __restrict__ edit_out) {
  __shared__ uint8_t cig_stage[64 * 11];                       // a step's bytes: at most ten digits and the operation a column
  __shared__ uint8_t edit_stage[64 * 14];                      // ... ')', ten digits, 'x', '(' and a letter
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const bool want_al = (what & 1) != 0, want_cig = (what & 2) != 0, want_ed = (what & 4) != 0, strings = want_ed || (want_al && write);
  for (int w = blockIdx.x; w < n_items; w += gridDim.x) {
    const GmTextItem it = items[w];
    const int n = (int)it.n_ops;
    const uint8_t* o = ops + it.ops_off;
    const bool rev = (it.flags & 4) != 0;
    const uint32_t cig_len = write ? lens[2 * w] : 0u, edit_len = write ? lens[2 * w + 1] : 0u;
    uint8_t* cig = write && want_cig ? cig_out + offs[2 * w] : nullptr;
    uint8_t* edit = write && want_ed ? edit_out + offs[2 * w + 1] : nullptr;
    const uint32_t* rw = reads ? reads + (size_t)it.idx * read_words : nullptr;
    auto is_qgap = [&](int b) { return colour ? (b & 15) == 1 : b == 'I'; };
    auto is_dgap = [&](int b) { return colour ? ((b & 15) >= 2 && (b & 15) <= 5) : b == 'D'; };
    // ---- carries ----
    uint32_t cig_cur = 0, edit_cur = 0;                        // byte cursors
    int run_ct = 3, run_len = 0;                               // the open CIGAR run (3: none)
    int ed_m = 0, ed_ins = 0, ed_x = 0;                        // match columns since the last column that was none, and that column's kind
    long long pj0 = it.genome_start; int pi0 = it.read_start;
    int cx = 0, cn = 0;                                        // colour space: X and the N flag in front of read position pi0
    const bool translate = strings && colour && !qin;
    if (translate)
      for (int j0 = 0; j0 < it.read_start; j0 += 64) {
        const int cnt = min(64, it.read_start - j0);
        (void)cs_stretch(lane < cnt ? nib(rw, j0 + lane) : 0, cnt, lane, &cx, &cn);
      }
    if (want_cig && it.read_start > 0) {                       // the leading clip
      const int nd = ndig((uint32_t)it.read_start);
      if (cig && lane == 0) { uint8_t* at = cig + (rev ? cig_len - (uint32_t)(nd + 1) : 0u); put_num(at, (uint32_t)it.read_start, nd); at[nd] = (uint8_t)clip_char; }
      cig_cur = (uint32_t)(nd + 1);
    }
    for (int c0 = 0; c0 <= n; c0 += 64) {                      // (column n: the edit string's flush)
      const int t = c0 + lane; const bool in = t < n;
      const int b = in ? (int)o[t] : 0;
      const bool qgap = in && is_qgap(b), dgap = in && is_dgap(b);
      const int n_in = min(64, n - c0);                        // columns of this step (0: only the flush)
      // ---- CIGAR ----
      if (want_cig && n_in > 0) {
        const int ct = !in ? 3 : qgap ? 2 : dgap ? 1 : 0;      // M I D
        int ctn = 3; if (t + 1 < n) { const int bn = (int)o[t + 1]; ctn = is_qgap(bn) ? 2 : is_dgap(bn) ? 1 : 0; }
        int prev = __shfl_up(ct, 1); if (lane == 0) prev = run_ct;
        const unsigned long long starts = __ballot(in && ct != prev), mine = starts & ((below << 1) | 1ull);
        const int len = mine ? lane - top_bit(mine) + 1 : run_len + lane + 1;
        const bool last = in && ct != ctn;
        const int nd = ndig((uint32_t)len), nb = last ? nd + 1 : 0;
        int total; const int off = wave_excl_scan(nb, lane, &total);
        if (cig) {
          if (last) { uint8_t* at = cig_stage + (rev ? total - off - nb : off); put_num(at, (uint32_t)len, nd); at[nd] = (uint8_t)(ct == 0 ? 'M' : ct == 1 ? 'I' : 'D'); }
          __syncthreads();
          uint8_t* out = cig + (rev ? cig_len - cig_cur - (uint32_t)total : cig_cur);
          for (int k = lane; k < total; k += 64) out[k] = cig_stage[k];
          __syncthreads();
        }
        cig_cur += (uint32_t)total;
        run_ct = __shfl(ct, n_in - 1); run_len = __shfl(len, n_in - 1);
      }
      if (!strings) continue;
      // ---- the column's two characters ----
      const bool rcol = in && !qgap, gcol = in && !dgap;
      const unsigned long long rmask = __ballot(rcol), gmask = __ballot(gcol);
      const int pi = pi0 + __popcll(rmask & below); const long long pj = pj0 + __popcll(gmask & below);
      int d = '-', q = '-';
      if (gcol) {
        const bool rcs = IX && (it.flags & 1);                 // (strand 1 of a contig: the complement of the forward letter, see GmPostItem)
        const long long gp = !IX ? pj : (rcs ? it.gbase - pj : it.gbase + pj);
        int code = nib(genome, gp);
        if (rcs) code = (int)((gm_cmpl_tab((it.flags & 2) != 0) >> (code * 4)) & 0xf);
        d = ls_char(code);
      }
      if (qin) q = in ? (int)qin[it.ops_off + t] : 0;
      else if (!colour) { if (rcol) q = ls_char(nib(rw, pi)); }
      else {
        const int cnt = __popcll(rmask);
        const int st = cs_stretch(lane < cnt ? nib(rw, pi0 + lane) : 0, cnt, lane, &cx, &cn);
        const int mine = __shfl(st, __popcll(rmask & below));
        if (rcol) {
          const int type = b & 15, lay = dgap ? type - 2 : type - 6;
          int code = ((lay + it.initbp) & 3) ^ (mine & 3); if (is_rna && code == 3) code = 4;
          if (mine & 12) code = 15;
          const int lower = (b & 0x80) ? 0x20 : 0;
          q = (code == 15 && !dgap) ? (d | lower) : (ls_char(code) | lower);      // an unknown read letter shows the genome's
        }
      }
      pi0 += __popcll(rmask); pj0 += __popcll(gmask);
      if (write && want_al && in) { db_out[it.ops_off + t] = (uint8_t)d; qr_out[it.ops_off + t] = (uint8_t)q; }
      if (!want_ed) continue;
      // ---- edit string ----
      const bool act = t <= n;
      const bool non_m = act && !(in && d == q && d != '-');
      const bool ins = in && d == '-';
      const bool xm = in && non_m && !ins && q != '-' && d == to_upper(q);
      const unsigned long long nm_mask = __ballot(non_m), ins_mask = __ballot(ins), x_mask = __ballot(xm);
      int nb = 0, m = 0, p_ins = 0, p_x = 0;
      if (non_m) {
        const unsigned long long before = nm_mask & below;
        if (before) { const int p = top_bit(before); m = lane - p - 1; p_ins = (int)((ins_mask >> p) & 1); p_x = (int)((x_mask >> p) & 1); }
        else { m = ed_m + lane; p_ins = ed_ins; p_x = ed_x; }
      }
      const uint32_t consec = (uint32_t)(m + p_x);
      const bool close = non_m && p_ins && (m != 0 || !ins), open = ins && !(p_ins && m == 0), low = in && is_lower(q);
      const int nd = consec ? ndig(consec) : 0;
      if (non_m) nb = (close ? 1 : 0) + nd + (!in ? 0 : ins ? (low ? 1 : 0) + (open ? 1 : 0) + 1 : (q == '-' || xm) ? 1 : low ? 2 : 1);
      int total; const int off = wave_excl_scan(nb, lane, &total);
      if (edit) {
        if (non_m) {
          int at = off;
          auto put = [&](int c) { if (rev) edit_stage[total - 1 - at] = (uint8_t)rev_char(c); else edit_stage[at] = (uint8_t)c; at++; };
          if (close) put(')');
          if (nd) { put_num(edit_stage + (rev ? total - at - nd : at), consec, nd); at += nd; }
          if (in) {
            if (ins) { if (low) put('x'); if (open) put('('); put(to_upper(q)); }
            else if (q == '-') put('-');
            else if (xm) put('x');
            else if (low) { put('x'); put(to_upper(q)); }
            else put(q);
          }
        }
        __syncthreads();
        uint8_t* out = edit + (rev ? edit_len - edit_cur - (uint32_t)total : edit_cur);
        for (int k = lane; k < total; k += 64) out[k] = edit_stage[k];
        __syncthreads();
      }
      edit_cur += (uint32_t)total;
      if (nm_mask) { const int p = top_bit(nm_mask); ed_m = 63 - p; ed_ins = (int)((ins_mask >> p) & 1); ed_x = (int)((x_mask >> p) & 1); }
      else ed_m += 64;
    }
    if (want_cig && it.tail > 0) {                             // the trailing clip
      const int nd = ndig((uint32_t)it.tail);
      if (cig && lane == 0) { uint8_t* at = cig + (rev ? cig_len - cig_cur - (uint32_t)(nd + 1) : cig_cur); put_num(at, (uint32_t)it.tail, nd); at[nd] = (uint8_t)clip_char; }
      cig_cur += (uint32_t)(nd + 1);
    }
    if (!write && lane == 0) { lens[2 * w] = cig_cur; lens[2 * w + 1] = edit_cur; }
  }
}

int gm_launch_sw_text(int n_items, const GmTextItem* d_items, int colour, int what, int write, const uint8_t* d_ops, const uint32_t* d_genome, const uint32_t* d_reads,
                      int read_words, int is_rna, const uint8_t* d_qin, int clip_char, uint32_t* d_lens, const unsigned long long* d_offs, uint8_t* d_db, uint8_t* d_qr,
                      uint8_t* d_cigar, uint8_t* d_edit, hipStream_t stream, int ix) {
  if (n_items < 1) return GM_E_ARG;
  const int grid = n_items < GM_TEXT_MAX_GRID ? n_items : GM_TEXT_MAX_GRID;
  if (ix) hipLaunchKernelGGL(k_sw_text<true>, dim3(grid), dim3(64), 0, stream, d_items, n_items, colour, what, write, d_ops, d_genome, d_reads, read_words, is_rna, d_qin, clip_char,
                             d_lens, d_offs, d_db, d_qr, d_cigar, d_edit);
  else hipLaunchKernelGGL(k_sw_text<false>, dim3(grid), dim3(64), 0, stream, d_items, n_items, colour, what, write, d_ops, d_genome, d_reads, read_words, is_rna, d_qin, clip_char,
                          d_lens, d_offs, d_db, d_qr, d_cigar, d_edit);
  if (hipGetLastError() != hipSuccess) return GM_E_NODEVICE;
  return GM_OK;
}
