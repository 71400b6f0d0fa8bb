// gm_sam.hip -- the SAM text of a chunk's mappings, made on the device (gm_sam_records, gm_host_sam.inc): what hit_output prints for an unpaired read (ref:
// gmapper/output.c:227-774), from the arrays of the batch seams.
//
//   k_sam_records   one wave per output record (a block is one wave), grid-stride over the records; a record is a mapping, or the unaligned record of a read.
//
// The host has checked every record against the caller's buffers (gm_host_sam.inc): the read, the name, the contig, and the CIGAR / edit / qralign / base-quality
// slices all lie inside what was uploaded, and every integer a record prints stands in its GmSamRec.  The kernel runs twice: the sizing launch (write = 0) leaves the
// length of every record in lens[], k_win_scan turns them into 64-bit offsets, the writing launch stores every byte.  Both launches run the same code, so the sizes
// cannot disagree with the bytes.
//
// A record is a sequence of segments behind a wave-uniform byte cursor.  Every segment is stored by all lanes, consecutive bytes by consecutive lanes:
//   literal     at most 17 bytes, lane k its k-th.
//   number      the digit count fixes the length; lane k stores digit k.
//   slice       bytes of a global buffer (name, contig name, CIGAR, XX:Z, ZE:Z, CQ:Z, the file's own colour read), as they are, or mirrored with an offset added
//               (QUAL re-based to PHRED + 33 and turned with the read).
//   packed      letters of a 4-bit bitfield (SEQ of a letter-space read, the colours of CS:Z): a lane takes one WORD, eight positions, and lays its eight characters
//               down in LDS -- at the mirrored place and complemented for strand 1 -- 512 positions a step; the step is then stored from LDS.  Neither direction
//               reads a byte a lane from global memory.  A clipped position of a read that came as text keeps the file's letter (seq_from_text, ref: output.c:326-351).
//   colour SEQ  the non-gap characters of the qralign slice: a ballot of the non-gap columns of a 64-column step and a popcount give each letter its place, the
//               count of the steps before is carried; strand 1 stores the complement at the mirrored place (the total comes from a counting pass over the slice).
// No atomics, no doubles: Z0 / Z1 come as integers from the host's log.
#include "gm_common.h"
#include "gm_internal.h"

namespace {

__device__ __forceinline__ int all_char(int code) {            // base_translate, ref: common/fasta.c:689-690
  constexpr uint64_t lo = pack8("ACGTUMRW"), hi = pack8("SYKVHDBN");
  return (int)(((code & 8) ? hi : lo) >> (8 * (code & 7))) & 0xff;
}
__device__ __forceinline__ int seq_char(int code) { return code < 4 ? (int)((0x54474341u >> (8 * code)) & 0xffu) : 'N'; }      // an aligned read base: non-ACGT -> N (ref: output.c:485-533)
__device__ __forceinline__ int rc_char(int c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }
__device__ __forceinline__ int seq_from_text(int c) {          // ref: gmapper/output.c:326-351
  switch (c) { case 'R': case 'Y': case 'S': case 'W': case 'K': case 'M': case 'B': case 'D': case 'H': case 'V': return 'N'; default: return c >= 'a' ? c - 32 : c; }
}
__device__ __forceinline__ int cs_seq_char(int c) { if (c >= 'a') c -= 32; return (c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N') ? c : 'N'; }

enum { PK_SEQ = 0, PK_COLOURS = 1, PK_LETTERS = 2 };

}  // namespace

__global__ void __launch_bounds__(64)
k_sam_records(const GmSamArgs A, int write) {
  __shared__ uint8_t stage[512];
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int L = A.read_len;
  for (int w = blockIdx.x; w < A.n_recs; w += gridDim.x) {
    const GmSamRec R = A.recs[w];
    uint8_t* o = write ? A.out + A.offs[w] : nullptr;
    uint32_t cur = 0;
    auto lit = [&](const char* s, int n) { if (o && lane < n) o[cur + lane] = (uint8_t)s[lane]; cur += (uint32_t)n; };
    auto num_u = [&](uint32_t v) {
      const int nd = ndig(v);
      if (o && lane < nd) { uint32_t p = 1; for (int k = nd - 1 - lane; k > 0; k--) p *= 10u; o[cur + lane] = (uint8_t)('0' + (v / p) % 10u); }
      cur += (uint32_t)nd;
    };
    auto num_i = [&](int v) { if (v < 0) { lit("-", 1); num_u((uint32_t)(-(long long)v)); } else num_u((uint32_t)v); };
    auto slice = [&](const uint8_t* src, uint32_t n) { if (o) for (uint32_t k = lane; k < n; k += 64) o[cur + k] = src[k]; cur += n; };
    auto slice_turned = [&](const uint8_t* src, uint32_t n, bool rev, int add) {
      if (o) for (uint32_t k = lane; k < n; k += 64) o[cur + k] = (uint8_t)(src[rev ? n - 1 - k : k] + add);
      cur += n;
    };
    // n positions of a bitfield; text: the read's line in the file, used at positions outside [keep_lo, keep_hi)
    auto packed = [&](const uint32_t* rw, int n, int mode, bool rev, const uint8_t* text, int keep_lo, int keep_hi) {
      if (o) for (int s0 = 0; s0 < n; s0 += 512) {
        const int cnt = min(512, n - s0), i0 = s0 + 8 * lane;
        if (i0 < n) {
          uint32_t x = rw[i0 >> 3];
          for (int k = 0; k < 8 && i0 + k < n; k++, x >>= 4) {
            const int i = i0 + k, code = (int)(x & 15u);
            int ch;
            if (mode == PK_COLOURS) ch = code < 4 ? '0' + code : '.';
            else if (text && (i < keep_lo || i >= keep_hi)) ch = seq_from_text((int)text[i]);
            else ch = mode == PK_LETTERS ? all_char(code) : seq_char(code);
            if (rev) ch = ch == '.' ? '.' : rc_char(ch);
            const int t = i - s0;
            stage[rev ? cnt - 1 - t : t] = (uint8_t)ch;
          }
        }
        __syncthreads();
        uint8_t* dst = o + cur + (rev ? n - s0 - cnt : s0);
        for (int k = lane; k < cnt; k += 64) dst[k] = stage[k];
        __syncthreads();
      }
      cur += (uint32_t)n;
    };
    const int rd = R.read;
    const uint32_t* rw = A.reads + (size_t)rd * A.read_words;
    const uint8_t* qline = A.quals ? A.quals + (size_t)rd * ((size_t)L + 1) : nullptr;
    const uint8_t* sline = A.seqs ? A.seqs + (size_t)rd * ((size_t)L + (A.colour ? 2 : 1)) : nullptr;
    auto csfasta = [&]() {                                     // the read as csfasta text (CS:Z, ref: output.c:451,730)
      if (sline) { slice(sline, (uint32_t)L + 1u); return; }
      if (o && lane == 0) o[cur] = (uint8_t)seq_char(A.initbp[rd] & 3);
      cur += 1;
      packed(rw, L, PK_COLOURS, false, nullptr, 0, 0);
    };
    auto tail = [&](bool extra) {                              // ref: output.c:452-465,729-761
      if (A.rg_len) { lit("\tRG:Z:", 6); slice(A.cnames + A.cname_off[A.n_contigs], (uint32_t)A.rg_len); }
      if (extra) {
        lit("\tZM:i:", 6); num_i(R.zm); lit("\tZR:i:", 6); num_i(R.zr); lit("\tZV:i:", 6); num_i(R.zv); lit("\tZH:i:", 6); num_i(R.zh);
        lit("\tZE:Z:", 6); slice(A.edit + R.edit_off, R.edit_len);
      }
      lit("\n", 1);
    };
    // QNAME
    if (A.names) slice(A.names + A.name_off[rd], (uint32_t)(A.name_off[rd + 1] - A.name_off[rd] - 1ull));
    else { lit("r", 1); num_u((uint32_t)rd); }
    if (R.cn < 0) {                                            // the unaligned record, ref: output.c:411-466
      lit("\t4\t*\t0\t0\t*\t*\t0\t0\t", 17);
      if (A.colour) {
        lit("*\t*\tCQ:Z:", 9);
        if (qline) slice(qline, (uint32_t)L); else lit("*", 1);
        lit("\tCS:Z:", 6); csfasta();
      } else {
        packed(rw, L, PK_LETTERS, false, sline, L, L);
        if (qline) { lit("\t", 1); slice(qline, (uint32_t)L); } else lit("\t*", 2);
      }
      tail(false);
    } else {
      const bool rev = (R.flags & 1) != 0;
      if (rev) lit("\t16\t", 4); else lit("\t0\t", 3);
      slice(A.cnames + A.cname_off[R.cn], A.cname_off[R.cn + 1] - A.cname_off[R.cn]);
      lit("\t", 1); num_u(R.pos); lit("\t", 1); num_i(R.mqv); lit("\t", 1);
      slice(A.cigar + R.cigar_off, R.cigar_len);
      lit("\t*\t0\t0\t", 7);
      if (A.colour) {                                          // SEQ = the aligned letters post_sw called (ref: output.c:485-537)
        const uint8_t* q = A.qralign + R.qr_off; const int n = (int)R.qr_len;
        int nq = 0;
        for (int c0 = 0; c0 < n; c0 += 64) { const int t = c0 + lane; nq += __popcll(__ballot(t < n && q[t] != '-')); }
        if (o) {
          int carry = 0;
          for (int c0 = 0; c0 < n; c0 += 64) {
            const int t = c0 + lane; const int c = t < n ? (int)q[t] : '-';
            const bool ng = c != '-';
            const unsigned long long m = __ballot(ng);
            if (ng) { const int rank = carry + __popcll(m & below), ch = cs_seq_char(c); if (rev) o[cur + (uint32_t)(nq - 1 - rank)] = (uint8_t)rc_char(ch); else o[cur + (uint32_t)rank] = (uint8_t)ch; }
            carry += __popcll(m);
          }
        }
        cur += (uint32_t)nq;
        lit("\t", 1);
        if (R.pq_len) slice_turned(A.post_quals + R.pq_off, R.pq_len, rev, 0); else lit("*", 1);      // post_sw's base qualities, ref: output.c:613-621
      } else {
        packed(rw, L, PK_SEQ, rev, sline, R.keep_lo, R.keep_hi);
        if (qline) { lit("\t", 1); slice_turned(qline, (uint32_t)L, rev, A.dq); } else lit("\t*", 2);      // ref: output.c:539-570
      }
      lit("\tAS:i:", 6); num_i(R.as);
      if (A.ztags) { lit("\tZ0:i:", 6); num_i(R.z0); lit("\tZ1:i:", 6); num_i(R.z1); }                       // ref: output.c:691-696
      lit("\tNM:i:", 6); num_i(R.nm);
      if (A.colour) {                                          // ref: output.c:717-730
        if (qline) { lit("\tCQ:Z:", 6); slice(qline, (uint32_t)L); }
        lit("\tCS:Z:", 6); csfasta();
        lit("\tCM:i:", 6); num_i(R.cm);
        lit("\tXX:Z:", 6); slice(A.qralign + R.qr_off, R.qr_len);
      }
      tail(A.extra != 0);
    }
    if (!write && lane == 0) A.lens[w] = cur;
  }
}

int gm_launch_sam_records(const GmSamArgs& args, int write, hipStream_t stream) {
  if (args.n_recs < 1) return GM_E_ARG;
  const int grid = args.n_recs < GM_TEXT_MAX_GRID ? args.n_recs : GM_TEXT_MAX_GRID;
  hipLaunchKernelGGL(k_sam_records, dim3(grid), dim3(64), 0, stream, args, write);
  if (hipGetLastError() != hipSuccess) return GM_E_NODEVICE;
  return GM_OK;
}
