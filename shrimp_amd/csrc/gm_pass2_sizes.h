// LDS sizes of the pass-2 kernels and what follows from them, on plain numbers (a header without HIP: the launchers of gm_sw.hip, the admission tests of the host entries
// and tests/host/pass2_sizes_main.cpp share it).
#pragma once
#include <cstddef>
#include <cstdint>

static const size_t GM_SWF_LDS_LIMIT = 160 * 1024;      // LDS of a CU: what one wave of the batch kernels may take; the admission test of the host entries and the launchers share it

// LDS of the letter-space pass-2 kernels of NG windows a wave (k_pass2_g4: NG = 4 with int carry rows, 8 with int16_t ones): reads, windows, three carry values a column
inline size_t gm_pass2_g4_lds(int ng, int read_len, int window_len) {
  const size_t r16 = (size_t)((read_len + 15) & ~15), w16 = (size_t)((window_len + 15) & ~15);
  return ng * r16 + ng * w16 + ng * (size_t)window_len * 3 * (ng == 8 ? sizeof(int16_t) : sizeof(int)) + 64;
}

// LDS of the colour-space pass-2 kernels: one window a wave (ng = 1, k_pass2_cs), or NG (k_pass2_cs_g4: 4 with int carry rows, 8 with int16_t ones) -- the colours and the
// four translations of a read, the window, twelve carry values a column
inline size_t gm_pass2_cs_lds(int ng, int read_len, int window_len) {
  const size_t q16 = (size_t)((read_len + 15) & ~15), w16 = (size_t)((window_len + 15) & ~15);
  return ng * 5 * q16 + ng * w16 + ng * (size_t)window_len * 12 * (ng == 8 ? sizeof(int16_t) : sizeof(int)) + 64;
}

// The longest window pass 2 takes beside reads of read_len: what the kernel gm_launch_pass2 / gm_launch_pass2_cs choose fits into GM_SWF_LDS_LIMIT, and no more than the
// 16 bits of GmHit.w_len.  gm_map_reads / gm_map_pairs refuse a longer window (GM_E_RANGE) before they upload anything.
// (by the launchers' own size functions.  Letter space: the four-window kernel, which every mapping call gets; colour space: the one-window kernel, which global alignment
// falls back to when the four-window one does not fit, and the four-window one with int carry rows, which local alignment needs -- the eight-window shape, taken only
// within 64 KB, fits wherever that one does)
inline int gm_pass2_max_window(int colour, int local, int read_len) {
  auto lds = [&](int W) -> size_t { return !colour ? gm_pass2_g4_lds(4, read_len, W) : gm_pass2_cs_lds(local ? 4 : 1, read_len, W); };
  int lo = 0, hi = 65535;
  while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (lds(mid) <= GM_SWF_LDS_LIMIT) lo = mid; else hi = mid - 1; }
  return lo;
}

// K1b's list-mode kernel (k_prune, gm_launch_prune) beside a survivor capacity of scap whose survivors come in `segs` segments (the index's slabs; 1: unsegmented): a
// table of 2^hbits slots of 8 bytes for twice a segment's share of the capacity.  The launcher and the admission test of the mapping calls both ask here.
inline int gm_prune_hbits(int scap, int segs) {
  if (segs < 1) segs = 1;
  const int share = segs > 1 ? (2 * scap) / segs : scap;
  int hbits = 8; while ((1 << hbits) < 2 * (share > 128 ? share : 128)) hbits++;
  return hbits;
}
inline size_t gm_prune_lds(int scap, int segs) { return (size_t)8 << gm_prune_hbits(scap, segs); }
