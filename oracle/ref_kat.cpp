// ref_kat.cpp -- known-answer generator for the reference's own sw_vector() / sw_full_ls().
// TEST INFRASTRUCTURE ONLY.  Compiled (by oracle/Makefile.ref, only where /root/reference
// exists) against the reference headers where they lie and linked with oracle/_ref/libref_sw.so.
// Writes text records consumed by tools/make_golden.py -> tests/golden/sw_kat.txt.gz
//   V goff glen rlen <genome words hex,...> <read words hex,...> score
//   F goff glen rlen ax ay alen awidth revcmpl <genome words> <read words> score read_start rmapped genome_start gmapped matches mismatches insertions deletions dbalign qralign
//   L ...  (second argument "local"): sw_full_ls with local_alignment = 1 -> tests/golden/sw_kat_local.txt.gz
// Second argument "scores": the same cases under five other score sets -> tests/golden/sw_kat_scores.txt.gz.  Each set opens with
//   P name dblen qrlen a_open a_ext b_open b_ext match mismatch          (the setups' arguments)
// and is followed by the V, F and L records of n cases (L: threshold rlen * match / 2, with and without the anchor box); the set "large" ends with a dozen V
// records at read lengths 129, 256, 257 and 1000 (more than one stripe of the vector filter), half of them on windows of at most 256 columns.
// Second argument "anchors": default scores under the anchor widths -1 (the threshold band whatever the box), 0, 1, 9 and 99 -> tests/golden/sw_kat_anchors.txt.gz.  Each
// width opens with
//   P w<width> dblen qrlen a_open a_ext b_open b_ext match mismatch anchor_width
// and holds the same n cases (the generator is re-seeded): F records (global, threshold 0), G records (global at the threshold rlen * match / 2, which the band of width
// -1 depends on; the L records' fields) and L records (local, with the box and without).  Beside the boxes of the other modes: boxes that leave the matrix on the left
// (x < 0), on the right (x + length > glen) and at the bottom (y + length > rlen), boxes up to 12 wide, and boxes on windows shorter than the read.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>
#include <random>
#include "common/sw-vector.h"
#include "common/sw-full-common.h"
#include "common/sw-full-ls.h"
#include "common/anchors.h"

static void put(std::vector<uint32_t>& bf, int i, int v) { bf[i / 8] |= (uint32_t)(v & 0xf) << (4 * (i % 8)); }
static void dump(const std::vector<uint32_t>& bf) { for (size_t i = 0; i < bf.size(); i++) printf("%s%x", i ? "," : "", bf[i]); }

struct ScoreSet { const char* name; int match, mismatch, a_go, a_ge, b_go, b_ge; };
static const ScoreSet DEFAULT_SET = {"default", 10, -15, -33, -7, -33, -3};
static const ScoreSet SCORE_SETS[] = {
  {"unit",    1,  -1,   -1,  -1,  -1,  -1},     // smallest values, maximal ties
  {"linear", 10, -15,    0, -12,   0,  -9},     // open 0: the affine recurrences degenerate
  {"swapped", 10, -15, -20,  -2, -45,  -9},     // a much cheaper than b
  {"steep",   7, -40,  -60,  -1, -25, -30},     // extend > open on one side, mismatch dearer than a short gap
  {"large",  32, -60, -100, -20, -90, -25},     // int16 headroom: 32 * 1000 = 32000
};

int main(int argc, char** argv) {
  int n = argc > 1 ? atoi(argv[1]) : 2000;
  const bool local_mode = argc > 2 && !strcmp(argv[2], "local");   // "L" records: sw_full_ls with local_alignment = 1, with and without an anchor
  const bool score_mode = argc > 2 && !strcmp(argv[2], "scores"); // "P" lines, and V, F and L records under each of SCORE_SETS
  const bool anchor_mode = argc > 2 && !strcmp(argv[2], "anchors"); // "P" lines, and F, G and L records under each of ANCHOR_WIDTHS
  static const int ANCHOR_WIDTHS[] = {-1, 0, 1, 9, 99};
  std::mt19937_64 rng(20260101);
  const int n_sets = score_mode ? (int)(sizeof SCORE_SETS / sizeof SCORE_SETS[0]) : anchor_mode ? (int)(sizeof ANCHOR_WIDTHS / sizeof ANCHOR_WIDTHS[0]) : 1;
  for (int si = 0; si < n_sets; si++) {
  const ScoreSet& S = score_mode ? SCORE_SETS[si] : DEFAULT_SET;
  const int width = anchor_mode ? ANCHOR_WIDTHS[si] : 8;
  if (anchor_mode) rng.seed(20260101);                // the same cases under every width
  sw_vector_setup(1400, 1000, S.a_go, S.a_ge, S.b_go, S.b_ge, S.match, S.mismatch, 0, true);
  sw_full_ls_setup(1400, 1000, S.a_go, S.a_ge, S.b_go, S.b_ge, S.match, S.mismatch, true, width);
  if (anchor_mode) printf("P w%d 1400 1000 %d %d %d %d %d %d %d\n", width, S.a_go, S.a_ge, S.b_go, S.b_ge, S.match, S.mismatch, width);
  if (score_mode) printf("P %s 1400 1000 %d %d %d %d %d %d\n", S.name, S.a_go, S.a_ge, S.b_go, S.b_ge, S.match, S.mismatch);
  const int n_long = score_mode && !strcmp(S.name, "large") ? 12 : 0;   // V records only, reads of more than one stripe
  for (int t = 0; t < n + n_long; t++) {
    int rlen = 20 + rng() % 131;                       // 20..150
    int kind = rng() % 8;
    if (anchor_mode && t % 8 == 6) kind = 0;             // a window shorter than the read, together with a box
    int glen = (kind == 0) ? (int)(rlen - rng() % 10)  // window shorter than the read
                           : (int)(rlen * 1.4);
    if (t >= n) {
      static const int long_len[4] = {129, 256, 257, 1000};
      const int k = t - n;
      rlen = long_len[k % 4]; kind = 1 + k / 4;         // exact copies (1000 x 32 = 32000), substitutions, indels
      glen = (k + k / 4) % 2 == 0 ? 160 + (int)(rng() % 97) : (int)(rlen * 1.4) + (rlen < 200 ? 120 : 0);   // 160..256 columns, or beyond 256: each length has both
    }
    if (glen < 8) glen = 8;
    int goff = rng() % 23;
    std::vector<int> g(goff + glen + 9), r(rlen);
    for (auto& b : g) b = rng() % 4;
    // read = mutated copy of a window diagonal, so that scores are meaningful
    int start = goff + (glen > rlen ? rng() % (glen - rlen + 1) : 0);
    int gi = start;
    double psub = (kind == 1) ? 0.0 : (kind == 2 ? 0.15 : 0.03), pind = (kind == 3) ? 0.05 : ((t >= n && kind == 1) ? 0.0 : 0.005);   // (the long exact copies have no indels either)
    for (int i = 0; i < rlen; i++) {
      double u = (rng() % 100000) / 100000.0;
      if (u < pind) { r[i] = rng() % 4; continue; }          // insertion in read
      if (u < 2 * pind) gi += 1 + rng() % 3;                  // deletion from read
      int b = g[gi < (int)g.size() ? gi : (int)g.size() - 1]; gi++;
      if ((rng() % 100000) / 100000.0 < psub) b = (b + 1 + rng() % 3) & 3;
      r[i] = b;
    }
    if (kind == 4) { for (int k = 0; k < 3; k++) { r[rng() % rlen] = 15; g[goff + rng() % glen] = 15; } }   // N codes (N==N matches)
    if (kind == 5) { for (int k = 0; k < 4; k++) g[goff + rng() % glen] = 4 + rng() % 11; }                 // IUPAC codes
    if (kind == 6) { for (auto& b : g) b = 0; for (auto& b : r) b = 0; }                                    // homopolymer: every tie rule fires
    std::vector<uint32_t> gb((goff + glen + 16) / 8 + 1, 0), rb(rlen / 8 + 1, 0);
    for (size_t i = 0; i < g.size(); i++) put(gb, (int)i, g[i]);
    for (int i = 0; i < rlen; i++) put(rb, i, r[i]);
    int sv = sw_vector(gb.data(), goff, glen, rb.data(), rlen, NULL, -1, false);
    if (t >= n) { printf("V %d %d %d ", goff, glen, rlen); dump(gb); printf(" "); dump(rb); printf(" %d\n", sv); continue; }
    if (!local_mode && !anchor_mode) { printf("V %d %d %d ", goff, glen, rlen); dump(gb); printf(" "); dump(rb); printf(" %d\n", sv); }
    // full SW around a plausible anchor box
    struct anchor a; memset(&a, 0, sizeof a);
    a.x = (start - goff) + (int)(rng() % 7) - 3; a.y = 0; a.length = 14 + rng() % (rlen > 20 ? rlen - 14 : 6); a.width = 1 + rng() % 4; a.weight = 2;
    if (rng() % 4 == 0) { a.y = rng() % 10; a.x += a.y; }
    if (anchor_mode) {                                   // boxes the pipeline produces and the other modes lack; d: the diagonal the read was copied from
      const int d = start - goff, half = a.length / 2;
      switch (t % 8) {
        case 2: a.x = -(1 + (int)(rng() % 5)); a.y = 0; a.width = 6 + rng() % 7; break;                                        // x < 0 (wide enough to reach the read's diagonal from a small d)
        case 3: a.y = glen - d - half; if (a.y > rlen - 1) a.y = rlen - 1; if (a.y < 0) a.y = 0; a.x = d + a.y; break;          // x + length > glen
        case 4: a.y = rlen - half; if (a.y < 0) a.y = 0; a.x = d + a.y; break;                                                  // y + length > rlen
        case 5: a.width = (t % 16 == 5) ? 12 : 5 + rng() % 8; break;                                                            // up to 12 wide
        default: break;
      }
    }
    if (!local_mode)
      for (int rv = 0; rv < 2; rv++) {
        struct sw_full_results sfr; memset(&sfr, 0, sizeof sfr);
        sw_full_ls(gb.data(), goff, glen, rb.data(), rlen, 0, sv, &sfr, rv, &a, 1, 0);
        if (sfr.score <= 0) continue;   // reference backtraces from stale scratch in this case; not a defined answer
        printf("F %d %d %d %lld %lld %d %d %d ", goff, glen, rlen, a.x, a.y, a.length, a.width, rv); dump(gb); printf(" "); dump(rb);
        printf(" %d %d %d %d %d %d %d %d %d %s %s\n", sfr.score, sfr.read_start, sfr.rmapped, sfr.genome_start, sfr.gmapped,
               sfr.matches, sfr.mismatches, sfr.insertions, sfr.deletions, sfr.dbalign, sfr.qralign);
        free(sfr.dbalign); free(sfr.qralign);
      }
    if (local_mode || score_mode || anchor_mode) {
      const int thresh = (rlen * S.match) / 2;
      if (sv < thresh) continue;                      // gmapper calls the full SW only then (mapping.c:390)
      if (t % 3 == 0 && !anchor_mode) { a.width = 1; a.length = 12; }  // thin anchors: the best local alignment leaves the band more often (the second run)
      for (int loc = anchor_mode ? 0 : 1; loc < 2; loc++)            // (anchors: G records, global mode at this threshold, before the L records)
      for (int rv = 0; rv < 2; rv++)
        for (int na = 0; na < (loc ? 2 : 1); na++) {  // with the anchor box, and without (threshold band)
          struct sw_full_results sfr; memset(&sfr, 0, sizeof sfr);
          sw_full_ls(gb.data(), goff, glen, rb.data(), rlen, thresh, sv, &sfr, rv, na ? NULL : &a, na ? 0 : 1, loc);
          if (sfr.score <= 0) continue;
          printf(loc ? "L " : "G "); printf("%d %d %d %lld %lld %d %d %d %d %d %d ", goff, glen, rlen, a.x, a.y, a.length, a.width, rv, na, thresh, sv); dump(gb); printf(" "); dump(rb);
          printf(" %d %d %d %d %d %d %d %d %d %s %s\n", sfr.score, sfr.read_start, sfr.rmapped, sfr.genome_start, sfr.gmapped,
                 sfr.matches, sfr.mismatches, sfr.insertions, sfr.deletions, sfr.dbalign, sfr.qralign);
          free(sfr.dbalign); free(sfr.qralign);
        }
    }
  }
  }
  return 0;
}
