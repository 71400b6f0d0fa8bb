// ref_kat_cs.cpp -- known-answer generator for the reference's own colour-space kernels: sw_vector() with use_colours
// and sw_full_cs().  TEST INFRASTRUCTURE ONLY.  Compiled (by oracle/Makefile.ref, only where /root/reference exists)
// against the reference headers where they lie and linked with oracle/_ref/libref_sw.so.
// Records (consumed by tools/make_golden.py -> tests/golden/sw_kat_cs.txt.gz); bitfields are hex words, comma separated:
//   C goff glen rlen initbp <genome_cs words> <genome_ls words> <read colour words> score
//   S goff glen rlen initbp ax ay alen awidth revcmpl thresh <genome_ls words> <read colour words>
//     score read_start rmapped genome_start gmapped matches mismatches insertions deletions crossovers dbalign qralign   ("-" when empty)
//   L ...  (second argument "local"): the S record's fields for sw_full_cs in local mode -> tests/golden/sw_kat_cs_local.txt.gz
//   X / Y ...  (second argument "xover"): sw_full_cs with a per-position crossover_score[] (what every csfastq read hands it, ref: mapping.c:375-379, gmapper.c:532-544),
//     global (X) and local (Y) mode; the S record's fields with the rlen scores (comma separated, in [2 * global, -1] as gmapper.c:538-542 clamps them) behind the read words
//     -> tests/golden/sw_kat_cs_xover.txt.gz
//   C / S / L with second argument "rna": the genome holds U for every T (an RNA contig) and both functions get is_rna = true (what gmapper passes for a genome whose last
//     contig is RNA, ref: genome.c:1063-1064, mapping.c:375-388,1318-1327) -- lstocs reads U as T, cstols hands back U for T (util.h:157-205); global and local mode
//     -> tests/golden/sw_kat_cs_rna.txt.gz
// Second argument "scores": the same cases under six other score sets -> tests/golden/sw_kat_cs_scores.txt.gz.  Each set opens with
//   P name dblen qrlen a_open a_ext b_open b_ext match mismatch crossover indel_taboo_len      (sw_full_cs_setup's arguments; the vector filter's mismatch is match + crossover)
// and is followed by the C, S (both strands), L, X and Y (one strand each, Y on every other case) records of n cases, thresholds scaled by the set's match score
// and the per-position crossover scores drawn in [2 * crossover, -1].
// Second argument "anchors": default scores under the anchor widths -1 (the threshold band whatever the box), 0, 1, 9 and 99 -> tests/golden/sw_kat_cs_anchors.txt.gz.
// Each width opens with
//   P w<width> dblen qrlen a_open a_ext b_open b_ext match mismatch crossover indel_taboo_len anchor_width
// and holds the S and L records (both strands) of the same n cases (the generator is re-seeded), with the boxes of oracle/ref_kat.cpp's mode "anchors": boxes that leave
// the matrix on the left, on the right and at the bottom, boxes up to 12 wide, boxes on windows shorter than the read.
// Otherwise scores are the binary's colour-space defaults (ref: gmapper-defaults.h:52-58): match 10, mismatch -24, crossover -20,
// gaps -33/-7 (reference) -33/-3 (query); the vector filter's mismatch is match + crossover (ref: gmapper.c:2935).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>
#include <random>
#include "common/util.h"
#include "common/sw-vector.h"
#include "common/sw-full-common.h"
#include "common/sw-full-cs.h"
#include "common/anchors.h"

static void put(std::vector<uint32_t>& bf, int i, int v) { bf[i / 8] |= (uint32_t)(v & 0xf) << (4 * (i % 8)); }
static void dump(const std::vector<uint32_t>& bf) { for (size_t i = 0; i < bf.size(); i++) printf("%s%x", i ? "," : "", bf[i]); }

struct ScoreSet { const char* name; int match, mismatch, xover, a_go, a_ge, b_go, b_ge, taboo; };
static const ScoreSet DEFAULT_SET = {"default", 10, -24, -20, -33, -7, -33, -3, 0};
static const ScoreSet SCORE_SETS[] = {      // the letter-space sets of ref_kat.cpp with a crossover score each, and one with an indel taboo
  {"unit",     1,  -1,  -1,   -1,  -1,  -1,  -1, 0},
  {"linear",  10, -15, -14,    0, -12,   0,  -9, 0},
  {"swapped", 10, -15, -20,  -20,  -2, -45,  -9, 0},
  {"steep",    7, -40, -40,  -60,  -1, -25, -30, 0},
  {"large",   32, -60, -60, -100, -20, -90, -25, 0},
  {"swapped_taboo", 10, -15, -20, -20, -2, -45, -9, 3},
};

int main(int argc, char** argv) {
  int n = argc > 1 ? atoi(argv[1]) : 1500;
  const bool local = argc > 2 && !strcmp(argv[2], "local");     // "L" records: the same cases through sw_full_cs(.., local_alignment = true) (ref: sw-full-cs.c:199-203,315,439-552); no C / S records
  const bool xover = argc > 2 && !strcmp(argv[2], "xover");     // "X" / "Y" records only
  const bool rna = argc > 2 && !strcmp(argv[2], "rna");         // C, S and L records on an RNA genome with is_rna = true
  const bool score_mode = argc > 2 && !strcmp(argv[2], "scores");   // "P" lines, and C, S, L, X and Y records under each of SCORE_SETS
  const bool anchor_mode = argc > 2 && !strcmp(argv[2], "anchors");   // "P" lines, and S and L records under each of ANCHOR_WIDTHS
  static const int ANCHOR_WIDTHS[] = {-1, 0, 1, 9, 99};
  std::mt19937_64 rng(20260202), xrng(20261005);
  const int n_sets = score_mode ? (int)(sizeof SCORE_SETS / sizeof SCORE_SETS[0]) : anchor_mode ? (int)(sizeof ANCHOR_WIDTHS / sizeof ANCHOR_WIDTHS[0]) : 1;
  for (int si = 0; si < n_sets; si++) {
  const ScoreSet& S = score_mode ? SCORE_SETS[si] : DEFAULT_SET;
  const int width = anchor_mode ? ANCHOR_WIDTHS[si] : 8;
  if (anchor_mode) rng.seed(20260202);                // the same cases under every width
  sw_vector_setup(1400, 1000, S.a_go, S.a_ge, S.b_go, S.b_ge, S.match, S.match + S.xover, 1, true);
  sw_full_cs_setup(1400, 1000, S.a_go, S.a_ge, S.b_go, S.b_ge, S.match, S.mismatch, S.xover, true, width, S.taboo);
  if (anchor_mode) printf("P w%d 1400 1000 %d %d %d %d %d %d %d %d %d\n", width, S.a_go, S.a_ge, S.b_go, S.b_ge, S.match, S.mismatch, S.xover, S.taboo, width);
  if (score_mode) printf("P %s 1400 1000 %d %d %d %d %d %d %d %d\n", S.name, S.a_go, S.a_ge, S.b_go, S.b_ge, S.match, S.mismatch, S.xover, S.taboo);
  for (int t = 0; t < n; t++) {
    int rlen = 20 + rng() % 56;                        // 20..75 colours
    int kind = rng() % 8;
    if (anchor_mode && t % 8 == 6) kind = 0;             // a window shorter than the read, together with a box
    int glen = (kind == 0) ? (int)(rlen - rng() % 6) : (int)(rlen * 1.4);
    if (glen < 8) glen = 8;
    int goff = 1 + rng() % 23;
    std::vector<int> g(goff + glen + 9);
    for (auto& b : g) b = rng() % 4;
    if (kind == 4) for (int k = 0; k < 3; k++) g[goff + rng() % glen] = 15;                 // N in the genome
    if (kind == 6) for (auto& b : g) b = rna ? 3 : 0;                                        // homopolymer: every tie rule fires
    if (rna) for (auto& b : g) if (b == 3) b = BASE_U;                                       // an RNA contig: uracil, no thymine
    // letter-space read = mutated copy of a window diagonal
    int start = goff + (glen > rlen ? rng() % (glen - rlen + 1) : 0);
    std::vector<int> rl(rlen);
    int gi = start;
    double psub = (kind == 1) ? 0.0 : (kind == 2 ? 0.10 : 0.02), pind = (kind == 3) ? 0.05 : 0.01;
    for (int i = 0; i < rlen; i++) {
      double u = (rng() % 100000) / 100000.0;
      if (u < pind) { rl[i] = rng() % 4; continue; }
      if (u < 2 * pind) gi += 1 + rng() % 3;
      int b = g[gi < (int)g.size() ? gi : (int)g.size() - 1]; if (b == BASE_U) b = 3; b &= 3; gi++;
      if ((rng() % 100000) / 100000.0 < psub) b = (b + 1 + rng() % 3) & 3;
      rl[i] = b;
    }
    int initbp = rng() % 4;
    std::vector<int> rc(rlen);
    for (int i = 0, last = initbp; i < rlen; i++) { rc[i] = lstocs(last, rl[i], false); last = rl[i]; }
    double pcol = (kind == 1) ? 0.0 : (kind == 5 ? 0.12 : 0.04);                             // colour (sequencing) errors -> crossovers
    for (int i = 0; i < rlen; i++) if ((rng() % 100000) / 100000.0 < pcol) rc[i] = (rc[i] + 1 + rng() % 3) & 3;
    if (kind == 7) for (int k = 0; k < 2; k++) rc[rng() % rlen] = 15;                        // '.' colours
    std::vector<uint32_t> gl((g.size() + 15) / 8 + 1, 0), gc((g.size() + 15) / 8 + 1, 0), rb(rlen / 8 + 1, 0);
    for (size_t i = 0; i < g.size(); i++) { put(gl, (int)i, g[i]); put(gc, (int)i, lstocs(i ? g[i - 1] : BASE_T, g[i], rna)); }   // ref: fasta.c:586-607
    for (int i = 0; i < rlen; i++) put(rb, i, rc[i]);
    int sv = sw_vector(gc.data(), goff, glen, rb.data(), rlen, gl.data(), initbp, rna);
    if (!local && !xover && !anchor_mode) { printf("C %d %d %d %d ", goff, glen, rlen, initbp); dump(gc); printf(" "); dump(gl); printf(" "); dump(rb); printf(" %d\n", sv); }
    struct anchor a; memset(&a, 0, sizeof a);
    a.x = (start - goff) + (int)(rng() % 7) - 3; a.y = 0; a.length = 10 + rng() % (rlen > 16 ? rlen - 10 : 6); a.width = 1 + rng() % 4; a.weight = 2;
    if (rng() % 4 == 0) { a.y = rng() % 10; a.x += a.y; }
    if (anchor_mode) {                                   // the boxes of oracle/ref_kat.cpp's mode "anchors"; d: the diagonal the read was copied from
      const int d = start - goff, half = a.length / 2;
      switch (t % 8) {
        case 2: a.x = -(1 + (int)(rng() % 5)); a.y = 0; a.width = 6 + rng() % 7; break;                                        // x < 0
        case 3: a.y = glen - d - half; if (a.y > rlen - 1) a.y = rlen - 1; if (a.y < 0) a.y = 0; a.x = d + a.y; break;          // x + length > glen
        case 4: a.y = rlen - half; if (a.y < 0) a.y = 0; a.x = d + a.y; break;                                                  // y + length > rlen
        case 5: a.width = (t % 16 == 5) ? 12 : 5 + rng() % 8; break;                                                            // up to 12 wide
        default: break;
      }
    }
    int thresh = (rng() % 3 == 0) ? (int)(0.6 * rlen * S.match) : (int)(0.3 * rlen * S.match);
    if (xover || score_mode) {
      // per-position scores as the read loop derives them from quality values: most positions good (near the global -20 .. -40), some poor (-1 .. -8)
      std::vector<int> xs(rlen);
      for (int i = 0; i < rlen; i++) { const int u = xrng() % 10; xs[i] = u < 6 ? -(int)(14 + xrng() % 27) : (u < 9 ? -(int)(1 + xrng() % 12) : -40); }
      if (score_mode) {                                                      // the same three bands, scaled to the set's crossover score and kept in [2 * global, -1]
        const int gx = -S.xover;
        for (int i = 0; i < rlen; i++) {
          const int u = xrng() % 10;
          int v = u < 6 ? gx * 7 / 10 + (int)(xrng() % (gx * 13 / 10 + 1)) : (u < 9 ? 1 + (int)(xrng() % (gx * 6 / 10 + 1)) : 2 * gx);
          xs[i] = -(v < 1 ? 1 : (v > 2 * gx ? 2 * gx : v));
        }
      }
      for (int md = 0; md < 2; md++) for (int rv = 0; rv < 2; rv++) {
        if (md == 1 && (t & 1)) continue;                                    // local mode on every other case
        if (score_mode && rv != ((t >> 1) & 1)) continue;                    // one strand a case
        struct sw_full_results sfr; memset(&sfr, 0, sizeof sfr);
        sw_full_cs(gl.data(), goff, glen, rb.data(), rlen, initbp, thresh, &sfr, rv != 0, false, &a, 1, md, xs.data());
        printf("%s %d %d %d %d %lld %lld %d %d %d %d ", md ? "Y" : "X", goff, glen, rlen, initbp, (long long)a.x, (long long)a.y, a.length, a.width, rv, thresh);
        dump(gl); printf(" "); dump(rb); printf(" ");
        for (int i = 0; i < rlen; i++) printf("%s%d", i ? "," : "", xs[i]);
        printf(" %d %d %d %d %d %d %d %d %d %d %s %s\n", sfr.score, sfr.read_start, sfr.rmapped, sfr.genome_start, sfr.gmapped,
               sfr.matches, sfr.mismatches, sfr.insertions, sfr.deletions, sfr.crossovers,
               (sfr.dbalign && sfr.dbalign[0]) ? sfr.dbalign : "-", (sfr.qralign && sfr.qralign[0]) ? sfr.qralign : "-");
        free(sfr.dbalign); free(sfr.qralign);
      }
      if (!score_mode) continue;
    }
    for (int md = 0; md < (rna || score_mode || anchor_mode ? 2 : 1); md++) for (int rv = 0; rv < 2; rv++) {
      const bool loc = rna || score_mode || anchor_mode ? md == 1 : local;
      if (score_mode && loc && rv != (t & 1)) continue;                      // L records: one strand a case
      struct sw_full_results sfr; memset(&sfr, 0, sizeof sfr);
      sw_full_cs(gl.data(), goff, glen, rb.data(), rlen, initbp, thresh, &sfr, rv != 0, rna, &a, 1, loc ? 1 : 0, NULL);
      printf("%s %d %d %d %d %lld %lld %d %d %d %d ", loc ? "L" : "S", goff, glen, rlen, initbp, (long long)a.x, (long long)a.y, a.length, a.width, rv, thresh);
      dump(gl); printf(" "); dump(rb);
      printf(" %d %d %d %d %d %d %d %d %d %d %s %s\n", sfr.score, sfr.read_start, sfr.rmapped, sfr.genome_start, sfr.gmapped,
             sfr.matches, sfr.mismatches, sfr.insertions, sfr.deletions, sfr.crossovers,
             (sfr.dbalign && sfr.dbalign[0]) ? sfr.dbalign : "-", (sfr.qralign && sfr.qralign[0]) ? sfr.qralign : "-");
      free(sfr.dbalign); free(sfr.qralign);
    }
  }
  }
  return 0;
}
