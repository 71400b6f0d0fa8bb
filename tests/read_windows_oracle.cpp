// read_windows_oracle.cpp -- TEST INFRASTRUCTURE: the candidate windows of a read batch from the CPU restatement (oracle/gm_oracle.hpp), for tests/test_read_windows.py.
//
// The oracle's C API has no window dump, so this driver brings one: gmo_map_tophits of oracle/gm_oracle_main.cpp stopped before read_pass1.  It is compiled by the test
// with the flags of oracle/Makefile into pytest's temporary directory:
//     g++ -O2 -std=c++17 -fopenmp -Wall -Wno-unused-function -shared -fPIC -I oracle -o <tmp>/librwo.so tests/read_windows_oracle.cpp
#include "gm_oracle.hpp"
#include <omp.h>

using namespace gmo;

namespace {
struct Session { Mapper M; Genome G; Index I; };
// as oracle/gm_oracle_main.cpp turns code rows into the text the read loop sees
std::string code_seq(const uint8_t* c, int L) { std::string s(L, 'N'); for (int i = 0; i < L; i++) s[i] = LSTRANS[c[i] & 15]; return s; }
// colour space: code 0 is the primer letter, the rest are colours (0-3, anything else '.')
std::string code_seq_cs(const uint8_t* c, int L) { std::string s(L, '.'); if (L) s[0] = LSTRANS[c[0] & 3]; for (int i = 1; i < L; i++) if (c[i] < 4) s[i] = (char)('0' + c[i]); return s; }
}  // namespace

extern "C" {

// the binary's defaults (letter space, or gmapper-cs with colour != 0) with the given match mode, automatic list cutoff
void* rwo_create_opts(int n_contigs, const uint8_t* const* codes, const uint64_t* lens, int colour, int match_mode, int hash_seeds, int n_seeds, const char* const* seeds);
void* rwo_create(int n_contigs, const uint8_t* const* codes, const uint64_t* lens, int colour, int match_mode) {
  return rwo_create_opts(n_contigs, codes, lens, colour, match_mode, 0, 0, nullptr);
}
// ... with a seed set of its own (n_seeds == 0: the defaults) and -H (hash_seeds != 0), as oracle/gm_oracle_main.cpp's "seeds=" and "hash-spaced-kmers=" options set them
void* rwo_create_opts(int n_contigs, const uint8_t* const* codes, const uint64_t* lens, int colour, int match_mode, int hash_seeds, int n_seeds, const char* const* seeds) {
  Session* S = new Session();
  load_default_seeds(S->M.P); derive_score_probs(S->M.P);
  if (colour) set_colour_space(S->M.P);
  S->M.P.match_mode = match_mode;
  S->M.P.Hflag = hash_seeds != 0;
  if (n_seeds > 0) {
    S->M.P.seeds.clear(); S->M.P.max_seed_span = 0; S->M.P.min_seed_span = 64;
    for (int i = 0; i < n_seeds; i++) add_spaced_seed(S->M.P, seeds[i]);
  }
  S->G.colour = S->M.P.colour;
  for (int c = 0; c < n_contigs; c++) {
    char nm[64]; snprintf(nm, sizeof nm, "contig%d", c + 1);
    S->G.add_contig(nm, codes[c], (size_t)lens[c]);
  }
  build_index(S->M.P, S->G, S->I);
  S->M.P.list_cutoff = auto_list_cutoff(S->M.P, S->G);
  S->M.G = &S->G; S->M.I = &S->I;
  return S;
}
void rwo_destroy(void* s) { delete (Session*)s; }
// window geometry as the options carry it: a percentage (of the read, of the window), or below zero an absolute count (-w, -l)
void rwo_set_windows(void* s, double window_len, double window_overlap) { Session* S = (Session*)s; S->M.P.window_len = window_len; S->M.P.window_overlap = window_overlap; }

// Every hit of both strands of every read, as the lists stand before pass 1: rows of 12 int64
//   read st cn g_off w_len score_window_gen matches anchor.x anchor.y anchor.length anchor.width 0
// read by read, strand 0 then strand 1, each list in its own order.  codes: n x L (colour space: the primer letter code, then L - 1 colours).
// Returns the number of rows there are; only the first `cap` are written.
long rwo_windows(void* s, int n, int L, const uint8_t* codes, int nthreads, long long* rows, long cap) {
  Session* S = (Session*)s;
  std::vector<std::vector<long long>> per(n);
#pragma omp parallel num_threads(nthreads > 0 ? nthreads : 1)
  {
    ThreadState T; S->M.init_thread(T);
#pragma omp for schedule(dynamic, 64)
    for (int i = 0; i < n; i++) {
      Read re; re.seq = S->M.P.colour ? code_seq_cs(codes + (size_t)i * L, L) : code_seq(codes + (size_t)i * L, L); re.name = "r";
      S->M.prepare_read(re);
      S->M.read_get_mapidxs(re);
      T.region_map_id++; T.region_map_id &= ((1 << Mapper::region_map_id_bits) - 1);
      S->M.read_get_region_counts(T, re, 0); S->M.read_get_region_counts(T, re, 1);
      S->M.read_get_anchor_list(T, re, 0); S->M.read_get_anchor_list(T, re, 1);
      S->M.read_get_hit_list(re, 0); S->M.read_get_hit_list(re, 1);
      for (int st = 0; st < 2; st++)
        for (const Hit& h : re.hits[st]) {
          const long long r[12] = {i, h.st, h.cn, h.g_off_pos_strand, h.w_len, h.score_window_gen, h.matches, h.anchor.x, h.anchor.y, h.anchor.length, h.anchor.width, 0};
          per[i].insert(per[i].end(), r, r + 12);
        }
    }
  }
  long w = 0;
  for (int i = 0; i < n; i++)
    for (size_t k = 0; k + 12 <= per[i].size(); k += 12) { if (w < cap) memcpy(rows + (size_t)w * 12, &per[i][k], 12 * sizeof(long long)); w++; }
  return w;
}

}  // extern "C"
