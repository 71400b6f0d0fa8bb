// gm_internal.h -- host-side objects behind the opaque handles of include/gmapper_hip.h
#pragma once
#include "gm_common.h"

struct GmSeedHost {
  uint64_t mask = 0; int span = 0, weight = 0;
  int kbits = 0;                        // log2(number of lists): 2 * weight, or 24 with -H (ref: genome.c:1034)
  uint32_t* d_dir = nullptr; uint32_t* d_pos = nullptr; uint32_t* d_bkt = nullptr;
  uint32_t* d_sdir = nullptr; uint32_t* d_spos = nullptr; uint32_t n_spos = 0;   // strip lists (gm_index_derive_strips)
  uint32_t n_pos = 0; uint64_t dir_words = 0;
  std::string text;
};

struct GmIndexHost {
  int device = 0;
  uint64_t total_len = 0;
  int n_contigs = 0;
  std::vector<uint32_t> contig_off;     // n_contigs + 1
  std::vector<std::string> names;
  uint32_t* d_genome = nullptr; uint64_t genome_words = 0;
  uint32_t* d_genome_cs = nullptr;      // colour space: colour translation of d_genome (same coordinates)
  uint32_t* d_contig_off = nullptr;
  // RNA contigs (uracil and no thymine, ref: fasta.c:528-542), derived on the device from the resident genome (gm_index_derive_rna: after a build, a load or a
  // broadcast alike): each contig's own flag, and the LAST contig's as genome_is_rna (genome.c:1063-1064)
  bool rna_ready = false; std::vector<uint8_t> contig_rna; uint8_t* d_contig_rna = nullptr; int genome_is_rna = 0;
  int n_seeds = 0, min_seed_span = 64, max_seed_span = 0;
  GmSeedHost seeds[GM_MAX_SEEDS];
  int slab_bits = 29, n_slabs = 1;
  gm_params_t params;
  uint32_t list_cutoff = 0;
  bool strips_ready = false;
  double fasta_to_bitfield_s = 0, fasta_total_s = 0;   // gm_index_build_fasta: seconds until the device build of the lists started, and of the whole call
  GmIndexDev dev_view() const;
};
struct gm_index : GmIndexHost {};

// stats slots written by the kernels (uint64 each)
enum { GS_LOOKUPS = 0, GS_ENTRIES, GS_SURVIVORS, GS_ANCHORS, GS_WINDOWS, GS_VEC_CALLS, GS_VEC_CELLS, GS_VEC_BYPASSED,
       GS_FULL_CALLS, GS_FULL_CELLS, GS_EXACT_ORDER, GS_OVERFLOW_SURV, GS_OVERFLOW_HITS, GS_PRUNED, GS_MP_UNFILTERED, GS_N };
// Counters are striped: same-address device atomics retire at ~12 ns each (MI355X_MICROARCH 'fanin'),
// which at one atomic per wave would cost more than the kernels themselves.  Stripe = block & 1023,
// one 128-byte line per stripe; the host sums the stripes.
#define GS_STRIPES 1024
#define GS_STRIDE 16
#define GS_ADD(stats, slot, val) atomicAdd(&(stats)[(size_t)(blockIdx.x & (GS_STRIPES - 1)) * GS_STRIDE + (slot)], (unsigned long long)(val))

// Tuning / path-forcing knobs (environment variables GM_K1_*, GM_K4_*, GM_K5_*, GM_SCAP, ... -- the kernel-variant tests force code paths with them) and
// the ablation bits of the lookup kernels exist only in builds with -DGM_TUNING (the Makefile's default; `make TUNING=0` is the release build: the knobs
// read as unset and every ablation branch folds away).  GM_HOST_THREADS, GM_OVERLAP and GM_POST_SW_HOST are run-time options of every build.
#include <cstdlib>
#include <cctype>
#include <string>
#include <vector>
#ifdef GM_TUNING
static inline const char* gm_tune(const char* name) { return getenv(name); }
#define GM_ABL(bits) (ablate & (bits))
#else
static inline const char* gm_tune(const char*) { return nullptr; }
#define GM_ABL(bits) (false)
#endif
#include "gm_lookup_plan.h"
// the knobs of the seed lookup's plan (GM_K1_*, GM_K4_*, GM_K5_*, GM_NO_V5, GM_NO_BUCKETS, GM_BKT_*): all unset in the release build
static inline K1Tune gm_k1_tune() { return k1_tune_read(gm_tune); }

// ---- kernel launchers (one per .hip file) -----------------------------------------------------
int gm_index_build_device(GmIndexHost* ix, hipStream_t stream);
// Genome FASTA files -> one bitfield in global coordinates, packed on the device (gm_fasta.hip).  On success d_genome ((total + 7) / 8 + 64 words, zero behind the
// last base; the allocation may be up to an eighth larger) is the caller's; on failure nothing is left allocated.
struct GmFastaGenome { uint32_t* d_genome = nullptr; uint64_t words = 0, total = 0; std::vector<std::string> names; std::vector<uint32_t> lens; };
int gm_fasta_to_device(int n_files, const char* const* paths, GmFastaGenome* out);
// GM_OK up to GM_MAX_CONTIGS contigs; beyond: GM_E_RANGE and a message with the count and the limit (gm_host.hip)
int gm_refuse_contig_count(const char* who, unsigned long long n_contigs);
// extract_name (ref: common/fasta.c:242-283) on a '>' / '@' line without its '\n': what follows the mark up to the first tab, trimmed, cut at the first blank
static inline std::string gm_extract_name(const std::string& line) {
  size_t b = 1, e = line.find('\t', 1); if (e == std::string::npos) e = line.size();
  while (b < e && isspace((unsigned char)line[b])) b++; while (e > b && isspace((unsigned char)line[e - 1])) e--;      // strtrim
  size_t k = b; while (k < e && line[k] != ' ' && line[k] != '\t') k++;
  return line.substr(b, k - b);
}
int gm_index_colour_genome_device(GmIndexHost* ix, hipStream_t stream);   // derives d_genome_cs from d_genome
int gm_index_from_lists_device(GmIndexHost* ix, int sn, const uint32_t* lens, const uint32_t* pos, uint32_t total);

// Raises `kernel`'s dynamic-LDS limit on the current device to `bytes` where that is above 48 KB and above what was set there before (hipFuncSetAttribute acts on
// the current device's code object: a process that maps on a second device raises it there too).  One lock and one high-water mark per (device, kernel): a limit
// is never lowered, also when two threads launch the same kernel at once.
hipError_t gm_lds_at_least(const void* kernel, size_t bytes);

// The launch scratch of the seed lookup (K1) and its prune (K1b).  One per session: every launch that touches it is queued on the session's front stream
// (s->stream), so its buffers are allocated on first use, grown only after that stream has drained, and freed with the session.
struct GmK1Scratch {
  int cus = 0;                                                    // the device's CU count (read once)
  uint64_t* k4_bins = nullptr; size_t k4_words = 0;               // k_lookup_v4: candidate bins
  uint32_t* k4_fb = nullptr;                                      // k_lookup_v4: fall-back list (+ its counter)
  uint32_t* k5_fb = nullptr; uint32_t* k5_pl = nullptr; int k5_cap = 0;   // k_lookup_v5: read-strands for the lane-per-list kernel + K1b / for K1b only (+ a counter each)
  uint2* k5_spill = nullptr; size_t k5_spill_n = 0;               // k_lookup_v5_rounds: candidate rows of the rounds after the first
  uint32_t* k1b_list = nullptr; int k1b_cap = 0;                  // k_prune_v2: read-strands left to k_prune (+ their counter)
  // in: pinned words the persistent K1 grid raises when its workgroups are resident (null: none), and this launch's epoch
  uint32_t* start_flags = nullptr; int flag_cap = 0; uint32_t epoch = 0;
  // out, of the last launch: workgroups that will raise a flag (0: none); the K1 variant chosen
  int flag_grid = 0; const char* kernel = nullptr;
  void release() {
    void* ptrs[] = {k4_bins, k4_fb, k5_fb, k5_pl, k5_spill, k1b_list};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    *this = GmK1Scratch();
  }
};

// K1 seed lookup + region filter: one workgroup per read-strand; read-strands with more than scap
// survivors are listed in d_heavy_list (count in d_surv_cnt) and re-run by gm_launch_lookup_redo
// Optional fusion of K1b into K1 (k_lookup_v5): when `fuse` is given and the chosen kernel can apply the prune rules itself, the kept
// keys go straight to fuse->d_surv2 / d_surv_cnt2 and *fuse->fused is set to 1 (the caller then skips gm_launch_prune).
struct GmFusePrune { uint64_t* d_surv2; uint32_t* d_surv_cnt2; int scap2; int window_len; int e_max; int* fused; };
int gm_launch_lookup(const GmIndexDev& ix, const uint32_t* d_reads, int n_reads, int read_len, int read_words,
                     uint64_t* d_surv, uint32_t* d_surv_cnt, int scap, uint32_t* d_heavy_list, uint32_t* d_heavy_cnt, int heavy_cap,
                     unsigned long long* d_stats, hipStream_t stream, GmK1Scratch* K, uint32_t* d_surv_seg = nullptr,   // d_surv_seg[rs][S + 1]: survivors after each slab
                     const GmFusePrune* fuse = nullptr);
int gm_index_derive_rna(GmIndexHost* ix, hipStream_t stream);        // per-contig RNA flags (gm_index.hip); idempotent
int gm_index_derive_strips(GmIndexHost* ix, hipStream_t stream);     // strip lists for k_lookup_v5 (gm_lookup5.hip); idempotent
// One lookup call as the host describes it to its kernel launches: index view, reads, geometry of a read-strand, output rows (stride scap), counters, heavy list, stats, stream
struct K1Call {
  const GmIndexDev& ix; const uint32_t* reads; int n_reads, read_len, read_words; K1Geom g; uint64_t* surv; uint32_t* surv_cnt; int scap;
  uint32_t* heavy_list; uint32_t* heavy_cnt; int heavy_cap; unsigned long long* stats; uint32_t* surv_seg; hipStream_t stream;
};
// k_lookup_v5 in the shape the plan gave: allocates, clears, launches.  1: launched; 0: no scratch; < 0: error.  The kept keys go to d_out (stride out_cap) / d_out_cnt -- with
// sh.prune K2's rows, c.surv then takes the raw members of read-strands that keep too many.  Its fall-back lists: K->k5_fb, K->k5_pl.  wlist: GM_K5_WLIST of the tuning build.
int gm_lookup5_launch(const K1Call& c, const K5Shape& sh, int wlist, uint64_t* d_out, uint32_t* d_out_cnt, int out_cap, GmK1Scratch* K);
int gm_launch_lookup_redo(const GmIndexDev& ix, const uint32_t* d_reads, int n_reads, int read_len, int read_words,
                          int n_heavy, const uint32_t* d_redo_list, const uint64_t* d_redo_off, uint64_t* d_out,
                          unsigned long long* d_stats, hipStream_t stream);

// K1b: exact removal of survivors with no other survivor within window_len + read_len (gm_prune.hip); the kept
// ones go to d_surv2 (stride scap2), d_surv_cnt2 = their number, or 0xFFFFFFFF for read-strands of the heavy tier
int gm_launch_prune(int n_reads, int read_len, int window_len, int e_max, int n_slabs, int slab_bits, const uint64_t* d_surv, const uint32_t* d_surv_cnt,
                    const uint32_t* d_surv_seg, int scap,
                    uint64_t* d_surv2, uint32_t* d_surv_cnt2, int scap2, uint32_t* d_heavy_list, uint32_t* d_heavy_cnt, int heavy_cap,
                    unsigned long long* d_stats, hipStream_t stream, GmK1Scratch* K,
                    const uint32_t* d_rs_list = nullptr, const uint32_t* d_rs_cnt = nullptr, int rs_cap = 0);   // list mode: only the listed read-strands

// K2 anchors + candidate windows: one wave per read-strand (LDS tier) + heavy tier on global arrays
int gm_launch_anchors(const GmIndexDev& ix, const GmScoreDev& sc, int n_reads, int read_len, int window_len,
                      const uint64_t* d_surv, const uint32_t* d_surv_cnt, int scap,
                      GmHit* d_hits, uint16_t* d_perm, uint32_t* d_hit_cnt, int hcap, unsigned long long* d_stats, hipStream_t stream);
int gm_launch_anchors_heavy(const GmIndexDev& ix, const GmScoreDev& sc, int n_reads, int read_len, int window_len,
                            int n_heavy, const uint32_t* d_heavy_list, const uint64_t* d_seg_off, const uint32_t* d_seg_n,
                            const uint32_t* d_seg_begin32, const uint32_t* d_seg_end32, uint64_t total_keys,
                            uint64_t* d_keys_in, uint64_t* d_keys_sorted, uint32_t* d_aux, uint32_t* d_nxt, uint32_t* d_ord,
                            GmHit* d_hits, uint16_t* d_perm, uint32_t* d_hit_cnt, int hcap, unsigned long long* d_stats, hipStream_t stream);

// Export of K2's windows (gm_read_windows, gm_windows.hip).  gm_launch_win_scan: d_off[0 .. n_rs] = exclusive scan of min(d_hit_cnt[rs], hcap), d_off[n_rs] = their
// sum (one launch).  gm_launch_win_scatter: window j of the `total` = d_off[n_rs] windows, read through d_perm, becomes d_out[j] with read = read_base + rs / 2.
int gm_launch_win_scan(const uint32_t* d_hit_cnt, int n_rs, int hcap, unsigned long long* d_off, hipStream_t stream);
int gm_launch_win_scatter(const GmHit* d_hits, const uint16_t* d_perm, const unsigned long long* d_off, int n_rs, int hcap, unsigned long long total, int read_base,
                          gm_read_window_t* d_out, hipStream_t stream);

// The selection seams (gm_select_pass1 / gm_select_pass2, gm_select.hip); GM_SEL_MAX below bounds K and the items of a read.
//   gm_launch_sel_pass1: a wave a read over wins[off[2 r] .. off[2 r + 2]) with their scores: overlap rule, threshold and the ext-heap; d_sel_id / d_sel_score[r * K ..]
//                        = window index and score after the rule of the d_sel_cnt[r] selected windows, in heap array order.
//   gm_launch_sel_emit:  the selected windows as records at d_hit_off[r] + slot, strand 1 turned by reverse_hit.
//   gm_launch_sel_pass2: a wave a read over items[hit_off[r] .. hit_off[r + 1]) (at most 64): d_order[hit_off[r] + k] = the item (0-based within the read) that is
//                        the k-th final mapping, d_cnt[r] = their number.
struct GmSel2Item { int32_t grp, start, endkey, key, score_full, keep; };      // grp = cn * 2 + gen_st; keep: the host's threshold compare
int gm_launch_sel_pass1(const GmScoreDev& sc, int n_reads, int read_len, int K, int window_len, int overlap_abs, const gm_read_window_t* d_wins,
                        const unsigned long long* d_off, const int* d_scores, int32_t* d_sel_id, int32_t* d_sel_score, uint32_t* d_sel_cnt, hipStream_t stream);
int gm_launch_sel_emit(const GmScoreDev& sc, int n_reads, int read_len, int K, const gm_read_window_t* d_wins, const uint32_t* d_contig_off, const int32_t* d_sel_id,
                       const int32_t* d_sel_score, const uint32_t* d_sel_cnt, const unsigned long long* d_hit_off, gm_pass1_hit_t* d_out, hipStream_t stream);
int gm_launch_sel_pass2(int n_reads, int num_outputs, int strata, int max_alignments, const unsigned long long* d_hit_off, const GmSel2Item* d_items,
                        int32_t* d_order, uint32_t* d_cnt, hipStream_t stream);

// Pass 1 as a seam (gm_score_windows / gm_select_pass1_f1 / gm_read_hits).
//   gm_launch_score_windows (gm_sw.hip): d_scores[i] = the score f1_run computes for window i of d_wins (never cut short), d_slots[i] (or null) = its f1 cache slot;
//                        window i's read is row d_wins[i].read - read_base of d_reads (d_initbp likewise; ix.read_rna: those rows' RNA flags or null); max_w >= every
//                        w_len; d_stats (or null): GS_VEC_CALLS / GS_VEC_CELLS are added to.  The host has checked the windows against the index and the batch.
//   gm_launch_sel_pass1_f1 (gm_select.hip): gm_launch_sel_pass1 with the f1 call cache (ref: f1-wrapper.h:97-134) per read-strand: d_comp, n_wins words of 64 bits,
//                        holds the (slot, score) pairs of the computed windows of the read-strand being walked; d_byp[r] = read r's bypassed calls.
#define GM_SCORE_WIN_LDS_LIMIT (48 * 1024)      // LDS a wave of k_score_windows may take (the read, the window, colour space its first-colour row, the carry rows)
#define GM_SCORE_WIN_CHUNK 1                    // consecutive windows a wave of k_score_windows takes at a time (it keeps the read while they share a read-strand); GM_SCORE_CHUNK in tuning builds
size_t gm_score_windows_lds(int colour, int read_len, int max_w);
int gm_launch_score_windows(const GmIndexDev& ix, const GmScoreDev& sc, unsigned long long n, const gm_read_window_t* d_wins, const uint32_t* d_reads, int read_len,
                            int read_words, int read_base, const uint8_t* d_initbp, int max_w, int* d_scores, uint32_t* d_slots, unsigned long long* d_stats,
                            hipStream_t stream);
int gm_launch_sel_pass1_f1(const GmScoreDev& sc, int n_reads, int read_len, int K, int window_len, int overlap_abs, const gm_read_window_t* d_wins,
                           const unsigned long long* d_off, const int* d_scores, const uint32_t* d_slots, unsigned long long* d_comp, int32_t* d_sel_id,
                           int32_t* d_sel_score, uint32_t* d_sel_cnt, uint32_t* d_byp, hipStream_t stream);

// K3 pass 1 (vector SW + overlap rule), one wave per read-strand
int gm_launch_pass1(const GmIndexDev& ix, const GmScoreDev& sc, const uint32_t* d_reads, int n_reads, int read_len, int read_words,
                    int window_len, int window_overlap_abs, GmHit* d_hits, const uint16_t* d_perm, const uint32_t* d_hit_cnt, int hcap,
                    unsigned long long* d_slots, unsigned long long* d_stats, hipStream_t stream,
                    const int32_t* d_pair_min = nullptr, const uint8_t* d_saved = nullptr,   // paired mode: only_paired / saved windows
                    const uint8_t* d_initbp = nullptr,                                         // colour space: primer letter per read
                    bool early_stop = false);       // unpaired reads: a window may stop once it cannot reach the threshold (its score is then a lower bound below it)

// K4a top-K selection (ref: read_get_vector_hits), one thread per read; K4b pass 2, one wave per selected hit
#define GM_SEL_MAX 64
// The pair selection of paired pass 2 on the device (gm_pair_mappings, gm_pair_select.hip; gm_map_pairs* keeps its host loop).
//   gm_launch_pair_sel_items: d_items[i] from the paired pass 2's record d_res[i] and the host's score_full of it.
//   gm_launch_sel_pair_pass2: a wave a pair over its d_pcnt[pr] candidate pairs d_plist[pr * GM_SEL_MAX ..] = (a << 8) | b, a / b windows of the pair's slices
//                             d_items{0,1}[d_off{0,1}[pr] .. + d_cnt{0,1}[pr]): d_out[pr * GM_SEL_MAX + k] = the k-th final pair in the same form, d_cnt[pr] their number.
//                             d_thr_tab[s], s < thr_n: the integer threshold for two windows whose score_max sum to s; abs_key: the key is the score, not its percentage.
struct GmPairSelItem { int32_t grp, start, endkey, score_full, score_max, sort_idx; };      // grp = cn * 2 + gen_st
int gm_launch_pair_sel_items(int n, const GmFullRes* d_res, const int32_t* d_score_full, GmPairSelItem* d_items, hipStream_t stream);
int gm_launch_sel_pair_pass2(int n_pairs, int abs_key, int num_outputs, int strata, int max_alignments, const int* d_thr_tab, int thr_n, const uint32_t* d_plist,
                             const uint32_t* d_pcnt, const GmPairSelItem* d_items0, const uint32_t* d_off0, const uint32_t* d_cnt0, const GmPairSelItem* d_items1,
                             const uint32_t* d_off1, const uint32_t* d_cnt1, uint32_t* d_out, uint32_t* d_cnt, hipStream_t stream);
int gm_launch_select(const GmScoreDev& sc, int n_reads, int read_len, const GmHit* d_hits, const uint16_t* d_perm,
                     const uint32_t* d_hit_cnt, int hcap, int32_t* d_sel, uint32_t* d_sel_cnt, uint32_t* d_sel_off,
                     uint32_t* d_work, uint32_t* d_n_work, hipStream_t stream, const uint8_t* d_saved = nullptr);
int gm_launch_build_work(int n_reads, const uint32_t* d_sel_cnt, uint32_t* d_sel_off, uint32_t* d_work, uint32_t* d_n_work, hipStream_t stream);
// anchor_width < 0 (no anchor band): both pass-2 launchers first OVERWRITE the anchor boxes of the selected hits in d_hits with the band the launch's threshold allows
// (k_threshold_box_hits, gm_sw.hip) -- after such a launch d_hits no longer holds what window generation found for them.  Nothing reads the boxes behind pass 2.
int gm_launch_pass2(const GmIndexDev& ix, const GmScoreDev& sc, const uint32_t* d_reads, int n_reads, int read_len, int read_words,
                    int window_len, GmHit* d_hits, const uint16_t* d_perm, int hcap, const int32_t* d_sel, const uint32_t* d_sel_cnt,
                    const uint32_t* d_work, const uint32_t* d_n_work, GmFullRes* d_res, uint8_t* d_ops, int ops_stride,
                    uint8_t* d_back, size_t back_stride, int grid, unsigned long long* d_stats, hipStream_t stream,
                    const int32_t* d_sel_sidx = nullptr, int input_strand = 0, int write_back = 0,
                    uint32_t* d_order = nullptr, uint32_t* d_cls_cnt = nullptr);        // the work items listed by kind (as many words as d_work), four counter words; without them: the one-window kernel

// gm_pass2_max_window, gm_pass2_g4_lds (letter space, ng = 4 / 8 windows a wave), gm_pass2_cs_lds (colour space, ng = 1 / 4 / 8), gm_prune_lds, GM_SWF_LDS_LIMIT
#include "gm_pass2_sizes.h"

// colour-space pass 2 (sw_full_cs per selected window); ops_stride bytes per result: backtrace bytes, then (genome << 4 | read) codes
// colour-space post_sw on the device (gm_post.hip): constants = CsPostConsts of gm_host.hip (logs taken on the host), one record per pass-2 result
struct GmCsPostDev { double let_m, let_x, col_m[2], col_x[2], pr_del_open, pr_del_extend, pr_ins_open, pr_ins_extend;
                     // reads with quality values (csfastq): qv[read][colour] = the colour's QV clamped to 0..250, qtab[2 q] / [2 q + 1] = log(1 - e(q)) / log(e(q) / 3) as the HOST's libm
                     // computes them (ref: sw-post.c:486-491), bq[result][read position] receives the base qualities (PHRED + 33, ref: :568-586); all null without QVs
                     const uint8_t* qv; const double* qtab; uint8_t* bq; };
struct GmPostRes { double posterior; int32_t cs_match, cs_mismatch, cs_xover, valid; };
#define GM_POST_THREADS 131072      // k_post_sw_cs: one thread per pass-2 result, a column scratch each (6.9 KB at 50 colours); 32 768 threads were half a wave per SIMD for a kernel that waits on its scratch: cfg4 5.62 -> 6.00 M reads/s (tools/post_threads_cfg4.sh)
int gm_launch_post_sw_cs(const GmCsPostDev& K, const uint32_t* d_reads, const uint8_t* d_initbp, int read_len, int read_words, const GmFullRes* d_res, uint8_t* d_ops,
                         int ops_stride, const uint32_t* d_n_work, uint32_t res_cap, GmPostRes* d_post, double* d_fw, uint32_t* d_info, int threads, hipStream_t stream);
// S3 batch (gm_post_sw_batch, k_post_sw_batch): one alignment of a gm_sw_full_cs_batch call.  The host fills an item only after it has checked the record against the caller's
// buffers: ops[ops_off .. + n_ops), genome positions from genome_start, read positions read_start .. < rlen of read `idx`; len = read positions in the alignment (columns
// of scratch the item takes), qual_off = where its base qualities go.  GmPostRes.valid: 1 answered, 2 the host routine decides.
// gbase / flags: where genome position p of the record lives in d_genome -- position gbase + p, or with flags & 1 (gm_post_sw_batch_ix, strand 1 of a contig: gbase is
// then the contig's LAST forward base) the complement of position gbase - p, an RNA contig's (flags & 2) with U for A.  The host-bitfield entry passes 0 for both.
struct GmPostItem { unsigned long long ops_off, qual_off; long long genome_start, gbase; uint32_t n_ops; int read_start, rlen, len, initbp, idx, flags; };
static const size_t GM_POST_COL_BYTES = 17 * 8 + 4;       // scratch a column and thread slot: 16 forward values, the column's scale, the column word
int gm_launch_post_sw_batch(const GmCsPostDev& K, int first, int n, int threads, const GmPostItem* d_items, const uint8_t* d_ops, const uint32_t* d_genome,
                            const uint32_t* d_reads, int read_words, int qv_stride, int is_rna, GmPostRes* d_post, uint8_t* d_qralign, uint8_t* d_quals,
                            double* d_fw, uint32_t* d_info, hipStream_t stream, int ix = 0);      // ix: the items carry gbase / flags (gm_post_sw_batch_ix)
int gm_launch_pass2_cs(const GmIndexDev& ix, const GmScoreDev& sc, const int* cs_params9, const uint32_t* d_reads, const uint8_t* d_initbp, int n_reads,
                       int read_len, int read_words, int window_len, GmHit* d_hits, int hcap, const int32_t* d_sel, const uint32_t* d_work,
                       const uint32_t* d_n_work, GmFullRes* d_res, uint8_t* d_ops, int ops_stride, uint32_t* d_back, size_t back_words, int grid,
                       unsigned long long* d_stats, hipStream_t stream, const int8_t* d_xover = nullptr,   // d_xover[n_reads][read_len]: per-position crossover scores (reads with QVs)
                       const int32_t* d_sel_sidx = nullptr,                                                // paired mode: sort index of every selected window
                       uint32_t* d_order = nullptr, uint32_t* d_cls_cnt = nullptr);                        // the work items listed by kind (as many words as d_work), four counter words

// paired mode (gm_pair.hip): mate ranges per window, pair top-K, saved marks, mate reversal
int gm_launch_revcomp_reads(uint32_t* d_reads, int n_reads, int read_len, int read_words, hipStream_t stream, const uint8_t* d_read_rna = nullptr);
int gm_launch_read_rna_flags(const uint32_t* d_reads, int n_reads, int read_len, int read_words, uint8_t* d_flags, hipStream_t stream);   // re->is_rna per packed letter-space read
struct MpDelta { int amin[2], amax[2], bmin[2], bmax[2]; };   // region deltas of mate 1 / mate 2 per strand (ref: mapping.c:2422-2430)
MpDelta gm_mp_region_deltas(int region_bits, const int* dmin1, const int* dmax1, const int* dmin2, const int* dmax2);
int gm_launch_mp_filter(int n_pairs, int region_bits, int region_overlap, uint64_t* d_surv1, uint32_t* d_cnt1, int scap1, uint64_t* d_surv2, uint32_t* d_cnt2, int scap2,
                        const int* dmin1, const int* dmax1, const int* dmin2, const int* dmax2, uint32_t* d_seg1, uint32_t* d_seg2, int n_slabs,
                        unsigned long long* d_unfiltered, hipStream_t stream);
int gm_launch_pair_up(int n_pairs, const GmHit* hits1, const uint16_t* perm1, const uint32_t* cnt1, int hcap1,
                      const GmHit* hits2, const uint16_t* perm2, const uint32_t* cnt2, int hcap2,
                      int32_t* pmin1, int32_t* pmax1, int32_t* pmin2, int32_t* pmax2, const int* delta_min, const int* delta_max, hipStream_t stream);
int gm_launch_pair_select(const GmScoreDev& sc, int n_pairs, int len1, int len2,
                          const GmHit* hits1, const uint16_t* perm1, const uint32_t* cnt1, int hcap1, const int32_t* pmin1, const int32_t* pmax1,
                          const GmHit* hits2, const uint16_t* perm2, const uint32_t* cnt2, int hcap2,
                          int32_t* sel1, int32_t* sidx1, uint32_t* selcnt1, int32_t* sel2, int32_t* sidx2, uint32_t* selcnt2,
                          uint32_t* pairs, uint32_t* pair_cnt, hipStream_t stream);
int gm_launch_mark_saved(uint8_t* d_saved, const uint32_t* d_list, int n, hipStream_t stream);

// One window of an index-resident seam call (gm_*_ix): glen positions of contig cn whose lowest FORWARD base is contig position foff; rc: the window is read on strand 1
// (the reverse complement of the contig), i.e. backwards and complemented.  The host has checked it against the contig (ix_window, gm_host.hip).
struct GmWin { uint32_t foff; int glen, cn, rc; };
int gm_launch_get_windows(const GmIndexDev& ix, int n, const GmWin* d_wins, int colours, uint32_t* d_words, int stride_words, hipStream_t stream);
// d_initbp null: letter space (load_window); else colour space (load_window_cs: colours and first-colour row; ix.genome_is_rna = the call's is_rna)
int gm_launch_sw_vector_batch_ix(const GmIndexDev& ix, const GmScoreDev& sc, int n, const GmWin* d_wins, const uint32_t* d_reads, int read_words, const int* d_rlen,
                                 const int* d_initbp, int max_g, int max_r, int* d_scores, hipStream_t stream, int early_thr = 0, uint8_t* d_stopped = nullptr);
// d_wins[i].glen is unused: the diagonal runs over the whole contig of the strand
int gm_launch_sw_gapless_batch_ix(const GmIndexDev& ix, int n, int match, int mismatch, const GmWin* d_wins, int colour_space, const uint32_t* d_reads, int read_words,
                                  const int* d_rlen, const int* d_gidx, const int* d_ridx, const int* d_initbp, int max_r, int* d_scores, hipStream_t stream);

// S1 batch kernel on caller-provided bitfields
int gm_launch_sw_vector_batch(const GmScoreDev& sc, int n, const uint32_t* d_genome, const long long* d_goff, const int* d_glen,
                              const uint32_t* d_reads, int read_words, const int* d_rlen, int max_g, int max_r, int* d_scores, hipStream_t stream,
                              int early_thr = 0, uint8_t* d_stopped = nullptr);   // > 0: pass 1's early stop against this threshold, stopped[i] = 1 where it fired

// colour space S1/S2 (gm_sw.hip): cs_params9 = match mismatch xover a_go a_ge b_go b_ge anchor_width indel_taboo_len (penalties positive)
int gm_launch_sw_gapless_batch(int n, int match, int mismatch, const uint32_t* d_genome, const uint32_t* d_genome_ls, const long long* d_woff, const int* d_glen,
                               const uint32_t* d_reads, int read_words, const int* d_rlen, const int* d_gidx, const int* d_ridx, const int* d_initbp, int max_r,
                               int* d_scores, hipStream_t stream);
int gm_launch_sw_vector_batch_cs(const GmScoreDev& sc, int n, const uint32_t* d_genome_cs, const uint32_t* d_genome_ls, const long long* d_goff,
                                 const int* d_glen, const uint32_t* d_reads, int read_words, const int* d_rlen, const int* d_initbp, int max_g, int max_r,
                                 int* d_scores, hipStream_t stream);

// S2 (sw_full_ls / sw_full_cs are calls of one item; gm_sw_full_ls_batch / gm_sw_full_cs_batch): one window as the batch kernels read it, and what they write back per window.
// flags: 1 = anchor box given (else the threshold band), 2 = revcmpl, 4 = the window is read on strand 1 (backwards and complemented; goff is then the global position of
// its lowest forward base), 8 = its contig is RNA (both 0 on caller bitfields); initbp: colour space only, the primer letter | GM_SEAM_RNA; idx: the caller's item
// (row of reads[] and of the crossover rows, slot of out[]); ops_off / ops_cap: the item's segment of the device ops buffer.
// By-row form (letter space, gm_read_mappings: k_sw_vector_items and k_sw_full_batch<.., true, true>): the read is row `initbp` of reads[] -- a field letter space never
// read -- and idx is the slot of out[] alone, so that the items of many hits name one copy of their read.
struct GmFullItem { long long goff, ax, ay; unsigned long long ops_off; int glen, rlen, alen, awidth, thresh, maxscore, flags, initbp, ops_cap, idx; };
// v[0..10] = score read_start rmapped genome_start (window-relative) gmapped matches mismatches insertions deletions crossovers n_ops
struct GmFullOut { int v[12]; };
size_t gm_sw_full_batch_lds(int max_g, int max_r);
size_t gm_sw_full_cs_batch_lds(int max_g, int max_r);
// items[first .. first + n) by `grid` waves; wave b owns back-pointer scratch d_back + b * back_stride (bytes; colour space: uint32 words)
int gm_launch_sw_full_batch(const GmScoreDev& sc, int first, int n, int grid, GmFullItem* d_items, const uint32_t* d_genome, const uint32_t* d_reads, int read_words,
                            int max_g, int max_r, uint8_t* d_back, size_t back_stride, GmFullOut* d_out, uint8_t* d_ops, int local, hipStream_t stream, int ix = 0,
                            int by_row = 0);      // by_row (with ix): the by-row form of GmFullItem

// Pass 2 as a seam (gm_read_mappings, gm_host_pass2.inc): the rule of hit_run_full_sw on hits that stay on the device.
//   gm_launch_p2_items (gm_pass2.hip): d_items[i] = the by-row pass-2 item of d_hits[i]; d_thresh_tab[m] = (int)abs_or_pct(sw_full_threshold, m * match) for m = 0 ..
//                        read_len, made on the host; every item gets ops_cap bytes of operations; d_thresh[i] = the item's thresh again, dense.
//   gm_launch_sw_vector_items (gm_sw.hip): d_scores[i] = sw_vector of item i's window (strand and RNA bits as the _ix kernels read them) against row d_items[i].initbp of
//                        d_reads: the second vector score, on the turned hit (ref: mapping.c:386-388).
//   gm_launch_p2_compact: d_work[0 .. *d_n_work) = the items with d_sv[i] >= d_thresh[i] in item order, maxscore = d_sv[i], ops_off = k * ops_cap; d_pos_of[i] = k, or
//                        -1 (two launches: the places, then the copies).
//   gm_launch_p2_records: d_recs[i] / d_p2in[i] from d_out[i] (the full kernel's, slot = hit) for a hit of the work list, the zero record for any other.
//   gm_launch_p2_sel_items: k_sel_pass2's items from the records, the hits and the host's answers.
struct GmP2In { int32_t score, rmapped, score_max; };        // what the host's double functions read of a hit
struct GmP2Host { int32_t score_full, key, keep; };          // what they answer
int gm_launch_p2_items(int n, const gm_pass1_hit_t* d_hits, int read_base, int read_len, const uint32_t* d_contig_off, const uint8_t* d_contig_rna, const int* d_thresh_tab,
                       int tiebreak_rev, int ops_cap, GmFullItem* d_items, int* d_thresh, hipStream_t stream);
int gm_launch_sw_vector_items(const GmScoreDev& sc, int n, const GmFullItem* d_items, const uint32_t* d_genome, const uint32_t* d_reads, int read_words, int max_g, int max_r,
                              int* d_scores, hipStream_t stream);
int gm_launch_p2_compact(int n, const GmFullItem* d_items, const int* d_thresh, const int* d_sv, GmFullItem* d_work, int* d_pos_of, uint32_t* d_n_work, hipStream_t stream);
int gm_launch_p2_records(int n, const gm_pass1_hit_t* d_hits, const int* d_pos_of, const GmFullOut* d_out, int ops_cap, gm_sw_full_rec_t* d_recs, GmP2In* d_p2in,
                         hipStream_t stream);
int gm_launch_p2_sel_items(int n, const gm_pass1_hit_t* d_hits, const gm_sw_full_rec_t* d_recs, const GmP2Host* d_ans, GmSel2Item* d_items, hipStream_t stream);
// Colour-space pass 2 as a seam (gm_read_mappings_cs, gm_host_pass2_cs.inc): every hit goes through sw_full_cs, then post_sw, on arrays that stay on the device.
// Colour-space by-row form of GmFullItem (k_sw_full_cs_batch<.., true, true>): initbp carries the primer letter | GM_SEAM_RNA, so the ROW of the sub-batch's reads -- and
// of the crossover rows -- rides in maxscore, a field sw_full_cs never reads; idx is the slot of out[] alone.
//   gm_launch_p2_items_cs: d_items[i] = that item of d_hits[i]: window, box, revcmpl and thresh as gm_launch_p2_items makes them, the primer letter of the read's row of
//                        d_initbp_rows, ops_off = i * ops_cap (no compaction: every hit is aligned).
//   gm_launch_p2_records_cs: d_recs[i] / d_p2in[i] from d_out[i]: the record gm_sw_full_cs_batch_ix leaves (all zero where there is no alignment); d_len[i] = the read
//                        positions post_sw will take of it (rmapped where score > 0, else 0).
//   gm_launch_p2_post_items: d_items[i] = k_post_sw_batch's item of hit i from its device record: operations, genome_start, read_start, len = rmapped, gbase / flags as
//                        gm_post_sw_batch_ix sets them, idx = the ROW of the read (k_post_sw_batch reads idx for the read and its QV row only: its answer goes to the item's
//                        own slot, so the existing <true> instantiation is the by-row form), qual_off = d_qoff[i], the exclusive scan of d_len (gm_launch_win_scan).  A hit
//                        without alignment gets an empty item (n_ops = len = 0), which the kernel leaves after two loads.
//   gm_launch_p2_move:   segment k: n bytes from d_src + seg.src to d_dst + seg.dst, a wave a segment.  The few items the host routine redoes: their operations come
//                        down packed (bytes bounded by those items), their re-called qralign and base qualities go back to their places.
struct GmP2Seg { unsigned long long src, dst; uint32_t len, pad; };
int gm_launch_p2_items_cs(int n, const gm_pass1_hit_t* d_hits, int read_base, int read_len, const uint32_t* d_contig_off, const uint8_t* d_contig_rna, const int* d_thresh_tab,
                          int tiebreak_rev, int ops_cap, const uint8_t* d_initbp_rows, int is_rna, GmFullItem* d_items, hipStream_t stream);
int gm_launch_p2_records_cs(int n, const gm_pass1_hit_t* d_hits, const GmFullOut* d_out, int ops_cap, gm_sw_full_rec_t* d_recs, GmP2In* d_p2in, uint32_t* d_len, hipStream_t stream);
int gm_launch_p2_post_items(int n, const gm_pass1_hit_t* d_hits, const gm_sw_full_rec_t* d_recs, const unsigned long long* d_qoff, int read_base, int read_len,
                            const uint32_t* d_contig_off, const uint8_t* d_contig_rna, const uint8_t* d_initbp_rows, GmPostItem* d_items, hipStream_t stream);
int gm_launch_p2_move(int n_segs, const GmP2Seg* d_segs, const uint8_t* d_src, uint8_t* d_dst, hipStream_t stream);
int gm_launch_sw_full_cs_batch(const int* cs_params9, int first, int n, int grid, GmFullItem* d_items, const uint32_t* d_genome_ls, const uint32_t* d_reads,
                               int read_words, int max_g, int max_r, const int8_t* d_xrows, int xstride, uint32_t* d_back, size_t back_words, GmFullOut* d_out,
                               uint8_t* d_ops, int local, hipStream_t stream, int ix = 0,      // ix: the items carry strand / RNA bits (gm_sw_full_cs_batch_ix)
                               int by_row = 0);      // by_row (with ix): the colour-space by-row form of GmFullItem

// Text of the alignments of an S2 batch call (gm_sw_full_batch_text[_ix], k_sw_text in gm_text.hip): one accepted record.  The host has checked it (swf_rec_check):
// ops[ops_off .. + n_ops), the genome positions from genome_start and the read positions read_start .. of read `idx` lie inside what was uploaded; tail = the read
// positions behind the alignment (the trailing clip).  gbase: as GmPostItem's; flags: 1 = strand 1 of a contig, 2 = its contig is RNA (both 0 on caller
// bitfields), 4 = the item is printed as a reverse-strand mapping (CIGAR runs reversed, edit string through reverse_alignment_edit_string).
struct GmTextItem { unsigned long long ops_off; long long genome_start, gbase; uint32_t n_ops; int read_start, tail, initbp, idx, flags; };
#define GM_TEXT_MAX_GRID 16384      // waves of one launch (grid-stride over the items): 64 a CU
// write = 0: the sizing launch -- d_lens[2 k] / [2 k + 1] = bytes of item k's CIGAR / edit string; write = 1: the bytes, at d_offs[2 k] / [2 k + 1] of d_cigar / d_edit
// (d_lens as the sizing launch left it), dbalign / qralign at the place of the operations in d_db / d_qr.  what: GM_TEXT_* bits; buffers of kinds not asked for may be
// null, d_genome / d_reads too when neither strings nor the edit string are; d_qin: null, or the qralign to use in place of the one rebuilt from the operations.
int gm_launch_sw_text(int n_items, const GmTextItem* d_items, int colour, int what, int write, const uint8_t* d_ops, const uint32_t* d_genome, const uint32_t* d_reads,
                      int read_words, int is_rna, const uint8_t* d_qin, int clip_char, uint32_t* d_lens, const unsigned long long* d_offs, uint8_t* d_db, uint8_t* d_qr,
                      uint8_t* d_cigar, uint8_t* d_edit, hipStream_t stream, int ix = 0);      // ix: the items carry gbase / flags (gm_sw_full_batch_text_ix)

// Text kernels (gm_text.hip, gm_sam.hip): eight characters as one 64-bit table, and the decimal digits of a 32-bit value.
constexpr uint64_t pack8(const char* s) { uint64_t v = 0; for (int i = 0; i < 8; i++) v |= (uint64_t)(uint8_t)s[i] << (8 * i); return v; }
__device__ __forceinline__ int ndig(uint32_t v) {
  return v < 10u ? 1 : v < 100u ? 2 : v < 1000u ? 3 : v < 10000u ? 4 : v < 100000u ? 5 : v < 1000000u ? 6 : v < 10000000u ? 7 : v < 100000000u ? 8 : v < 1000000000u ? 9 : 10;
}

// The SAM text of a chunk's mappings (gm_sam_records, k_sam_records in gm_sam.hip): one output record -- a mapping, or (cn < 0) the unaligned record of a read.  The host
// has checked it (gm_host_sam.inc): read < n_reads, cn inside the index, every slice inside its uploaded buffer; every integer the record prints is here, Z0 / Z1 through
// the host's log.  flags: 1 = the mapping is on strand 1; keep_lo / keep_hi: letter space, the read positions of the alignment (outside them a read that came as text
// prints the file's letter); pq_len == 0: QUAL of a colour-space record is '*'.
struct GmSamRec { unsigned long long cigar_off, edit_off, qr_off, pq_off; uint32_t cigar_len, edit_len, qr_len, pq_len, pos; int32_t read, cn, flags, mqv, as, z0, z1, nm, cm,
                  zm, zr, zv, zh, keep_lo, keep_hi; };
// names: null (the records are named r<read>), or the caller's text with name_off[r] the start of read r's name and name_off[r + 1] - 1 its end; seqs / quals: null, or
// one line a read of read_len (colour space, seqs: read_len + 1) characters and a separator; cnames / cname_off: the contig names end to end with n_contigs + 1
// offsets, the read group (rg_len bytes) behind them at cname_off[n_contigs]; dq: what re-bases a QV character to PHRED + 33; ztags: Z0 / Z1 are printed; extra: ZM ZR ZV
// ZH ZE are.  lens: the sizing launch's output, one length a record; offs / out: the writing launch's, record k at out + offs[k].
struct GmSamArgs { const GmSamRec* recs; int n_recs, colour, read_len, read_words, n_contigs, rg_len, dq, ztags, extra;
                   const uint32_t* reads; const uint8_t* initbp; const uint8_t* names; const unsigned long long* name_off; const uint8_t* seqs; const uint8_t* quals;
                   const uint8_t* cigar; const uint8_t* edit; const uint8_t* qralign; const uint8_t* post_quals; const uint8_t* cnames; const uint32_t* cname_off;
                   uint32_t* lens; const unsigned long long* offs; uint8_t* out; };
int gm_launch_sam_records(const GmSamArgs& args, int write, hipStream_t stream);      // write = 0: the sizing launch; 1: the bytes
