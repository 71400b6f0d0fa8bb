/*
 * gmapper_hip.h -- C ABI of libgmapper_hip.so: an MI355X (gfx950) implementation of the
 * SHRiMP2 gmapper hot path (spaced-seed lookup + Smith-Waterman extension).
 *
 * Plain C types only (pointers + sizes); no torch / HIP types cross this boundary.
 * All "ref:" citations are file:line in compbio-UofT/shrimp (SHRiMP 2.2.3).
 *
 * Seams replaced:
 *   S1  sw_vector_setup / sw_vector / sw_vector_stats      ref: common/sw-vector.h:1-6, common/sw-vector.c:388-515
 *       sw_gapless_setup / sw_gapless / sw_gapless_stats   ref: common/sw-gapless.h:11-14, common/sw-gapless.c:29-117
 *   S2  sw_full_ls_setup / sw_full_ls                       ref: common/sw-full-ls.h, common/sw-full-ls.c:568-683
 *   S4  handle_read (per-read pipeline -> SAM text)        ref: gmapper/mapping.h:23, gmapper/mapping.c:1773-1868
 *   S5  load_genome (index build) + its globals            ref: gmapper/genome.h:23-32, gmapper/genome.c:1012-1182
 * The reference calls S1/S2/S4 once per window / per read from an OpenMP thread; a GPU needs
 * batches, so every seam has a batch form; the single-call forms keep the reference's exact
 * parameter lists (for drop-in linking) and are thin wrappers over a batch of one.
 *
 * Errors: integer return codes (0 = ok, <0 = GM_E_*); nothing throws across the ABI.
 * Threading: one host thread per gm_session; a session owns its HIP streams on one device and its launch scratch.  TWO mapping calls (of two sessions) may be in
 * flight on the SAME device -- a third waits for one of them to return; sessions on different devices run side by side.  The unpaired file entry
 * uses this itself: a file of more than one chunk is mapped by the session and a twin of it (same index and parameters, made on first use, freed with the session) on two
 * threads, so that one chunk's tail runs under the next chunk's lookups (GM_FILE_ONE_SESSION=1 in the environment keeps it to the one session).
 */
#ifndef GMAPPER_HIP_H
#define GMAPPER_HIP_H

#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GM_OK            0
#define GM_E_NODEVICE   -1   /* no HIP device / HIP runtime error (message via gm_last_error) */
#define GM_E_ARG        -2   /* invalid argument */
#define GM_E_NOTSETUP   -3   /* call before *_setup (the reference abort()s here, sw-vector.c:463) */
#define GM_E_RANGE      -4   /* match*qrlen >= 32768 (ref: sw-vector.c:393-398, exit(1) there); more than GM_MAX_CONTIGS contigs */
#define GM_E_OVERFLOW   -5   /* a per-read candidate list exceeded every configured capacity */
#define GM_E_NOMEM      -6

const char *gm_last_error(void);
/* sizeof of the structs that cross the ABI, for bindings to check their mirrors against: which = 0 gm_params_t, 1 gm_pair_opts_t, 2 gm_map_stats_t, 3 gm_merge_options_t,
 * 4 gm_sw_full_rec_t, 5 gm_post_rec_t (-1 for any other value) */
int gm_abi_sizeof(int which);
/* number of visible HIP devices (0 when none); never initialises more than the runtime */
int gm_device_count(void);

/* ---- scoring / pipeline parameters = the reference's globals (ref: gmapper/gmapper.h:47-127) ---- */
typedef struct gm_params {
  int match_score, mismatch_score;             /* ref: gmapper-defaults.h:45-46   (10, -15) */
  int a_gap_open_score, a_gap_extend_score;    /* ref: gmapper-defaults.h:47,49   (-33, -7)  gap along the genome */
  int b_gap_open_score, b_gap_extend_score;    /* ref: gmapper-defaults.h:48,50   (-33, -3)  gap along the read   */
  double window_len;                           /* ref: gmapper-defaults.h:31  140.0 (%; negative = absolute).  A window longer than pass 2 has LDS for beside the call's
                                                  reads (3 140 columns beside 100 bases in letter space) is refused with GM_E_RANGE before anything is uploaded */
  double window_overlap;                       /* ref: gmapper-defaults.h:32   90.0 */
  double window_gen_threshold;                 /* ref: gmapper-defaults.h:62   55.0 */
  double sw_vect_threshold, sw_full_threshold; /* ref: gmapper-defaults.h:67-68; LS: vect := full (gmapper.c:2456-2458) */
  int match_mode;                              /* ref: gmapper-defaults.h:34    2 */
  int num_outputs, num_tmp_outputs;            /* ref: gmapper.h:53-55         10, 30 */
  int anchor_width;                            /* ref: gmapper-defaults.h:36    8; 0 .. 99, or -1: no anchor band -- the threshold band in every full alignment
                                                  (sw-full-ls.c:175-192, sw-full-cs.c:285-301); anything else: GM_E_ARG, as the reference exits (gmapper.c:2014-2016) */
  int region_bits, region_overlap;             /* ref: gmapper-defaults.h:22-23 11, 50 */
  uint32_t list_cutoff;                        /* 0 = automatic (ref: gmapper.c:2811-2837) */
  int hash_filter_calls;                       /* ref: gmapper-defaults.h:17 true; 0 == -Z */
  int tiebreak_rev;                            /* Tflag, ref: gmapper.h:87 true */
  int sam_unaligned;                           /* ref: gmapper.h:185 false */
  int longest_read_len;                        /* ref: gmapper-defaults.h:72 1000 */
  int strata;                                  /* --strata: only the best-scoring hits (ref: gmapper.h:85, mapping.c:1706-1712,2268-2274) false */
  int max_alignments;                          /* --max-alignments: drop reads with more final hits (ref: gmapper.h:54, mapping.c:1713-1722) 0 = all */
  int colour_space;                            /* shrimp_mode == MODE_COLOUR_SPACE, i.e. the gmapper-cs binary (ref: util.c:28-38) 0 */
  int crossover_score;                         /* ref: gmapper-defaults.h:54  -20; the vector filter's mismatch is match + crossover (gmapper.c:2935) */
  int indel_taboo_len;                         /* ref: gmapper.h:57  0 */
  double pr_xover;                             /* ref: gmapper.h:119  0.03: fixes score_alpha in colour space (gmapper.c:2557-2563) */
  int local_alignment;                         /* --local, i.e. Gflag off (ref: gmapper.c:2303-2305): sw_full_ls in local mode (soft clips); mapping qualities
                                                  are then unavailable (gmapper.c:2325-2328): MAPQ 255, no Z0-Z6 tags.  Letter space and colour space, unpaired and paired (sw_full_cs with
                                                  local_alignment, ref: sw-full-cs.c:199-203,315,439-552; no post_sw then, mapping.c:1648; with csfastq quality values too, unpaired and paired).  0 */
  int ungapped;                                /* -U (gapless_sw): pass 1 scores windows with sw_gapless (ref: sw-gapless.c:57-117), every anchor opens a window
                                                  (mapping.c:1095,1154).  As the reference's -U does, also set anchor_width 0, both gap opens -255 and
                                                  hash_filter_calls 0; requires local_alignment (gmapper.c:2330-2333).  In colour space sw_gapless runs on the contig's colour translation with the
                                                  read's first colour forced against the primer (sw-gapless.c:84-94).  0 */
  int hash_seeds;                              /* -H (Hflag): lists are keyed by kmer_to_mapidx_hash -- 4^12 lists per seed whatever its weight, so seeds
                                                  heavier than 14 are allowed (ref: gmapper.h:309-336, seeds.c:83-102,132-136).  An index property.  0 */
  int output_format;                           /* 0: SAM (-E, the binary's default); 1: --shrimp-format, one line per mapping -- readname contigname strand
                                                  contigstart contigend readstart readend readlength score editstring (ref: common/output.c:280-352 output_normal,
                                                  :36-115 alignment_edit_string); 2: -P/--pretty, each line followed by the aligned G: / R: (/ T:) rows
                                                  (ref: common/output.c:118-262 output_pretty).  Unaligned reads print nothing in 1 / 2; in paired mode every mate has its
                                                  own line under its own name, and the unmapped mate of a half-paired mapping prints ">name" (gmapper/output.c:292-294).  0 */
  int print_read_seq;                          /* -R: the read's sequence as a last column of the SHRiMP-format line (ref: gmapper.h Rflag, output.c:310-313)  0 */
  int strand_only;                             /* 1: -F / --positive (only the read as given), 2: -C / --negative (only its reverse complement): the other strand gets no
                                                  anchor list (ref: mapping.c:879-880, gmapper.c:1979-1992).  Unpaired only -- paired mode maps both strands, as the
                                                  reference does after its warning (gmapper.c:2448-2451).  0 */
  /* output policy of read_output / readpair_output (ref: output.c:955-1008,1070-1291; gmapper.c:2252-2268) */
  int single_best_mapping;                     /* --single-best-mapping: only the mapping with the highest quality -- unpaired: the first such; paired: the best unpaired
                                                  mapping of each mate and the pair that holds the best paired one (with all_contigs: ONE record pair over all classes;
                                                  an unpaired winner is joined with the other mate's best unpaired mapping into an IMPROPER pair when both qualities
                                                  reach 10, unless no_improper_mappings).  Without mapping qualities (--local, no_mapping_qualities) it does nothing, as in the reference.  0 */
  int all_contigs;                             /* --all-contigs: no Z0-Z6 tags (ref: output.c:691); changes what single_best_mapping selects.  0 */
  int no_mapping_qualities;                    /* --no-mapping-qualities: MAPQ 255, no Z tags, no post_sw (colour space prints sw_full_cs's own strings), as --local implies.  0 */
  int no_improper_mappings;                    /* --no-improper-mappings  0 */
  /* optional tail of every SAM record (ref: output.c:452-465,729-756) */
  int extra_sam_fields;                        /* --extra-sam-fields: ZM:i matches, ZR:i window-generation score, ZV:i vector score, ZH:i full SW score, ZE:Z edit string
                                                  (alignment_edit_string, reversed for mappings on the reverse strand) on mapped records.  0.
                                                  UNTESTED corner: a read or window letter outside A/C/G/T on a reverse-strand mapping -- the reference's
                                                  reverse_alignment_edit_string never returns on such a letter (its loop index stops advancing, output.c:164-220), so no golden can
                                                  exist; this library passes the letter through unchanged */
  int sam_r2;                                  /* --sam-r2 (paired mode only): R2:Z (colour space: X2:Z) = the mate's sequence as given.  0 */
  char read_group[64];                         /* --read-group: RG:Z:<name> on every record ("" = none; the @RG header line is the caller's, as the @SQ lines are) */
  /* the read loop's preprocessing, applied by the file entry points to every read before it is mapped (ref: gmapper.c:262-284 trim_read, :427-472, :495-521) */
  int trim_front, trim_end;                    /* --trim-front / --trim-end: that many characters off either end of the sequence (and its quality string).  0, 0.
                                                  trim_front is refused in colour space, as the binary refuses it (gmapper.c:2134-2137) */
  int trim_first, trim_second;                 /* paired mode: which mates are trimmed (--trim-first: 1, 0; --trim-second: 0, 1).  1, 1 -- but trimming the FIRST mate is
                                                  refused: the reference trims it after packing it (gmapper.c:427-438,474-475) and prints records that contradict themselves */
  int trim_illumina;                           /* --trim-illumina (letter space, FASTQ): a tail of 'B' quality values is cut off with its bases.  0 */
  int min_avg_qv;                              /* --min-avg-qv: a read with quality values whose integer mean (sum / length) is below this gets no record at all (ref: gmapper.h:81,
                                                  gmapper.c:456-462,491-498).  10; < 0: none */
  int ignore_qvs;                              /* --ignore-qvs: the quality values are printed but not used -- no min_avg_qv, no range check; colour space: the global crossover
                                                  score and error rates (ref: gmapper.c:532,2962).  0 */
  int no_qv_check;                             /* --no-qv-check: a quality value outside [-10, 50] is NOT an error (ref: gmapper.c:463-472: the binary exits there).  0 */
} gm_params_t;

void gm_params_default(gm_params_t *p);        /* letter-space defaults of the reference binary (gmapper-ls) */
void gm_params_default_cs(gm_params_t *p);     /* colour-space defaults (gmapper-cs): mismatch -24, vector threshold 47%, ref: gmapper.c:1748-1755 */

/* ---------------------------------------------------------------------------------------------
 * S5: index.  Replaces load_genome() and the globals genomemap / genomemap_len / genome_contigs /
 * contig_offsets / genome_len (ref: gmapper/genome.c:1012-1182, gmapper/gmapper.h:262-275).
 * contigs[c] is the reference's own 4-bit bitfield (8 bases per uint32, base i in nibble i%8 of
 * word i/8; ref: common/util.h:41, common/fasta.c:609-673).  seeds are "0/1" strings
 * (ref: gmapper/seeds.c:9-43); n_seeds == 0 selects the binary's default 3 seeds of weight 12
 * (ref: gmapper-defaults.h:212-227).  The index is built on the device (histogram-free radix
 * sort of (k-mer, position) pairs) and stays resident in HBM.
 * Limits of a seed set: a span of 32 or less (the k-mer key is gathered through a 64-bit mask, two bits a
 * position), a weight of 14 or less without hash_seeds (any weight with it), at most GM_MAX_SEEDS = 16 seeds,
 * only '0' and '1', at least one '1'.  A set beyond a limit is refused by gm_index_build, gm_index_build_fasta
 * and gm_index_load with GM_E_ARG; gm_last_error() names the seed and the limit.  Open against the reference:
 * it accepts spans up to 64 (MAX_SEED_SPAN, ref: gmapper-definitions.h) -- spans of 33 to 64 are refused
 * here, not mapped.  Held to the reference's output up to span 32, weight 14 and 16 seeds
 * (tests/test_seed_sets.py).
 * ------------------------------------------------------------------------------------------- */
typedef struct gm_index gm_index_t;
/* The most contigs an index holds.  A window carries its contig number in 16 bits (the anchor kernel's aux word and window sort key, the hit record) where the
 * reference's cn is an int, so gm_index_build, gm_index_build_fasta and gm_index_load refuse a genome of more contigs before they allocate anything that outlives
 * the call: GM_E_RANGE, gm_last_error() names the count and this limit.  A contig number is never narrowed in silence. */
#define GM_MAX_CONTIGS 65536
int  gm_index_build(gm_index_t **out, int device, int n_contigs, const uint32_t *const *contigs,
                    const uint32_t *contig_len, const char *const *contig_names,
                    int n_seeds, const char *const *seeds, const gm_params_t *params);
void gm_index_free(gm_index_t *ix);
/* S5 as the reference has it: load_genome(files, nfiles), ref: gmapper/genome.c:1012-1182.  FASTA, plain or gzip, one or more contigs a file, files in the
 * given order; the text is packed into the resident bitfield on the device, then the index is built as by gm_index_build -- the two give the same index for
 * the same contigs.  The genome is read in letter space, also for a colour-space index (genome.c:1053).  The reference's reader (common/fasta.c:316-553):
 *   - a line whose first character is '>' starts a contig; its name is the header cut as the read files' names are cut (after the '>': up to the first tab,
 *     trimmed, cut at the first blank -- so the tab test of genome.c:1079 on the name cannot fire); a line whose first character is '#' is skipped wherever
 *     it stands; every other line is sequence; the last line may lack its '\n'; an empty line inside a sequence adds nothing (as in the reference);
 *   - letters of either case A C G T U M R W S Y K V H D B N -> 0..15, X and '.' -> 15 (gm_sequence_to_bitfield's letter-space table); any other byte of a
 *     sequence line ('\r', blank, tab, digit, a '>' that is not at a line start, ...) fails the call with GM_E_ARG and a message that names the file, the
 *     contig and the byte offset (the reference: "invalid sequence; tag: [..]", genome.c:1094-1097);
 *   - a genome of 2^32 bases or more, or of more than GM_MAX_CONTIGS contigs, fails as in gm_index_build.
 * Deliberate divergence: a file that does not start with a '>' line (after '#' lines), a header with no name and no sequence before the next header or the
 * end, a header line with nothing after the '>', and an unreadable or empty file return GM_E_ARG.  The reference prints a message and silently goes on with
 * the contigs it has so far.  Lines longer than the reference's 8 MiB line buffer are out of scope.  gm_last_error() names the file. */
int  gm_index_build_fasta(gm_index_t **out, int device, int n_files, const char *const *paths,
                          int n_seeds, const char *const *seeds, const gm_params_t *params);
/* names and lengths of the contigs of an index (for a caller that did not parse the genome itself); *name lives as long as the index */
int  gm_index_n_contigs(const gm_index_t *ix);
int  gm_index_contig(const gm_index_t *ix, int c, const char **name, uint32_t *len);
/* the header gmapper prints before its records (ref: gmapper.c:2980-3008): @HD VN:1.0 SO:unsorted, one @SQ per contig, @RG ID/SM when rg_id is given,
 * @PG ID:gmapper VN:2.2.3 CL:<command_line> when command_line is given.  *text: gm_free */
int  gm_sam_header(const gm_index_t *ix, const char *rg_id, const char *rg_sample, const char *command_line, char **text, size_t *len);
/* how long gm_index_build_fasta took for this index: seconds until the genome bitfield and the contig table were resident (where the device build of the
 * lists starts), and seconds of the whole call; GM_E_ARG for an index made another way */
int  gm_index_build_timing(const gm_index_t *ix, double *to_bitfield_s, double *total_s);
/* The reference's on-disk index ("-S prefix" / "-L prefix": <prefix>.genome + <prefix>.seed.<n>, gzip; ref: gmapper/genome.c:15-270,
 * 670-831).  gm_index_save writes files stock gmapper can load; gm_index_load reads files stock gmapper wrote (letter or colour space, with or without -H: the mode and Hflag words of the files must match params)
 * and uploads them -- the lists are taken as they are, only the per-slab directory is derived on the device. */
int  gm_index_save(const gm_index_t *ix, const char *prefix);
int  gm_index_load(gm_index_t **out, int device, const char *prefix, const gm_params_t *params);
/* introspection (mirrors the reference's globals) */
uint32_t gm_index_list_cutoff(const gm_index_t *ix);
uint64_t gm_index_bytes(const gm_index_t *ix);
int      gm_index_n_slabs(const gm_index_t *ix);
int      gm_index_has_buckets(const gm_index_t *ix);   /* 1 when the 64-byte bucket layout is resident (small genomes) */
/* genomemap_len[sn][mapidx] / genomemap[sn][mapidx][0..len) copied back to the host (tests) */
int gm_index_get_list(const gm_index_t *ix, int sn, uint32_t mapidx, uint32_t *len, uint32_t *positions, uint32_t cap);
/* raw device pointers + sizes of the resident arrays, for the single RCCL broadcast at start-up
 * (SURVEY.md section 8(e)); kind: 0 genome, 1+3*sn directory of seed sn, 2+3*sn positions of seed sn,
 * 3+3*sn the 64-byte buckets of seed sn (bytes == 0 when that layout is not resident), 1+3*n_seeds the colour translation
 * of the genome (bytes == 0 in letter space); larger kinds return GM_E_ARG */
int gm_index_device_array(const gm_index_t *ix, int kind, void **dev_ptr, uint64_t *bytes);
/* allocate an index with the same shape (from the metadata blob of a built index) so that a
 * non-root rank can receive the arrays; meta is host memory */
int gm_index_meta(const gm_index_t *ix, void *meta, uint64_t *meta_bytes);
int gm_index_alloc_like(gm_index_t **out, int device, const void *meta, uint64_t meta_bytes);

/* ---------------------------------------------------------------------------------------------
 * S1: vector Smith-Waterman filter (score only).  ref: common/sw-vector.c:388-515
 * Same parameter lists as the reference (penalties passed negative).  State is per calling
 * thread, as in the reference (threadprivate).  With use_colours the read's first colour is compared with lstocs(genome_ls[j], initbp)
 * (see the colour-space block below), with is_rna a U in the genome letters counting as T there (ref: sw-vector.c:129,289; util.h:182-205).
 * ------------------------------------------------------------------------------------------- */
int sw_vector_setup(int dblen, int qrlen, int a_gap_open, int a_gap_ext, int b_gap_open, int b_gap_ext,
                    int match, int mismatch, int use_colours, bool reset_stats);
int sw_vector(uint32_t *genome, int goff, int glen, uint32_t *read, int rlen,
              uint32_t *genome_ls, int initbp, bool is_rna);
void sw_vector_stats(uint64_t *invocs, uint64_t *cells, double *secs);
int sw_vector_cleanup(void);
/* batch form: n independent windows; genome/read are host bitfields, words are uploaded once.
 * g_off[i] indexes into `genome` (one shared bitfield), reads[i*read_words .. ) holds read i. */
int gm_sw_vector_batch(int n, const uint32_t *genome, uint64_t genome_words, const int64_t *g_off, const int *glen,
                       const uint32_t *reads, int read_words, const int *rlen, int *scores);
/* the same with pass 1's early stop (unpaired reads, ref: mapping.c:1332-1335 only compares the score with the threshold): a window whose remaining
 * cells can no longer lift any alignment to `threshold` stops there; stopped[i] = 1 and scores[i] = the best score up to that point, which like the
 * final one is below `threshold`.  stopped[i] = 0: scores[i] is the value gm_sw_vector_batch returns.  Letter space, reads up to 128 bases stop early. */
int gm_sw_vector_batch_bounded(int n, const uint32_t *genome, uint64_t genome_words, const int64_t *g_off, const int *glen,
                               const uint32_t *reads, int read_words, const int *rlen, int threshold, int *scores, uint8_t *stopped);

/* S1, ungapped form (-U / gapless_sw): the best ungapped segment on the diagonal of `genome` (glen positions from its first word) through
 * (g_idx, r_idx).  ref: common/sw-gapless.h:11-14, sw-gapless.c:29-117; f1_setup / f1_run call these instead of sw_vector when gapless_sw is set
 * (f1-wrapper.h:66-68,122-125).  Colour space: genome = colours, genome_ls = the letters, and a diagonal that starts at the read's first colour
 * compares it with lstocs(genome_ls[g], init_bp) (:84-94).  sw_gapless_stats: invocations, cells (+= rlen per call, :111), time inside (here ns). */
int  sw_gapless_setup(int match, int mismatch, bool reset_stats);
int  sw_gapless(uint32_t *genome, int glen, uint32_t *read, int rlen, int g_idx, int r_idx, uint32_t *genome_ls, int init_bp, bool is_rna);
void sw_gapless_stats(uint64_t *invocs, uint64_t *cells, uint64_t *ticks);
/* batch form: call i's bitfield starts at word genome_woff[i] of `genome` (and of `genome_ls`, which is NULL in letter space; initbp may then be NULL) */
int gm_sw_gapless_batch(int n, const uint32_t *genome, const uint32_t *genome_ls, uint64_t genome_words, const int64_t *genome_woff, const int *glen,
                        const uint32_t *reads, int read_words, const int *rlen, const int *g_idx, const int *r_idx, const int *initbp, int *scores);

/* ---------------------------------------------------------------------------------------------
 * S2: full Smith-Waterman with traceback, letter space.  ref: common/sw-full-ls.c:568-683
 * struct layouts follow the reference (ref: common/sw-full-common.h:13-48, gmapper-definitions.h:66-74)
 * for the fields this path fills; dbalign/qralign are malloc()ed and owned by the caller,
 * as with the reference's xstrdup (ref: sw-full-ls.c:676-677).  Both alignment modes: local_alignment = 0 (global in the read, gmapper's
 * default) and 1 (--local: floored states, and when the best score in the anchor band is not maxscore a second run over the band
 * the threshold allows, :395-398); anchors = one box as gmapper passes it, or NULL (that threshold band, :179-192).
 * ------------------------------------------------------------------------------------------- */
struct gm_anchor { long long x, y; int length, width, weight, cn, score; };
struct gm_sw_full_results {                    /* field for field struct sw_full_results (ref: common/sw-full-common.h:13-48) */
  int read_start, rmapped, genome_start, gmapped, matches, mismatches, insertions, deletions, score;
  int posterior_score, pct_posterior_score;   /* filled by hit_run_post_sw in the reference, untouched here */
  char *dbalign, *qralign, *qual;
  double posterior;
  int mqv; double z0, z1, z2, z3, pr_top_random_at_location, pr_missed_mp, insert_size_denom;
  int crossovers;                             /* colour space only */
  bool dup, in_use;
};
int sw_full_ls_setup(int dblen, int qrlen, int a_gap_open, int a_gap_ext, int b_gap_open, int b_gap_ext,
                     int match, int mismatch, bool reset_stats, int anchor_width);
void sw_full_ls(uint32_t *genome, int goff, int glen, uint32_t *read, int rlen, int threshscore, int maxscore,
                struct gm_sw_full_results *sfr, bool revcmpl, struct gm_anchor *anchors, int anchors_cnt,
                int local_alignment);
int sw_full_ls_cleanup(void);
void sw_full_ls_stats(uint64_t *invocs, uint64_t *cells, double *secs);   /* ref: common/sw-full-ls.h:11, called from gmapper.c:745 */

/* ---------------------------------------------------------------------------------------------
 * S1/S2 in colour space.  sw_vector_setup(..., use_colours = 1, ...) makes sw_vector() compare the read's first colour with
 * lstocs(genome_ls[j], initbp) (ref: common/sw-vector.c:112-146); `mismatch` is then match + crossover (ref: gmapper.c:2935).
 * sw_full_cs: four letter-space translations of the colour read, 3-state affine DP in four layers with crossovers between
 * layers on the NW and N transitions, traceback with crossover marks (lower-case in qralign), ref: common/sw-full-cs.c:249-1236.
 * Both modes (local_alignment 0 / 1, ref: sw-full-cs.c:199-203,315,439-552) and one anchor box, as gmapper calls it (ref: mapping.c:375-379).  crossover_score: NULL (the
 * global penalty everywhere) or rlen per-position penalties, what gmapper passes for every read with quality values (ref: mapping.c:375-379, gmapper.c:532-544, used per row
 * at sw-full-cs.c:312-322); the device keeps them in 8 bits (gmapper clamps them to [2 * global, -1]).  An argument combination that is not implemented (several anchors, a
 * score outside [-128, 127]) is refused LOUDLY -- the reason on stderr and in gm_last_error(), sfr->score = 0 -- never answered as if the window held no alignment.
 * is_rna (all three seams; gmapper passes genome_is_rna, the flag of the LAST contig it read: genome.c:1063-1064): lstocs reads a U as T, cstols takes a U as T and hands back U
 * where it would hand back T (util.h:157-205) -- in sw_vector's and sw_gapless's first-colour comparison and in the four letter translations of sw_full_cs.  In letter space the
 * argument changes nothing (sw-vector.c uses it in the colour-space row only).
 * RNA in the batch entries (gm_map_reads* / gm_map_pairs*): a contig with uracil and no thymine is an RNA contig (fasta.c:528-542) -- its reverse complement holds U for A and its
 * colour translation reads U as T (genome.c:1107-1118); the last contig's flag is what the SW stages get, as in the reference; a letter-space read with U and no T is
 * reverse-complemented with U for A (gmapper.c:487).  The read's flag is taken from the letters the device gets, i.e. AFTER the file entries' trimming (the reference takes it
 * from the file's sequence before trimming: the two differ only for a read that holds both U and T and loses every T to the trim).
 * ------------------------------------------------------------------------------------------- */
int sw_full_cs_setup(int dblen, int qrlen, int a_gap_open, int a_gap_ext, int b_gap_open, int b_gap_ext,
                     int match, int mismatch, int global_xover_penalty, bool reset_stats, int anchor_width, int indel_taboo_len);
void sw_full_cs(uint32_t *genome_ls, int goff, int glen, uint32_t *read, int rlen, int initbp, int threshscore,
                struct gm_sw_full_results *sfr, bool revcmpl, bool is_rna, struct gm_anchor *anchors, int anchors_cnt,
                int local_alignment, int *crossover_score);
int sw_full_cs_cleanup(void);
void sw_full_cs_stats(uint64_t *invocs, uint64_t *cells, double *secs);   /* ref: common/sw-full-cs.h:9, called from gmapper.c:742 */

/* ---------------------------------------------------------------------------------------------
 * S3: post_sw, the colour-space posterior of one alignment (16-state forward-backward over the aligned columns, doubles through libm in
 * the reference's operation order -- a host routine here as in the reference).  ref: common/sw-post.h:6-9, sw-post.c:364-758; called by
 * hit_run_post_sw (gmapper/mapping.c:1609-1625).  post_sw re-calls sfr->qralign in place, recounts matches / mismatches / crossovers,
 * mallocs sfr->qual (base qualities, PHRED+33) and fills sfr->posterior.  State is per calling thread.  Returns follow the reference (1).
 * The batch form, gm_post_sw_batch, is declared behind the S2 batch entries whose records it takes.
 * ------------------------------------------------------------------------------------------- */
int  post_sw_setup(int max_len, double pr_snp, double pr_xover, double pr_del_open, double pr_del_extend, double pr_ins_open, double pr_ins_extend,
                   bool use_read_qvs, bool use_sanger_qvs, int qual_vector_offset, int qual_delta, bool reset_stats);
void post_sw(uint32_t *read, int initbp, char *qual, struct gm_sw_full_results *sfr);
int  post_sw_cleanup(void);
int  post_sw_stats(uint64_t *invocs, uint64_t *cells, double *secs);
/* batch form of the colour-space vector filter: as gm_sw_vector_batch plus the letter-space genome and one initial base per read */
int gm_sw_vector_batch_cs(int n, const uint32_t *genome_cs, const uint32_t *genome_ls, uint64_t genome_words, const int64_t *g_off,
                          const int *glen, const uint32_t *reads, int read_words, const int *rlen, const int *initbp, int *scores);

/* ---------------------------------------------------------------------------------------------
 * S2, batch forms: n independent sw_full_ls / sw_full_cs calls in one go, on this thread's sw_full_ls_setup / sw_full_cs_setup state (without it: GM_E_NOTSETUP).
 * Input layout of gm_sw_vector_batch: one shared genome bitfield, g_off[i] a base offset into it, reads[i * read_words ..) read i.  One call makes a fixed
 * number of device allocations, copies and kernel launches whatever n is (the back-pointer scratch belongs to the resident waves, not to the items).
 *   anchors       n boxes (x, y, length, width as sw_full_ls / sw_full_cs take them), or NULL.  Letter space: NULL, or an item whose box has length <= 0, runs over the
 *                 band the threshold allows (the single seam's anchors == NULL).  Colour space needs a box for every item, as the single seam does.
 *   revcmpl       n flags or NULL (all 0);  threshscore n;  maxscore n (letter space, read in local mode only; may be NULL otherwise)
 *   crossover_scores  colour space: NULL (the global penalty everywhere) or n rows of xover_stride >= rlen[i] per-position scores, the single seam's crossover_score[]
 * Output: recs[i] for every item.  status 0: answered, with the values the single seam leaves in struct gm_sw_full_results (letter space, score 0: rmapped = gmapped = 1,
 * genome_start = g_off[i]; colour space below threshscore: all 0).  status < 0 (GM_E_*): the device path cannot take this item -- sizes beyond the setup's, a window
 * outside the bitfield, a colour-space box missing, a crossover score outside [-128, 127], a window that does not fit LDS beside the longest read of the call (colour space: 48 bytes a column) -- it is
 * refused with score 0, the reason of the last such item is in gm_last_error(), and the other items of the call are answered all the same.
 * *ops: one buffer of *ops_len bytes (gm_free), item i's edit operations at ops[ops_off .. ops_off + n_ops) in alignment order:
 *   letter space   'M' match or mismatch, 'I' insertion (a genome letter against a gap in the read), 'D' deletion (a read letter against a gap in the genome)
 *   colour space   low nibble 1 = insertion; 2..5 = deletion, 6..9 = match / mismatch, the read letter taken from letter translation 0..3 of the colour read
 *                  (translation k starts from primer letter (initbp + k) % 4: the base called in that column); bit 7 = a crossover at this column (lower case in qralign)
 * gm_sw_full_batch_strings: dbalign / qralign of one item exactly as the single seams return them, rebuilt on the host from the item's record, the ops buffer and the
 * caller's own bitfields (genome: the shared one, genome_len positions; read: read i's words, rlen positions; ops_len: *ops_len of the batch call); both malloc()ed, gm_free.
 * A record whose operations or alignment do not lie inside those lengths is refused with GM_E_ARG before anything is read through it.  Letter space without alignment: two empty strings; colour space: two NULLs.
 * ------------------------------------------------------------------------------------------- */
typedef struct gm_sw_full_rec {
  int score, read_start, rmapped, gmapped, matches, mismatches, insertions, deletions, crossovers /* colour space only, else 0 */;
  int status;                            /* 0 ok; < 0: this item was refused (GM_E_*), score = 0 */
  int64_t genome_start;                  /* counted from the start of `genome`, i.e. includes g_off[i] */
  uint64_t ops_off; uint32_t n_ops;      /* this item's edit operations: ops[ops_off .. ops_off + n_ops) */
} gm_sw_full_rec_t;
int gm_sw_full_ls_batch(int n, const uint32_t *genome, uint64_t genome_words, const int64_t *g_off, const int *glen,
                        const uint32_t *reads, int read_words, const int *rlen, const struct gm_anchor *anchors, const uint8_t *revcmpl,
                        const int *threshscore, const int *maxscore, int local_alignment, gm_sw_full_rec_t *recs, uint8_t **ops, uint64_t *ops_len);
int gm_sw_full_cs_batch(int n, const uint32_t *genome_ls, uint64_t genome_words, const int64_t *g_off, const int *glen,
                        const uint32_t *reads, int read_words, const int *rlen, const uint8_t *initbp, const struct gm_anchor *anchors, const uint8_t *revcmpl,
                        const int *threshscore, const int *crossover_scores, int xover_stride, int is_rna, int local_alignment,
                        gm_sw_full_rec_t *recs, uint8_t **ops, uint64_t *ops_len);
int gm_sw_full_batch_strings(int colour_space, const gm_sw_full_rec_t *rec, const uint8_t *ops, uint64_t ops_len, const uint32_t *genome, uint64_t genome_len,
                             const uint32_t *read, int rlen, int initbp, int is_rna, char **dbalign, char **qralign);

/* ---------------------------------------------------------------------------------------------
 * S3, batch form: post_sw of n alignments of ONE gm_sw_full_cs_batch call, on this thread's post_sw_setup state (without it: GM_E_NOTSETUP, where the single seam
 * aborts).  Pass 2 of a colour-space chunk is then two calls -- gm_sw_full_cs_batch, gm_post_sw_batch -- instead of 2 n.
 * Input: recs / ops / ops_len as that call returned them, and the arrays it was given (the shared letter-space bitfield, the reads, rlen, initbp, is_rna).
 *   quals   NULL, or n QV strings in the file's characters; used only when post_sw_setup got use_read_qvs (with its qual_vector_offset and qual_delta), exactly as
 *           the single seam uses its `qual` argument.
 * Output: post[i] for every item; *qralign_out: one buffer of ops_len bytes (gm_free), item i's re-called qralign -- exactly what post_sw leaves in sfr->qralign, upper
 * and lower case, '-' in a column without a read position, not NUL-terminated -- at the place of its operations, [recs[i].ops_off, + n_ops); *quals_out / *quals_len:
 * the items' sfr->qual strings (base qualities, PHRED+33) end to end (gm_free), item i's at [qual_off, + qual_len).  dbalign is untouched by post_sw: a caller who
 * wants it still uses gm_sw_full_batch_strings.
 * Items: recs[i].status < 0 comes back with the same status; score <= 0 (no alignment) is answered with status 0, qual_len 0, posterior 0.  A record that does not
 * lie inside what the caller holds -- operations outside ops_len, an alignment that runs past the genome or the read, an operation byte that is none of the encoding,
 * an alignment longer than post_sw_setup's max_len (or than 59 918 read positions, what one wave's column scratch holds), a QV string that is missing or shorter than
 * qual_vector_offset + rlen[i] while QVs are in use -- is refused on the host with GM_E_ARG before anything is uploaded (the checks of gm_sw_full_batch_strings); the
 * reason of the last refused item is in gm_last_error(), its neighbours are answered.  n <= 0: GM_OK, nothing is written.
 * One call makes a fixed number of device allocations, copies and launches whatever n is: the kernel's column scratch (140 bytes a column) belongs to its thread slots, is
 * sized by the longest alignment of a launch and capped at 512 MiB (fewer threads then); items of very different lengths go into at most three launches by length.
 * Exactness: matches / mismatches / crossovers, the qralign slice and the qual slice are EQUAL to the single seam's for every item.  The device differs from the host
 * routine in exp / log only (ocml against glibc); an item where those last bits could decide an output byte -- a letter call between two posteriors within 1e-9 of each
 * other, a base quality within 1e-7 of its truncation boundary or at a cut-off -- is answered by the library's host routine instead and marked by_host = 1 (its posterior
 * then carries the single seam's bits).  For by_host = 0 the posterior is within 1e-9 relative of the single seam's; the largest difference seen from the reference's over the
 * 1 833 records of tests/golden/sw_kat_post.txt.gz on an MI355X: 5.4e-16 without QVs, 4.2e-16 with QVs (profiles/r07a_post_sw_batch_error.json).
 * post_sw_stats counts an answered item with an alignment like a single call: invocs += 1, cells += 16 x read positions.
 * gm_post_sw_batch_last_plan is a DIAGNOSTIC hook, not part of the stable surface (it may change or go with the launch planning; the tests use it to see that thread
 * slots were reused): how the last call on this thread was laid out -- returns its number of launches (0: nothing reached the device) and, for launch `launch`, the
 * items it took, its thread slots and the columns of scratch a slot had (the longest alignment of the launch).  items > threads: slots served several items in turn.
 * ------------------------------------------------------------------------------------------- */
typedef struct gm_post_rec {
  double   posterior;                          /* what post_sw leaves in sfr->posterior */
  int      matches, mismatches, crossovers;    /* recounted, as post_sw leaves them */
  int      status;                             /* 0 answered; < 0 (GM_E_*): this item was refused */
  int      by_host;                            /* 1: the host routine answered this item (see "Exactness") */
  uint32_t qual_len;                           /* read positions in the alignment = strlen(sfr->qual) */
  uint64_t qual_off;                           /* this item's base qualities: quals_out[qual_off .. qual_off + qual_len) */
} gm_post_rec_t;
int gm_post_sw_batch(int n, const gm_sw_full_rec_t *recs, const uint8_t *ops, uint64_t ops_len,
                     const uint32_t *genome_ls, uint64_t genome_words,
                     const uint32_t *reads, int read_words, const int *rlen, const uint8_t *initbp,
                     const char *const *quals, int is_rna,
                     gm_post_rec_t *post, char **qralign_out, char **quals_out, uint64_t *quals_len);
int gm_post_sw_batch_last_plan(int launch, int *items, int *threads, int *columns);   /* diagnostic, see above */

/* ---------------------------------------------------------------------------------------------
 * The text of a batch's alignments: dbalign / qralign, the CIGAR and the edit string of every record of ONE gm_sw_full_ls_batch / gm_sw_full_cs_batch call, made on
 * the device in one call (one wave an alignment).  What hit_output needs of an alignment then comes from one more call a chunk instead of a host loop an item.
 * Input: recs / ops / ops_len as the batch call returned them and the arrays it was given (colour space: the shared LETTER-space bitfield, the colour reads, initbp).
 *   what        GM_TEXT_* bits, at least one; outputs of a kind not asked for may be NULL and are left alone
 *   qralign_in  NULL, or gm_post_sw_batch's qralign_out for these records (ops_len bytes): item i's slice of it stands in place of the qralign rebuilt from the
 *               operations (post_sw re-calls letters and moves no gap; a slice whose gaps are not the operations' is refused).  reads / initbp are then not read.
 *   reverse     NULL (none) or n flags: item i is printed as a mapping to the reverse strand
 *   clip_char   'S' or 'H'
 * Output, every buffer released with gm_free:
 *   GM_TEXT_ALIGN  *dbalign_out / *qralign_out, ops_len bytes each: item i's strings at the place of its operations, [recs[i].ops_off, + n_ops), no NUL -- the layout
 *                  of gm_post_sw_batch's qralign_out -- byte for byte what gm_sw_full_batch_strings returns (colour space: the four letter translations, lower case on
 *                  a crossover, the genome's letter for an unknown read letter); bytes outside every item's slice are 0.  Never reversed.
 *   GM_TEXT_CIGAR  *cigar_out with cigar_off[n + 1]: item i's CIGAR at [cigar_off[i], cigar_off[i + 1]), tight, no separators -- make_cigar (ref: gmapper/output.c:15-64)
 *                  on those strings: runs of columns, a gap in qralign 'D', a gap in dbalign 'I', anything else 'M', as <decimal length><op>; a leading clip of
 *                  recs[i].read_start and a trailing clip of rlen[i] - read_start - (read positions in the alignment), each only when > 0, with clip_char.
 *                  reverse[i]: the runs in reverse order (reverse_cigar, ref: :67-80).
 *   GM_TEXT_EDIT   *edit_out with edit_off[n + 1], likewise: alignment_edit_string (ref: common/output.c:60-121; the ZE:Z tag) on the item's final dbalign / qralign;
 *                  reverse[i]: passed through reverse_alignment_edit_string (ref: gmapper/output.c:83-122) -- digit runs whole, parentheses swapped, A C G T
 *                  complemented, any other character unchanged.
 * Items: status[i] = recs[i].status where that is < 0, and 0 for score <= 0, both with empty slices.  A record that does not lie inside what the caller holds -- the
 * checks of gm_sw_full_batch_strings -- or whose initbp is > 3 is refused on the host with status[i] = GM_E_ARG before anything is uploaded; the reason of the last
 * one is in gm_last_error(), its neighbours are answered.  A missing required argument, what == 0 or bits beyond 7: the call fails with GM_E_ARG.  n <= 0: GM_OK,
 * nothing is written.  No setup state is needed and no score is read.
 * Cost: a fixed number of device allocations, copies and launches whatever n is -- a sizing launch, one copy of the n lengths whose exclusive scan on the host gives the
 * offsets, a writing launch.  The genome bitfield is uploaded once a call, as by the twins.
 * ------------------------------------------------------------------------------------------- */
#define GM_TEXT_ALIGN 1   /* dbalign + qralign */
#define GM_TEXT_CIGAR 2
#define GM_TEXT_EDIT  4
int gm_sw_full_batch_text(int colour_space, int what, int n,
                          const gm_sw_full_rec_t *recs, const uint8_t *ops, uint64_t ops_len,
                          const uint32_t *genome, uint64_t genome_words,
                          const uint32_t *reads, int read_words, const int *rlen, const uint8_t *initbp, int is_rna,
                          const char *qralign_in, const uint8_t *reverse, int clip_char,
                          int *status,
                          char **dbalign_out, char **qralign_out,
                          char **cigar_out, uint64_t *cigar_off,
                          char **edit_out, uint64_t *edit_off);

/* ---------------------------------------------------------------------------------------------
 * S1 - S3, batch forms on the resident index: the entries above with (genome, genome_words, g_off) replaced by (ix, cn[], gen_st[], g_off[]).  The kernels read
 * the genome the index already holds on its device; no genome byte crosses the bus.  A window is addressed as the reference's call sites hold it (mapping.c:353-361,
 * 1306-1319):
 *   window i = glen[i] positions from offset g_off[i] of contig cn[i] on strand gen_st[i]
 *              0: genome_contigs[cn];  1: genome_contigs_rc[cn], i.e. the reverse complement of the contig, the offset counted from ITS start
 * Strand 1 of a contig is what the reference keeps in genome_contigs_rc[cn]: position p is complement_base(forward[clen - 1 - p], contig is RNA).  In colour space its
 * colours are those of genome_cs_contigs_rc[cn]: the translation of that reverse complement, the first colour against 'T' (genome.c:1107-1118).  Nothing is stored in
 * the index for it: windows of either strand are read from the forward arrays, by the routines the mapping pipeline reads them with.
 * Device: an entry makes the index's device current for its own duration and sets the caller's current device back before it returns.
 * State: each entry runs on the calling thread's setup state as its host-bitfield twin does -- sw_vector_setup (whose use_colours selects letter or colour space for
 * gm_sw_vector_batch_ix), sw_gapless_setup, sw_full_ls_setup, sw_full_cs_setup, post_sw_setup; without it: GM_E_NOTSETUP.  The stats count as the twins count.  The
 * work runs on the index's device (see above).
 *   is_rna   -1: the index's own genome_is_rna, which is what gmapper passes (the flag of the LAST contig, genome.c:1063-1064); 0 / 1: that value, as the single seams
 *            take it.  A contig's own flag always decides its reverse complement and its colour translation.
 * Colour space: gm_sw_vector_batch_ix under use_colours, gm_sw_gapless_batch_ix with colour_space = 1 and gm_index_get_windows with colours = 1 need an index built
 * with colour_space = 1; on a letter-space index they return GM_E_ARG with a message.  gm_sw_full_cs_batch_ix and gm_post_sw_batch_ix read letters only and work on
 * either kind of index.  gm_sw_vector_batch_bounded_ix is letter space, as its twin.
 * gm_sw_gapless_batch_ix scores against the WHOLE contig of that strand, as sw_gapless(genome, glen = contig length, ...) does; g_idx[i] is a position of that
 * strand's contig.
 * Records: recs[i].genome_start is counted from the start of the strand's contig, i.e. it includes g_off[i] -- the value the reference leaves in sfr->genome_start for
 * that call.  gm_post_sw_batch_ix takes the records, ops and ops_len of ONE gm_sw_full_cs_batch_ix call together with the cn / gen_st it was given.
 * Strings: gm_sw_full_batch_strings stays the one string builder.  A caller with its own genome_contigs[_rc][cn] passes that bitfield and the record as it is.  A
 * caller without a host genome fetches the windows with gm_index_get_windows -- window i as a bitfield of its own at words + i * stride_words, position 0 in nibble 0,
 * stride_words >= (glen[i] + 7) / 8; colours = 1: the colours of the strand's contig instead of its letters -- and passes that with a COPY of the record whose
 * genome_start is less g_off[i].
 * Refusals, all before anything is read through the arguments: cn outside the index, gen_st > 1, g_off < 0, glen < 1, g_off + glen beyond the contig.  The full and
 * post forms refuse the ITEM (status = GM_E_ARG, score 0, the reason of the last one in gm_last_error(), its neighbours answered; the twins' other refusals apply
 * too).  gm_index_get_windows, the vector forms and the gapless form have no per-item status: they fail the call with GM_E_ARG and name the item, as
 * gm_sw_gapless_batch does.  n <= 0: GM_OK, nothing is written.  ix == NULL: GM_E_ARG, no device is touched.
 * Cost: as for the twins, one call makes a fixed number of device allocations, copies and kernel launches whatever n is -- and here none of them is sized by the
 * genome: what is uploaded is 16 bytes a window, the reads and the per-item scalars (figures: profiles/r08a_seam_ix_timing.json).
 * ------------------------------------------------------------------------------------------- */
int gm_index_genome_is_rna(const gm_index_t *ix);   /* 1 / 0: the index's genome_is_rna (what is_rna = -1 stands for); < 0: GM_E_* */
int gm_index_get_windows(const gm_index_t *ix, int n, const int *cn, const uint8_t *gen_st, const int64_t *g_off, const int *glen,
                         int colours, uint32_t *words, int stride_words);
int gm_sw_vector_batch_ix(const gm_index_t *ix, int n, const int *cn, const uint8_t *gen_st, const int64_t *g_off, const int *glen,
                          const uint32_t *reads, int read_words, const int *rlen, const int *initbp, int is_rna, int *scores);
int gm_sw_vector_batch_bounded_ix(const gm_index_t *ix, int n, const int *cn, const uint8_t *gen_st, const int64_t *g_off, const int *glen,
                          const uint32_t *reads, int read_words, const int *rlen, int threshold, int *scores, uint8_t *stopped);
int gm_sw_gapless_batch_ix(const gm_index_t *ix, int n, const int *cn, const uint8_t *gen_st, int colour_space,
                          const uint32_t *reads, int read_words, const int *rlen, const int *g_idx, const int *r_idx, const int *initbp, int is_rna, int *scores);
int gm_sw_full_ls_batch_ix(const gm_index_t *ix, int n, const int *cn, const uint8_t *gen_st, const int64_t *g_off, const int *glen,
                          const uint32_t *reads, int read_words, const int *rlen, const struct gm_anchor *anchors, const uint8_t *revcmpl,
                          const int *threshscore, const int *maxscore, int local_alignment, gm_sw_full_rec_t *recs, uint8_t **ops, uint64_t *ops_len);
int gm_sw_full_cs_batch_ix(const gm_index_t *ix, int n, const int *cn, const uint8_t *gen_st, const int64_t *g_off, const int *glen,
                          const uint32_t *reads, int read_words, const int *rlen, const uint8_t *initbp, const struct gm_anchor *anchors, const uint8_t *revcmpl,
                          const int *threshscore, const int *crossover_scores, int xover_stride, int is_rna, int local_alignment,
                          gm_sw_full_rec_t *recs, uint8_t **ops, uint64_t *ops_len);
int gm_post_sw_batch_ix(const gm_index_t *ix, int n, const int *cn, const uint8_t *gen_st, const gm_sw_full_rec_t *recs, const uint8_t *ops, uint64_t ops_len,
                          const uint32_t *reads, int read_words, const int *rlen, const uint8_t *initbp, const char *const *quals, int is_rna,
                          gm_post_rec_t *post, char **qralign_out, char **quals_out, uint64_t *quals_len);
/* gm_sw_full_batch_text on the records of ONE gm_sw_full_*_batch_ix call with the cn / gen_st it was given (genome_start counted on the strand's contig): the genome
 * letters come from the resident forward arrays (strand 1 backwards and complemented, an RNA contig with U for A), so a caller without a host genome gets its strings,
 * CIGARs and edit strings without fetching a window.  It reads letters only and works on either kind of index; the contig and strand of a record are checked as
 * gm_post_sw_batch_ix checks them (per item); nothing sized by the genome is uploaded. */
int gm_sw_full_batch_text_ix(const gm_index_t *ix, int colour_space, int what, int n, const int *cn, const uint8_t *gen_st,
                          const gm_sw_full_rec_t *recs, const uint8_t *ops, uint64_t ops_len,
                          const uint32_t *reads, int read_words, const int *rlen, const uint8_t *initbp, int is_rna,
                          const char *qralign_in, const uint8_t *reverse, int clip_char,
                          int *status,
                          char **dbalign_out, char **qralign_out,
                          char **cigar_out, uint64_t *cigar_off,
                          char **edit_out, uint64_t *edit_off);

/* ---------------------------------------------------------------------------------------------
 * S4: the per-read pipeline.  Replaces handle_read() for unpaired letter-space reads
 * (ref: gmapper/mapping.c:1773-1868) and the read loop body around it (ref: gmapper/gmapper.c:436-560).
 * Input: n reads of one length, as 4-bit bitfields (read_words = (read_len+7)/8 words each), plus
 * names ('\n' separated) and original sequence text for SAM SEQ.  Output: the SAM records the
 * reference would append to its thread output buffer, in input order (ref: gmapper/output.c:227-774).
 * ------------------------------------------------------------------------------------------- */
typedef struct gm_session gm_session_t;
int  gm_session_create(gm_session_t **out, const gm_index_t *ix, const gm_params_t *params, int max_batch_reads);
void gm_session_free(gm_session_t *s);

typedef struct gm_map_stats {
  uint64_t reads, reads_matched, sam_records;
  uint64_t lookups, list_entries, list_bytes;      /* seed-lookup algorithmic work (SURVEY.md 8(d) B_seed) */
  uint64_t survivors, anchors, windows;            /* after region filter / collapse / window generation */
  uint64_t vec_calls, vec_cells, vec_bypassed;     /* pass-1 vector SW (ref: sw-vector.c:509 swcells) */
  uint64_t full_calls, full_cells;                 /* pass-2 (vector re-score + banded full SW) */
  uint64_t exact_order_reads;                      /* read-strands that needed heap-order emulation */
  uint64_t retries;                                /* capacity-overflow re-runs */
  uint64_t survivors_pruned;                       /* survivors with no neighbour within window_len + read_len, removed before K2 (exact) */
  uint64_t mp_unfiltered;                          /* mate-pair region counts: always 0 in a result -- a sub-batch with (pair, strand) items beyond the filter's LDS tiers is
                                                      redone through the exact row-based path (counted in retries); rows beyond their capacity fail the call (GM_E_OVERFLOW) */
  uint64_t post_sw_host_redo;                      /* colour space: device post_sw results the host routine redid because a value to be rounded (AS, MAPQ, Z0 / Z1) lay at a boundary */
  double   ms_lookup, ms_anchors, ms_pass1, ms_select, ms_pass2, ms_host;   /* device time per stage (events) */
} gm_map_stats_t;

/* A22: the read loop's text -> bitfield step inside the library.  gm_sequence_to_bitfield == fasta_sequence_to_bitfield with the reference's code
 * tables (ref: common/fasta.c:609-673, :151-200; fasta.h:26-42): letters A C G T U M R W S Y K V H D B N -> 0..15 (X and '.' -> 15, either case);
 * in colour space the first character is the primer letter (returned in *initbp), then colours 0-3 ('4', 'N', '.', 'X' -> 15).  Host code, no device.
 * gm_map_reads_text takes the reads as lines of one length and keeps the characters for the fields the reference prints from the file's text
 * (SEQ of unaligned reads and clipped ends, ref: gmapper/output.c:326-351; CS:Z, :451,727). */
int gm_sequence_to_bitfield(int colour_space, const char *seq, int seq_len, uint32_t *words, int *initbp);
int gm_map_reads_text(gm_session_t *s, int n_reads, int read_len, const char *seqs, const char *names, const char *quals, int qual_delta,
                      char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* File input: the reads file as the reference's reader takes it -- FASTA or FASTQ (fastq: 0 / 1, -1 detects from the first character),
 * plain or gzip, '#' comment lines, sequences over several lines, names cut at the first blank, any mix of read lengths, primer + colours in a
 * colour-space session (ref: common/fasta.c:61-150 fasta_open, :315-552 fasta_get_next_read_with_range).  Reads longer than longest_read_len are
 * dropped without a record and reading stops at a malformed entry, as in the reference (gmapper.c:495-521, fasta.c:362-372).  Records come back in
 * the file's order. */
int gm_map_reads_file(gm_session_t *s, const char *path, int fastq, int qual_delta, char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* The same, streaming (ref: gmapper.c:322-398,588-607: the reference reads chunks of reads and prints as it goes): the file is read at most chunk_reads reads at a time
 * (0 = 2^20; the next chunk is read and preprocessed by a second thread while this one is mapped), every read goes through the read loop's preprocessing (gm_params_t:
 * trim_*, min_avg_qv, ignore_qvs, no_qv_check) and each chunk's records are handed to `write` in the file's order.  Neither the file nor the output is held whole: host
 * memory stays at a few hundred bytes per read of one chunk.  `write` returns 0 to go on; anything else stops the call with an error.
 * gm_map_reads_file is this function with a write function that collects the text. */
typedef int (*gm_write_fn)(void *ctx, const char *text, size_t len);
int gm_map_reads_file_cb(gm_session_t *s, const char *path, int fastq, int qual_delta, size_t chunk_reads, gm_write_fn write, void *ctx, gm_map_stats_t *stats);
/* The preprocessing by itself (host code, no device): seq (primer letter first in colour space) and qual (NULL for FASTA input) are NUL-terminated and edited in place;
 * *drop = 1 when the read gets no record.  mate: 0 unpaired, 1 / 2 the mates of a pair. */
int gm_preprocess_read_text(const gm_params_t *params, int mate, char *seq, char *qual, int qual_delta, int *drop);
/* host-buffer form: reads are uploaded, SAM text is returned in a malloc()ed buffer (*sam, *sam_len) */
int gm_map_reads(gm_session_t *s, int n_reads, int read_len, const uint32_t *reads_packed,
                 const char *names, char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* device-resident form for measurement: reads_dev is a device pointer to the same packed layout;
 * runs the whole device pipeline and the host finalisation (pass-2 selection, MAPQ, SAM text)
 * unless emit_sam == 0, in which case only the alignment records are produced and counted. */
int gm_map_reads_device(gm_session_t *s, int n_reads, int read_len, const void *reads_dev,
                        int emit_sam, char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* FASTQ input (the reference's -Q, letter space): as gm_map_reads, plus the reads' QUAL strings ('\n' separated, as in the file) and the
 * file's quality offset (--qv-offset; the binary's letter-space default is 64, gmapper-defaults.h:41).  QVs do not influence letter-space
 * alignment; they travel to the SAM QUAL column: reversed with the read and re-based to PHRED+33 for mapped reads, verbatim for unmapped
 * ones (ref: output.c:419-421,539-570). */
int gm_map_reads_fastq(gm_session_t *s, int n_reads, int read_len, const uint32_t *reads_packed, const char *names,
                       const char *quals, int qual_delta, char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* colour-space reads (SOLiD): colours_packed holds n_colours 4-bit colour codes per read (0-3, 15 for a skipped cycle) in the
 * same bitfield layout, initbp[i] the primer letter code (A0 C1 G2 T3) -- what fasta_sequence_to_bitfield / fasta_get_initial_base
 * produce (ref: gmapper.c:475-487).  The session's index must have been built with colour_space = 1.  Replaces handle_read() for
 * the gmapper-cs binary: colour k-mers from colour 1 on, the colour vector filter on the read's input strand, sw_full_cs, the
 * post_sw forward-backward pass and the colour-space SAM fields (ref: mapping.c:1297-1319,375-379,1613-1614; sw-post.c:639-758;
 * output.c:441-451,485-493,572-580,717-730). */
int gm_map_reads_cs(gm_session_t *s, int n_reads, int n_colours, const uint32_t *colours_packed, const uint8_t *initbp,
                    const char *names, char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* csfastq reads: as gm_map_reads_cs, plus one QV character per colour ('\n' separated strings, offset qual_delta; 33 is the binary's colour-space
 * default, gmapper-defaults.h:42).  The QVs give per-position crossover scores in sw_full_cs (ref: gmapper.c:532-544, sw-full-cs.c:312), per-colour
 * error rates in post_sw (sw-post.c:486-491), the SAM QUAL column (post_sw's base qualities) and the CQ:Z tag (output.c:613-621,724-727). */
int gm_map_reads_cs_fastq(gm_session_t *s, int n_reads, int n_colours, const uint32_t *colours_packed, const uint8_t *initbp,
                          const char *names, const char *quals, int qual_delta, char **sam, size_t *sam_len, gm_map_stats_t *stats);
void gm_free(void *p);          /* every *sam the library hands out; a large text buffer is parked for the next call instead of being unmapped */
void gm_release_cache(void);    /* drops the parked buffer */

/* ---------------------------------------------------------------------------------------------
 * Paired mode.  Replaces handle_readpair() (ref: gmapper/mapping.c:2502-2636) with the binary's
 * default paired option sets (ref: gmapper/gmapper.c:2636-2720: two matches per mate, half-paired
 * fall-back, mapping qualities) and readpair_output() (ref: gmapper/output.c:1070-1291).
 * pair_mode / insert sizes are the reference's -p and -I options (ref: gmapper.c:1583-1623,
 * gmapper-defaults.h:28-31,184-191); mean/stddev feed the insert-size term of the paired MAPQ
 * (ref: output.c:795-808).  mates1[i] and mates2[i] are the two reads of pair i; each side has
 * ONE length per call.  Output: for every pair the paired records, then the half-paired records
 * of mate 1, then of mate 2 -- the text the reference appends to its output buffer.
 * ------------------------------------------------------------------------------------------- */
enum { GM_PAIR_OPP_IN = 1, GM_PAIR_OPP_OUT = 2, GM_PAIR_COL_FW = 3, GM_PAIR_COL_BW = 4 };   /* ref: gmapper-definitions.h:42-46 */
typedef struct gm_pair_opts {
  int pair_mode;                               /* ref: gmapper.h:140 */
  int min_insert_size, max_insert_size;        /* ref: gmapper-defaults.h:28-29  0 / 1000 */
  double insert_size_mean, insert_size_stddev; /* ref: gmapper-defaults.h:30-31  200 / 100 */
  int half_paired;                             /* ref: gmapper.h:181 true; 0 = --no-half-paired: each mate's list entries are filtered by the other mate's region
                                                  counts (mapping.c:545-608,733-742, use_mp_region_counts = 1) and no unpaired rescue runs (gmapper.c:2657-2683) */
  int match_mode;                              /* the reference's -n in paired mode (ref: gmapper-defaults.h:35 DEF_MATCH_MODE_PAIRED 4; gmapper.c:2652-2673):
                                                  4: two k-mer matches per mate (region counts; with half_paired = 0 also the mate's);
                                                  3: one match is enough where the mate has hits within reach (use_mp_region_counts 2, or 3 with half_paired = 0;
                                                     hit list mode 3, mapping.c:733-742,1080-1093,1153-1157);
                                                  2: no region counts at all, a window per anchor.   0 is read as 4.
                                                  PERFORMANCE LIMIT of modes 2 and 3: a read-strand's list entries all reach the window kernel, whose LDS tier holds 4 096 of them;
                                                  on genomes beyond a few hundred Mbp (17 k - 72 k entries per read-strand at 3 Gbp) nearly every read-strand then takes the
                                                  heavy tier (a segmented sort and a stream synchronisation per sub-batch): the output stays exact, the throughput drops by
                                                  more than an order of magnitude.  Mode 4 (the reference's default) has no such limit */
} gm_pair_opts_t;
void gm_pair_opts_default(gm_pair_opts_t *o);
int gm_map_pairs(gm_session_t *s, int n_pairs, int len1, const uint32_t *mates1_packed, int len2, const uint32_t *mates2_packed,
                 const char *names1, const char *names2, const gm_pair_opts_t *opts,
                 char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* Colour-space pairs (gmapper-cs -p <mode>; ref: handle_readpair mapping.c:2502-2636 with the colour-space branches of read_pass1_per_strand :1297-1319,
 * hit_run_full_sw :375-379 and hit_output output.c:353-355,441-451,485-537,572-580,717-730): mates as packed colours and one primer-letter byte per read, as
 * gm_map_reads_cs takes them, in all four pair modes (a mate the mode reverses keeps its colours and swaps its strand labels). */
int gm_map_pairs_cs(gm_session_t *s, int n_pairs, int len1, const uint32_t *mates1_packed, const uint8_t *initbp1, int len2, const uint32_t *mates2_packed,
                    const uint8_t *initbp2, const char *names1, const char *names2, const gm_pair_opts_t *opts,
                    char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* Paired reads from files: `path2` NULL = one file with the mates adjacent, else mate 1 from path1 and mate 2 from path2 (gmapper's -1 / -2; ref: gmapper.c:363-620).
 * Formats and rules as gm_map_reads_file; pairs of any mix of lengths; a pair with a mate beyond longest_read_len is dropped whole.  Letter or colour space by the session. */
int gm_map_pairs_file(gm_session_t *s, const char *path1, const char *path2, int fastq, int qual_delta, const gm_pair_opts_t *opts,
                      char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* streaming form (see gm_map_reads_file_cb): at most chunk_pairs pairs at a time (0 = 2^19); a pair is never split across chunks (ref: gmapper.c:2319-2322) */
int gm_map_pairs_file_cb(gm_session_t *s, const char *path1, const char *path2, int fastq, int qual_delta, const gm_pair_opts_t *opts, size_t chunk_pairs,
                         gm_write_fn write, void *ctx, gm_map_stats_t *stats);
/* csfastq pairs: as gm_map_pairs_cs, plus one QV character per colour and mate ('\n' separated strings, offset qual_delta), used as gm_map_reads_cs_fastq uses them
 * (per-position crossover scores in sw_full_cs, per-colour error rates in post_sw, QUAL = post_sw's base qualities, CQ:Z). */
int gm_map_pairs_cs_fastq(gm_session_t *s, int n_pairs, int len1, const uint32_t *mates1_packed, const uint8_t *initbp1, int len2, const uint32_t *mates2_packed,
                          const uint8_t *initbp2, const char *names1, const char *names2, const char *quals1, const char *quals2, int qual_delta,
                          const gm_pair_opts_t *opts, char **sam, size_t *sam_len, gm_map_stats_t *stats);
/* FASTQ pairs: as gm_map_pairs, plus the mates' QUAL strings ('\n' separated) and the file's quality offset; the QUAL column is printed as
 * gm_map_reads_fastq prints it (mates keep their input orientation: read_reverse() leaves seq and qual alone, ref: gmapper.c:174-185). */
int gm_map_pairs_fastq(gm_session_t *s, int n_pairs, int len1, const uint32_t *mates1_packed, int len2, const uint32_t *mates2_packed,
                       const char *names1, const char *names2, const char *quals1, const char *quals2, int qual_delta,
                       const gm_pair_opts_t *opts, char **sam, size_t *sam_len, gm_map_stats_t *stats);

/* ---------------------------------------------------------------------------------------------
 * Merging.  Replaces the mergesam program (ref: mergesam/mergesam.c main :308-816, sam_reader.c pp_ll_combine_and_check :417-716,
 * render.c :210-277; SPLITTING_AND_MERGING:100-148): SAM texts of several gmapper runs -- the same reads against different contig groups,
 * different reads against the same genome, or both -- become one SAM text in the order of the reads text, with the mapping qualities
 * recomputed from the Z0-Z6 fields gmapper writes unless --all-contigs was given.  Host code (text in, text out).
 *
 * reads_text is the reads file (FASTA or FASTQ; for pairs the file gmapper read, mates adjacent): only the names are used, and a record
 * belongs to the first read, from the last matched one on, whose name starts with its QNAME (ref: sam_reader.c:947).  Every SAM text
 * must list its records in that order (gmapper's output does).  The fields mirror mergesam's options of the same names; the
 * reference's --un / --al files are `output` 1 / 2 (FASTA / FASTQ text of the unaligned / aligned reads instead of SAM).
 * command_line, when given, is what follows "CL:" in the @PG line mergesam adds for itself (NULL: no such line). */
#define GM_MERGE_OUT_SAM              0
#define GM_MERGE_OUT_UNALIGNED_READS  1
#define GM_MERGE_OUT_ALIGNED_READS    2
typedef struct gm_merge_options {
  int max_outputs;            /* -o/--report (10) */
  int max_alignments;         /* --max-alignments (0 = all) */
  int strata;                 /* --strata */
  int half_paired;            /* --half-paired (1) / --no-half-paired (0) */
  int sam_unaligned;          /* --sam-unaligned */
  int single_best;            /* --single-best-mapping (forces max_outputs = 1) */
  int all_contigs;            /* --all-contigs: last merge of these reads, the Z fields are dropped */
  int no_mapping_qualities;   /* --no-mapping-qualities (MAPQ 255 unless leave_mapq) */
  int leave_mapq;             /* --leave-mapq-untouched */
  int no_improper_mappings;   /* --no-improper-mappings */
  int min_mapq;               /* --min-mapq (with all_contigs) */
  int fastq;                  /* reads text: 0 FASTA, 1 FASTQ, -1 detect from the first character (mergesam's default) */
  int threads;                /* -N */
  int output;                 /* GM_MERGE_OUT_* */
  int header_given;           /* --sam-header: the caller supplies the header; only the first sorted line and the @PG line are written */
  const char *command_line;
} gm_merge_options_t;
void gm_merge_options_default(gm_merge_options_t *o);
int gm_merge_sam(const gm_merge_options_t *opts, const char *reads_text, size_t reads_len, int n_files, const char *const *sam_text,
                 const size_t *sam_len, char **out, size_t *out_len);     /* *out: gm_free */

/* per-read top-K candidate rows after pass 1 (heap array order), for stage parity tests:
 * 12 x int64 per row: read st cn g_off w_len score_vector pct_score_vector matches ax ay alen awidth */
int gm_debug_tophits(gm_session_t *s, int n_reads, int read_len, const uint32_t *reads_packed,
                     long long *rows, long cap, long *n_rows);
/* the same in colour space: the reads' primer letters (A0 C1 G2 T3) go up with their colours; gm_debug_tophits takes none and leaves the session's primer buffer as it is */
int gm_debug_tophits_cs(gm_session_t *s, int n_reads, int n_colours, const uint32_t *colours_packed, const uint8_t *initbp,
                        long long *rows, long cap, long *n_rows);

/* The candidate windows of a read batch: every window read_get_hit_list_per_strand (ref: mapping.c:1025-1229) yields for each read on each strand, as the list stands
 * before pass 1 touches it -- seed lookup, region counts, anchor merge and collapse, window generation on the device, under the session's parameters
 * (seeds, -H, list cutoff, match_mode 1 / 2, region bits / overlap, window length, window-generation threshold, -F / -C, -U).  This is the front of a pipeline a
 * caller composes from the gm_*_ix seams: nothing else of it has to run on the CPU.
 *   Windows of read r, strand st: wins[off[2 r + st] .. off[2 r + st + 1]), in the reference's list order, ascending (cn, g_off).  Windows of one read-strand with
 *   equal (cn, g_off) come in no particular order (the reference keeps those in anchor order; pass 1 cannot tell them apart).
 *   off: 2 * n_reads + 1 entries, the caller's.  *wins: one buffer of *n_wins records, released with gm_free; NULL when *n_wins == 0.
 *   Letter space: initbp must be NULL.  Colour space: read_len is the number of colours and initbp (one primer letter code 0..3 per read) is required; the argument
 *   checks are those of gm_map_reads / gm_map_reads_cs (GM_E_ARG, GM_E_RANGE).  n_reads <= 0: GM_OK, off[0] = 0, *wins = NULL.
 *   n_reads may exceed the session's sub-batch size: the sub-batches run one after the other and their windows are appended.  The call takes its turn on the device
 *   like a mapping call and leaves the session ready for any other call.
 *   stats (or NULL): reads, lookups, list_entries, list_bytes, survivors, anchors, windows (== *n_wins), survivors_pruned, exact_order_reads, retries, ms_lookup,
 *   ms_anchors; every other field 0.
 *   Unpaired sessions only: a session has no pair mode of its own (pairing is an argument of gm_map_pairs*), so this call has no paired form (gm_pair_mappings is the one-call seam for pairs), and the
 *   mate-pair region counts of the paired option sets (-p) never apply here.
 * How a window feeds the _ix seams (cn, gen_st, g_off, glen), with contig_len the length of contig cn:
 *   read strand 0: (cn, 0, g_off, w_len) with the read as given;
 *   read strand 1: (cn, 1, contig_len - g_off - w_len, w_len) with the read as given -- what reverse_hit (ref: mapping.c:254-263) makes of the hit, and what the
 *                  reference scores for ZV and, in colour space, in pass 1.  In letter space the window may equally be taken as (cn, 0, g_off, w_len) with the
 *                  reverse complement of the read (the reference's pass 1).
 *   The anchor box is relative to the window as the list holds it (before reverse_hit): a caller that turns a hit onto strand 1 of the contig reverses the box
 *   itself, as anchor_reverse (ref: anchors.h:30-34) does. */
typedef struct gm_read_window {      /* 12 x 32 bits = 48 bytes, no padding */
  int32_t  read;                     /* index of the read in this call */
  int32_t  st;                       /* read strand: 0 the read as given, 1 its reverse complement (read_hit.st) */
  int32_t  cn;
  uint32_t g_off;                    /* window start on the FORWARD contig (g_off_pos_strand; == g_off before reverse_hit) */
  int32_t  w_len;
  int32_t  score_window_gen, matches;
  int32_t  ax, ay, alen, awidth;     /* anchor box relative to the window, as read_get_hit_list_per_strand leaves it (before reverse_hit) */
  int32_t  reserved;                 /* 0 */
} gm_read_window_t;
int gm_read_window_size(void);       /* sizeof(gm_read_window_t), for the Python mirror */
int gm_read_windows(gm_session_t *s, int n_reads, int read_len, const uint32_t *reads_packed, const uint8_t *initbp,
                    gm_read_window_t **wins, uint64_t *n_wins, uint64_t *off, gm_map_stats_t *stats);

/* The two selections of a read batch, so that a chunk is a chain of batch calls on arrays with nothing per read on the CPU in between:
 *   gm_read_windows -> gm_score_windows (or, a read per window: gm_sw_vector_batch_ix; -U: gm_sw_gapless_batch_ix) -> gm_select_pass1[_f1] -> gm_sw_full_ls_batch_ix (colour space: gm_sw_full_cs_batch_ix, then
 *   gm_post_sw_batch_ix) -> gm_select_pass2 -> gm_sw_full_batch_text_ix.
 * Both take their rules from the session's gm_params_t, read neither the genome nor the reads, make a fixed number of device allocations, copies and launches whatever
 * n is, take their turn on the device like gm_read_windows and leave the session ready for any other call.  Unpaired sessions only (see gm_read_windows); the mapping
 * entries do not use them and print what they printed.
 *
 * gm_select_pass1: read_pass1_per_strand's overlap rule and threshold and read_get_vector_hits' ext-heap (ref: mapping.c:1261-1339, 1376-1411, heap.h:226-327; SURVEY
 * A10 / A13) on the windows of gm_read_windows and their scores.
 *   wins, n_wins, off[2 n_reads + 1]   exactly as gm_read_windows returned them;  scores[n_wins]: the vector (under -U: gapless) score of each window as pass 1
 *   takes it -- letter space: (cn, 0, g_off, w_len) against the read, for a strand-1 window against the read's reverse complement (mapping.c:1321-1328); colour space:
 *   the address the gm_read_windows block gives (strand 1: the reverse-complement contig), against the read as given (:1297-1319).  Scoring a letter-space strand-1
 *   window on the reverse-complement contig against the read as given is NOT the same call: the vector filter is not mirror-symmetric (2 of the 5 586 windows of
 *   tests/golden/stress_60bp score 25 points apart), and the reference's top hits are those of the first form;  read_len: the reads' length (colour space: the colours).
 *   Per read, strand 0 then strand 1, windows in list order: a window with matches < match_mode is passed over; a window on the contig of the last PASSING window of
 *   its read-strand with g_off + (uint)abs_or_pct(window_overlap, W) <= that window's g_off + W is skipped and counts from then on with score 0 -- W the session's
 *   (uint16_t)abs_or_pct(window_len, read_len), not the window's clamped w_len; score_max = min(read_len, w_len) * match; pct = (1000 * 100 * score) / score_max; the
 *   last passing window advances only where score >= (int)abs_or_pct(sw_vect_threshold, score_max).  A window enters the heap when score >= that threshold and
 *   (fewer than num_tmp_outputs are in it, or its key > the heap's minimum: a strict >); the key is pct, or the score for an absolute threshold.
 *   Output: *hits, one buffer of *n_hits records (gm_free; NULL when there are none), read r's at [hit_off[r], hit_off[r + 1]) in the heap's ARRAY order, which is the
 *   input order of pass 2 and of its stable sorts; hit_off: n_reads + 1 entries, the caller's.  A hit of strand 1 has been turned as reverse_hit turns it (gen_st = 1,
 *   g_off = contig_len - g_off - w_len, the anchor box through anchor_reverse); strand 0 keeps gen_st = 0: (cn, gen_st, g_off, w_len), the box and the read as given
 *   are what gm_sw_full_ls_batch_ix / gm_sw_full_cs_batch_ix take, nothing is left for the caller to turn.  win: the record's window in wins.
 *   NOT emulated here: the f1 call cache (hash_filter_calls, on by default).  This entry takes the scores it is given, so its result is the reference's under -Z.
 *   The cache matters wherever two windows of one read-strand share a cache slot and differ in score, and that takes no hash collision: hash_genome_window (ref:
 *   common/util.h:221-241) hashes base & 3, so S, Y, K and N fold onto A, C, G and T, and a window and its copy with such IUPAC letters (twins) ALWAYS share a slot
 *   while they score differently -- a perfect read whose damaged copy comes first in list order takes the copy's score and can come out unmapped
 *   (tests/golden/f1_twins_60bp: 49 of 300 reads).  gm_select_pass1_f1 and gm_read_hits below emulate the cache, as the mapping entries do.
 *   Refusals: num_tmp_outputs > 64: GM_E_RANGE (the mapping entries select at most 64 and say nothing; a seam must not); 2^31 windows or more: GM_E_RANGE.  Offsets
 *   that do not ascend from 0, off[2 n_reads] != n_wins, a window whose read / st contradicts its slot, cn outside the index, w_len < 1, a window that ends beyond
 *   its contig, read_len < 1: GM_E_ARG, before anything is uploaded.  n_reads <= 0: GM_OK, hit_off[0] = 0, *hits = NULL. */
typedef struct gm_pass1_hit {        /* 16 x 32 bits = 64 bytes, no padding */
  int32_t  read, st;                 /* as the window's: st is the READ strand the seeds matched on */
  int32_t  win;                      /* index of the window in wins */
  int32_t  cn, gen_st;               /* gen_st = st: the hit lies on strand gen_st of the contig, the read as given */
  uint32_t g_off;                    /* on strand gen_st of the contig */
  int32_t  w_len;
  int32_t  score_vector, pct_score_vector;      /* after the overlap rule: 0 for a skipped window */
  int32_t  score_max, matches, score_window_gen;
  int32_t  ax, ay, alen, awidth;     /* the anchor box, on the turned window for strand 1 */
} gm_pass1_hit_t;
int gm_pass1_hit_size(void);         /* sizeof(gm_pass1_hit_t), for the Python mirror */
int gm_select_pass1(gm_session_t *s, int n_reads, int read_len, const gm_read_window_t *wins, uint64_t n_wins, const uint64_t *off, const int *scores,
                    gm_pass1_hit_t **hits, uint64_t *n_hits, uint64_t *hit_off);

/* Pass 1 as a seam: the scores pass 1 gives the windows, the selection with the f1 call cache, and both behind gm_read_windows' front in one call.
 *
 * gm_score_windows: scores[i] = what f1_run computes for window i in read_pass1_per_strand (ref: mapping.c:1297-1329) under the session's scores and `ungapped` flag,
 * never cut short by the early stop; a window with matches < match_mode is scored like any other (the selection passes over it).
 *   reads    n_reads, read_len, reads_packed, initbp as gm_read_windows takes them: the batch goes up once and the kernel fetches a window's read by wins[i].read; no
 *            copy of a read per window is made on the host or the device, and nothing is turned by the caller.
 *   wins, n_wins, off[2 n_reads + 1]   as gm_read_windows returned them, or the caller's own (checked as gm_select_pass1 checks them).
 *   Letter space: (cn, g_off, w_len) on the forward contig against the read, for a strand-1 window against the read's reverse complement, made on the device (a read
 *   with U and no T through the RNA complement table).  Colour space: the window turned onto the read's input strand (strand 1: contig_len - g_off - w_len on the
 *   reverse-complement contig) against the read as given, with its primer letter.  `ungapped` sessions: sw_gapless over the whole contig on the diagonal through
 *   g_idx = g_off + ax, r_idx = ay -- letter space: the box as the record holds it, the read turned; colour space: the hit and its box turned by reverse_hit /
 *   anchor_reverse first.
 *   slots (n_wins, or NULL): hash_genome_window(array, goff, w_len) % 1048576 of the array and offset f1_run is handed (ref: common/util.h:221-241, f1-wrapper.h:27,
 *   106) -- letter space the forward letters, colour space the colour translation of the turned strand: the window's f1 cache slot.
 *   Refusals, on the host before anything is uploaded: the read arguments as gm_read_windows (GM_E_ARG, GM_E_RANGE), the windows and offsets as gm_select_pass1
 *   (GM_E_ARG, GM_E_RANGE); a window too long for the kernel's LDS beside these reads (48 KB: about 9 000 positions, 8 000 in colour space): GM_E_RANGE.  n_reads <= 0 or n_wins == 0: GM_OK.
 *
 * gm_select_pass1_f1: gm_select_pass1 with the cache rule of f1_run (ref: f1-wrapper.h:97-134) applied per read-strand (the tag advances once per read-strand,
 * mapping.c:1268).  In list order, a window that gets past the matches check and the overlap check takes the score of the FIRST earlier window of its read-strand that
 * was itself computed and has the same slot (one bypassed call), else it keeps its own score and is computed; a window passed over, skipped or bypassed is not
 * computed.  pct, the threshold and score_max are the window's own; the last passing window advances on the TAKEN score; hits carry the taken score.
 *   slots[n_wins]: gm_score_windows'.  slots == NULL: the call is gm_select_pass1, bit for bit.  bypassed (or NULL): the number of bypassed calls (f1_stats').
 *   Everything else, the refusals included, as gm_select_pass1.
 *
 * gm_read_hits: gm_read_windows -> gm_score_windows -> gm_select_pass1_f1 in one call, byte-equal to the three on the same input (equal windows of a read-strand in no
 * particular order, as gm_read_windows leaves them).  Per sub-batch the front of gm_read_windows runs unchanged (heavy tier, counter read, capacity growth), then the
 * scan and scatter, the scoring on the reads and records that are on the device already, the selection -- with the cache rule when and only when the session's
 * hash_filter_calls is set, so the hits are the reference's by default and its hits under -Z with hash_filter_calls = 0 -- and the emit.  Only the hits and hit_off
 * come down; hit `win` indices and the offsets are global across sub-batches.
 *   wins, n_wins, off, scores: all four NULL, or all four given: then the windows (gm_free), off[2 n_reads + 1] (the caller's) and the windows' OWN scores (gm_free;
 *   before the cache rule) come down too.
 *   stats (or NULL): as gm_read_windows, and vec_calls / vec_cells (every window is scored, none is bypassed on the device) and vec_bypassed (the cache rule's count).
 *   Refusals: num_tmp_outputs > 64: GM_E_RANGE; the four optional outputs given in part: GM_E_ARG; all others as gm_read_windows. */
int gm_score_windows(gm_session_t *s, int n_reads, int read_len, const uint32_t *reads_packed, const uint8_t *initbp,
                     const gm_read_window_t *wins, uint64_t n_wins, const uint64_t *off,
                     int *scores /* n_wins */, uint32_t *slots /* n_wins, or NULL */);
int gm_select_pass1_f1(gm_session_t *s, int n_reads, int read_len, const gm_read_window_t *wins, uint64_t n_wins, const uint64_t *off,
                       const int *scores, const uint32_t *slots, gm_pass1_hit_t **hits, uint64_t *n_hits, uint64_t *hit_off, uint64_t *bypassed /* or NULL */);
int gm_read_hits(gm_session_t *s, int n_reads, int read_len, const uint32_t *reads_packed, const uint8_t *initbp,
                 gm_pass1_hit_t **hits, uint64_t *n_hits, uint64_t *hit_off,
                 gm_read_window_t **wins, uint64_t *n_wins, uint64_t *off, int **scores /* these four: all NULL, or all given */,
                 gm_map_stats_t *stats);

/* gm_select_pass2: read_pass2's selection and compute_unpaired_mqv (ref: mapping.c:1628-1750, read_remove_duplicate_hits :1552-1600, hit_run_post_sw :1609-1625,
 * output.c:777-793, 975-984) on the records of ONE full batch call over the hits of gm_select_pass1, in that order.
 *   hit_off[n_reads + 1], hits[n_hits]   as gm_select_pass1 returned them (read, cn, gen_st and score_max are read);  recs[n_hits]: the records of the full call;
 *   post[n_hits]: colour space with mapping qualities on (neither local_alignment nor no_mapping_qualities): the answers of gm_post_sw_batch(_ix), required; else NULL.
 *   Per read: score_full = the record's score (a refused record counts as 0); with mapping qualities on and score_full > 0 the posterior (letter space:
 *   pow(2, (score - rmapped (2 alpha + beta)) / alpha); colour space: post's) and score_full = max(0, (int)rint(alpha log(posterior) / log 2 + rmapped (2 alpha +
 *   beta))); pct = (1000 * 100 * score_full) / score_max; kept where score_full >= abs_or_pct(sw_full_threshold, score_max) as doubles.  Two duplicate removals: a
 *   stable sort by (cn, gen_st, genome_start), every equal run collapsed to its FIRST maximum key (pct, or score_full for an absolute threshold), then the same by
 *   (cn, gen_st, -genome_start - rmapped + deletions - insertions).  A stable sort by descending key, the cut to num_outputs, strata (the leading run of equal
 *   score_full), max_alignments (more than that many leaves none).  With mapping qualities on: z1 = the sum of the posteriors, z0 = the posterior, mqv =
 *   qv_from_pr_corr(z0 / z1) and 0 below 4, single_best_mapping keeps the first mapping of the highest mqv; otherwise mqv = 255 and posterior = z0 = z1 = 0.
 *   The doubles go through the host's libm, as in the mapping entries (the same functions); the sorts and removals run on the device, a wave a read.
 *   Output: *maps, one buffer of *n_maps records (gm_free; NULL when there are none), read r's at [map_off[r], map_off[r + 1]) in the reference's output order;
 *   map_off: n_reads + 1 entries, the caller's.  hit: the mapping's index in hits / recs; score_full is the SAM AS, mqv the MAPQ, z0 / z1 the Z0 / Z1 tags' values.
 *   flags bit 0, the rounding guard: the mapping is a colour-space one whose post[hit].by_host == 0 (a device posterior, exact to 1e-9 relative but not to the bit),
 *   and a value that this read's AS, MAPQ, Z0 or Z1 is rounded from lies within 1e-7 of its rounding boundary.  Recipe: redo the posterior of every hit of such a
 *   read with the single post_sw seam, put the values into a copy of post with by_host = 1, and call again for those reads; the mapping entries do the same inside.
 *   (A read none of whose hits comes out has no record to carry the bit; its device posteriors decided nothing that is printed.)
 *   Refusals (GM_E_ARG, before anything is uploaded): offsets that do not ascend from 0, more than 64 hits of one read, a hit whose read is not its slot's, cn
 *   outside the index, gen_st > 1, score_max < 1, post missing where it is required.  n_reads <= 0: GM_OK, map_off[0] = 0, *maps = NULL. */
typedef struct gm_mapping {          /* 6 x 32 bits + 3 doubles = 48 bytes, no padding */
  int32_t  read;
  int32_t  hit;                      /* index into hits / recs */
  int32_t  score_full;               /* AS */
  int32_t  pct_score_full;
  int32_t  mqv;                      /* MAPQ */
  int32_t  flags;                    /* bit 0: rounding guard, see above */
  double   posterior, z0, z1;
} gm_mapping_t;
int gm_mapping_size(void);           /* sizeof(gm_mapping_t), for the Python mirror */
int gm_select_pass2(gm_session_t *s, int n_reads, const uint64_t *hit_off, const gm_pass1_hit_t *hits, const gm_sw_full_rec_t *recs, const gm_post_rec_t *post,
                    gm_mapping_t **maps, uint64_t *n_maps, uint64_t *map_off);

/* gm_sam_records: the last link of the chain -- the SAM text of a chunk's mappings, made on the device (a wave a record) from the arrays the seams above return.  After
 * it a chunk goes from packed reads to the reference's bytes through batch calls only.  The rules are hit_output's for an unpaired read (ref: gmapper/output.c:227-774),
 * under the session's gm_params_t; the mapping entries do not use this entry and print what they printed.
 *   reads       n_reads, read_len, reads_packed, initbp as the mapping entries take them (colour space: read_len colours, initbp required; letter space: initbp NULL).
 *   names       '\n' separated, or NULL: r<index>, the names gm_map_reads gives.  seqs: NULL, or the reads' text lines as gm_map_reads_text takes them (read_len
 *               letters; colour space: the primer letter and read_len colours).  quals / qual_delta: NULL, or '\n' separated QV strings of read_len characters and
 *               the file's offset.
 *   hits, recs  n_hits of each: gm_select_pass1's hits and the records of the ONE full batch call over them.  score_vector: ZV of every hit, or NULL:
 *               hits[i].score_vector (letter space prints pass 2's second vector score there, mapping.c:386-396: pass that).
 *   post, post_quals, post_quals_len   colour space with mapping qualities on: the answers of gm_post_sw_batch(_ix) and its quals_out; else NULL.
 *   qralign, ops_len   colour space: gm_post_sw_batch's qralign_out, or the text call's where there is no post_sw; hit i's slice is [recs[i].ops_off, + n_ops).
 *   cigar, cigar_off / edit, edit_off   gm_sw_full_batch_text[_ix] over ALL n_hits records with reverse[i] = hits[i].gen_st and clip_char 'S' (letter space) / 'H'
 *               (colour space): n_hits + 1 offsets each.  edit / edit_off are required iff extra_sam_fields.
 *   maps, map_off, n_maps   gm_select_pass2's: read r's mappings at [map_off[r], map_off[r + 1]).
 * Output: *sam (gm_free; NULL when nothing is printed), *sam_len bytes: the text gm_map_reads* would append for these reads, in input order; read r's records are the
 * bytes [read_off[r], read_off[r + 1]) (read_off: n_reads + 1 entries, the caller's).  A read with mappings gets one record per mapping, in maps order; a read without
 * gets the unaligned record when sam_unaligned is set and nothing otherwise.
 * Mapped record: QNAME, FLAG 0 / 16 (gen_st), RNAME, POS, MAPQ = mqv, CIGAR (the slice as given), "*\t0\t0", SEQ, QUAL, then the tags.
 *   POS         forward strand: genome_start + 1; strand 1: (contig_len - genome_start) - (rmapped - 1 - deletions + insertions) (output.c:626-634); the low 32 bits,
 *               printed unsigned.
 *   SEQ, QUAL   letter space: every base from its code (A C G T, anything else N); strand 1: the read reversed and complemented.  With seqs, the positions the
 *               alignment clips (outside [read_start, read_start + rmapped)) print the file's letter through seq_from_text (output.c:326-351), on strand 1 its
 *               complement, a '.' staying '.'.  QUAL: '*', or the QV characters re-based to PHRED + 33 (+ 33 - qual_delta) and reversed with the read.
 *               colour space: SEQ = the non-gap characters of the hit's qralign slice, upper-cased, anything outside A C G T N an N; strand 1: reversed and
 *               complemented.  QUAL = the hit's post_quals slice, reversed on strand 1; '*' without quals, without post / post_quals, or for an empty slice.
 *   tags        AS:i = score_full; Z0:i / Z1:i, only with mapping qualities on and not all_contigs: (int)(1000 * -log(z)) of the mapping's z0 / z1 -- computed on the
 *               HOST by the function the mapping entries print them with (the host's log, one per mapping) and uploaded as integers: the kernel has no double
 *               arithmetic; NM:i = mismatches + deletions + insertions (colour space: post's mismatches where post is given).  Colour space, then: CQ:Z (the QV
 *               line; only with quals), CS:Z (the seqs line verbatim; without seqs the primer letter and the colours, '.' for a code above 3), CM:i = crossovers
 *               (post's where given), XX:Z = the qralign slice.
 *   tail        RG:Z (read_group, when set); with extra_sam_fields ZM:i ZR:i ZV:i ZH:i ZE:Z = hits[].matches, hits[].score_window_gen, score_vector, recs[].score, the
 *               edit slice; then '\n'.
 * Unaligned record: QNAME "\t4\t*\t0\t0\t*\t*\t0\t0\t", then letter space: SEQ (the codes' letters A C G T U M R W S Y K V H D B N, or with seqs the file's letters
 *   through seq_from_text), a tab and QUAL (the QV line verbatim, or '*'); colour space: "*\t*\tCQ:Z:" the QV line or '*', "\tCS:Z:" as above; then the tail without
 *   the extra fields.
 * Scope: unpaired sessions (see gm_read_windows); sam_r2 is a paired option and is ignored; output_format 0 only: --shrimp-format / --pretty return GM_E_ARG.
 * Refusals (GM_E_ARG, on the host before anything is uploaded, the item named in gm_last_error()): a missing required array; map_off not ascending from 0 or not ending
 * at n_maps; a mapping whose read is not its slot's; hit outside n_hits; a hit whose cn is outside the index or whose gen_st is above 1; a record with status < 0 or
 * score <= 0 that a mapping points to; a cigar, edit, qralign or post_quals slice outside its buffer (cigar / edit: offsets that descend or pass the last one); names,
 * seqs or quals with fewer lines than reads, or a seqs / quals line of the wrong length; a qralign slice whose read positions are not the record's rmapped, or with
 * its clip run past read_len.  n_reads <= 0: GM_OK, read_off[0] = 0, *sam = NULL.  The session is usable after every refusal.
 * Cost: a fixed number of device allocations, copies and launches whatever the sizes -- the caller's buffers go up as they are beside one 112-byte line a record, a
 * sizing launch, the scan of gm_read_windows, a writing launch, one copy of the offsets and one of the text.  The call takes its turn on the device like
 * gm_select_pass2 and leaves the session ready for any other call. */
typedef struct gm_sam_input {
  /* the reads, as the mapping entries take them */
  int n_reads, read_len;                 /* colour space: number of colours */
  const uint32_t *reads_packed;          /* n_reads * ((read_len + 7) / 8) words */
  const uint8_t  *initbp;                /* colour space: required; letter space: NULL */
  const char *names;                     /* '\n' separated, or NULL: the names gm_map_reads gives when it gets NULL */
  const char *seqs;                      /* NULL, or the reads' text lines as gm_map_reads_text takes them */
  const char *quals; int qual_delta;     /* NULL, or '\n' separated QV strings and the file's offset */
  /* the chain's arrays */
  uint64_t n_hits;
  const gm_pass1_hit_t   *hits;          /* gm_select_pass1 */
  const gm_sw_full_rec_t *recs;          /* the ONE full batch call over those hits */
  const int              *score_vector;  /* ZV per hit; NULL: hits[i].score_vector (letter space: pass 2's second vector score, mapping.c:386-396) */
  const gm_post_rec_t    *post;          /* colour space with mapping qualities on, else NULL */
  const char *post_quals; uint64_t post_quals_len;   /* gm_post_sw_batch's quals_out, or NULL */
  const char *qralign; uint64_t ops_len; /* colour space: post's qralign_out (or the text call's, where there is no post_sw); letter space: NULL */
  const char *cigar; const uint64_t *cigar_off;      /* gm_sw_full_batch_text[_ix] over all n_hits, reverse[i] = gen_st, clip 'S' letter / 'H' colour */
  const char *edit;  const uint64_t *edit_off;       /* required iff extra_sam_fields */
  uint64_t n_maps; const gm_mapping_t *maps; const uint64_t *map_off;   /* gm_select_pass2, n_reads + 1 offsets */
} gm_sam_input_t;
int gm_sam_input_size(void);             /* sizeof(gm_sam_input_t), for the Python mirror */
int gm_sam_records(gm_session_t *s, const gm_sam_input_t *in, char **sam, size_t *sam_len, uint64_t *read_off /* n_reads + 1, caller's */);

/* gm_read_mappings: pass 2 as a seam -- packed reads to the arrays gm_sam_input_t takes, in one call.  The back half of the unpaired chain (the second vector score, the
 * full alignment, gm_select_pass2, the text of the mappings) behind gm_read_hits' front, on arrays that stay on the device: a caller who wants a chunk's mappings as
 * arrays (contig, strand, position, MAPQ, AS, CIGAR) makes this one call instead of gm_read_hits, a gather of a read per hit, gm_sw_vector_batch_ix,
 * gm_sw_full_ls_batch_ix, gm_select_pass2 and gm_sw_full_batch_text_ix with host code in between.  Letter space, unpaired (see gm_read_windows); the mapping entries do
 * not use it and print what they printed.
 * The rule it applies per hit is hit_run_full_sw's (ref: gmapper/mapping.c:332-402), letter space:
 *   thresh  = (int)abs_or_pct(sw_full_threshold, score_max): -sw_full_threshold for a negative (absolute) threshold, else score_max * (sw_full_threshold / 100.0) as
 *             doubles, truncated (ref: common/util.h:53) -- evaluated by the host in that very expression, once per possible score_max of the call;
 *   window  = (cn, gen_st, g_off, w_len) of the hit, resolved on the index as the _ix seams resolve it; the anchor box is the hit's; the read is the read as given;
 *   sv      = sw_vector of that window and read (:386-388), also in an `ungapped` session (:386-394); this is ZV;
 *   sv >= thresh: sw_full_ls(window, read, threshscore = thresh, maxscore = sv, revcmpl = gen_st && tiebreak_rev, the box, local_alignment) (:391-394): the hit's record,
 *             exactly gm_sw_full_ls_batch_ix's -- genome_start counted on the strand's contig; score 0: rmapped = gmapped = 1, genome_start = g_off;
 *   sv <  thresh: the record the reference leaves (calloc and score = 0, :365,396-398): every field 0, status 0, n_ops 0.
 * Then gm_select_pass2's rules on those records (its doubles through the host's libm by the same functions: what comes down for that step is score, rmapped and
 * score_max of every hit, not the hits), and gm_sw_full_batch_text_ix's CIGAR -- with extra_sam_fields also the edit string -- with reverse = gen_st and clip 'S' for
 * the hits that ARE mappings; every other hit has an empty slice.  Under the session's gm_params_t: global and local_alignment, ungapped, tiebreak_rev, match_mode 1 / 2,
 * hash_filter_calls, no_mapping_qualities, single_best_mapping, strata, max_alignments, num_outputs, any score set the session accepts.
 * Per sub-batch of the session: the front of gm_read_hits unchanged (heavy tier, counter read, capacity growth, scan, scatter, scores, selection, emit); a kernel that
 * makes the pass-2 items from the device hits, naming a hit's read by its ROW of the sub-batch's reads (no copy of a read per hit is made anywhere); the second vector
 * score; a compaction of the hits with sv >= thresh into the full-alignment work list, in hit order, by wave ballots and prefix sums (no atomics: nothing depends on
 * timing); the full alignment of that list only; the records; the selection; the text of the selected.  A fixed number of allocations, copies and launches a
 * sub-batch; device memory under one owner; the call takes its turn on the device like gm_read_hits and leaves the session ready for any other call.
 * Result: ONE struct, released by ONE call, gm_read_mappings_free (which frees the buffers and zeroes the struct; the struct itself is the caller's).  Indices and
 * offsets are the call's, not the sub-batch's.  The four offset arrays are always there (n_reads + 1 / n_hits + 1 entries); an array of records or bytes is NULL when it
 * would be empty.
 *   hits, hit_off[n_reads + 1]    as gm_read_hits returns them;
 *   score_vector[n_hits]          sv, the second vector score (ZV);  recs[n_hits]: see above; recs[i].ops_off / n_ops point into `ops`, whether or not it was asked for;
 *   maps, map_off[n_reads + 1]    as gm_select_pass2 returns them (hit: the index in hits / recs);
 *   cigar, cigar_off[n_hits + 1]  and, when has_edit (the session's extra_sam_fields), edit, edit_off[n_hits + 1]: as gm_sam_input_t takes them;
 *   ops, ops_len                  want_ops != 0 only: the edit operations of all records, compacted in hit order (else NULL, and ops_len is still their total).
 * stats (or NULL): as gm_read_hits fills it, and full_calls / full_cells: the hits that were aligned and their window x read cells.
 * Refusals, on the host before anything is uploaded, the session usable afterwards: s or out NULL: GM_E_ARG; a colour-space session: GM_E_ARG (colour space needs
 * post_sw and its host re-dos between the full alignment and the selection: use the chain of seams, gm_read_hits -> gm_sw_full_cs_batch_ix -> gm_post_sw_batch_ix ->
 * gm_select_pass2 -> gm_sw_full_batch_text_ix); the read arguments as gm_read_hits (GM_E_ARG, GM_E_RANGE); num_tmp_outputs > 64: GM_E_RANGE; a read length whose
 * windows do not fit the full-alignment kernel's LDS beside the read (the admission test of gm_sw_full_ls_batch): GM_E_RANGE.  A session has no pair mode of its own
 * (see gm_read_windows), so there is no paired session to refuse (pairs: gm_pair_mappings).  n_reads <= 0: GM_OK, no hits.  After any failure *out holds nothing to free. */
typedef struct gm_read_mappings {
  int32_t  n_reads, has_edit;
  uint64_t n_hits, n_maps, cigar_len, edit_len, ops_len;
  gm_pass1_hit_t   *hits;  uint64_t *hit_off;
  int32_t          *score_vector;
  gm_sw_full_rec_t *recs;
  gm_mapping_t     *maps;  uint64_t *map_off;
  char *cigar; uint64_t *cigar_off;
  char *edit;  uint64_t *edit_off;
  uint8_t *ops;
} gm_read_mappings_t;
int  gm_read_mappings_size(void);        /* sizeof(gm_read_mappings_t), for the Python mirror */
int  gm_read_mappings(gm_session_t *s, int n_reads, int read_len, const uint32_t *reads_packed, const uint8_t *initbp, int want_ops,
                      gm_read_mappings_t *out, gm_map_stats_t *stats);
void gm_read_mappings_free(gm_read_mappings_t *out);

/* gm_read_mappings_cs: colour-space pass 2 as a seam -- packed colour reads to the arrays gm_sam_input_t takes, in one call: gm_read_mappings for a colour-space
 * session.  It stands for the chain gm_read_hits -> gm_sw_full_cs_batch_ix -> gm_post_sw_batch_ix -> the rounding-guard recipe of gm_select_pass2 -> gm_select_pass2
 * again -> gm_sw_full_batch_text_ix, with its copy of a read per hit, its thread-local post_sw_setup, its host re-dos of by_host items and its re-do of flagged reads:
 * a sub-batch's hits, records, operations and posteriors stay on the device from the front to the text.  Unpaired; the mapping entries do not use it.
 * The rule per hit is hit_run_full_sw's for colour space (ref: gmapper/mapping.c:375-379) and hit_run_post_sw's (:1609-1625):
 *   thresh  = (int)abs_or_pct(sw_full_threshold, score_max), evaluated by the host in that double expression, once per possible score_max of the call (as gm_read_mappings);
 *   every hit, with no second vector score, no compaction and no second filter, goes through
 *             sw_full_cs(window, read, initbp, threshscore = thresh, revcmpl = gen_st && tiebreak_rev, is_rna of the index, the hit's box, local_alignment, the read's
 *             crossover row): the hit's record, exactly gm_sw_full_cs_batch_ix's (all zero where no alignment reaches thresh);
 *   crossover row: without quals, or under ignore_qvs, the global crossover score; with quals the per-position row the mapping entry gm_map_reads_cs_fastq makes of the
 *             read's QVs (ref: gmapper.c:532-544) -- one row a read goes up once per call, not one a hit;
 *   score > 0 and mapping qualities on (neither local_alignment nor no_mapping_qualities): post_sw under the SESSION's constants (pr_xover => alpha => pr_mismatch, the gap
 *             probabilities from the scores) and, with quals, the session's table of per-colour error rates.  The calling thread's post_sw_setup is neither read nor
 *             disturbed.  score_full, pct_score_full and the threshold compare by the functions gm_select_pass2 calls: they are gm_select_pass2's rules.
 * The rounding guard is applied INSIDE.  An item the kernel flags (a letter call or a base quality the last bits of exp / log could decide) is redone by the library's host
 * routine: by_host = 1.  A read that comes out of the selection with flag bit 0 set (see gm_select_pass2) has its device posteriors redone by the host routine and the
 * selection is run once more; after it every hit of such a read is by_host, so NO mapping of the result has flag bit 0 set.  A by_host = 0 posterior is within 1e-9 relative
 * of the single seam's (see gm_post_sw_batch); a by_host = 1 posterior carries the single seam's bits.  stats->post_sw_host_redo counts both kinds of re-do.  The guard's
 * tolerance is 1e-7; builds with the tuning knobs read GM_POST_GUARD_TOL, as the mapping entries do.
 * quals: NULL, or one QV string of n_colours characters a read, '\n' separated, as gm_map_reads_cs_fastq takes them; qual_delta re-bases a character to its QV.
 * Result: ONE struct, released by ONE call, gm_read_mappings_cs_free.  Every field of gm_read_mappings_t, with
 *   score_vector[n_hits]          pass 1's score of the hit (ZV): colour space has no second vector call;
 *   cigar / edit                  of the hits that ARE mappings, clip character 'H'; every other hit has an empty slice;
 *   ops, ops_len                  want_ops != 0 only; ops_len and recs[].ops_off are compacted in hit order whether or not ops comes down;
 * and what colour space adds to gm_sam_input_t:
 *   post[n_hits]                  gm_post_rec_t per hit (qual_off into post_quals); NULL when the session has no post_sw (local_alignment or no_mapping_qualities);
 *   post_quals, post_quals_len    the base qualities post_sw leaves, hit after hit (NULL / 0 without post_sw);
 *   qralign                       ops_len bytes, hit i's slice at [recs[i].ops_off, + n_ops): with post_sw its re-called qralign for every hit with an alignment; without,
 *                                 the qralign of the strings built from the operations for the hits that are mappings, zero bytes elsewhere.
 * Per sub-batch a fixed number of allocations, copies and launches (one more selection launch when the guard fires, one post_sw launch: the reads of a call have one
 * length); for the host re-dos only the flagged items' operations, genome stretches and reads are fetched.  Device memory under one owner; the call takes its turn on the
 * device like gm_read_hits.
 * Refusals, on the host before anything is uploaded, the session usable afterwards: s or out NULL: GM_E_ARG; a letter-space session: GM_E_ARG (use gm_read_mappings); the
 * read arguments as gm_read_hits checks them, initbp required (GM_E_ARG, GM_E_RANGE); quals with fewer lines than reads or a line whose length is not n_colours: GM_E_ARG;
 * quals under a crossover score whose doubled value does not fit 8 bits: GM_E_RANGE, the message of gm_map_reads_cs_fastq; num_tmp_outputs > 64: GM_E_RANGE; a read length
 * whose windows do not fit the full-alignment kernel's LDS (gm_sw_full_cs_batch's admission test), or whose survivor capacity is beyond the LDS of the front's prune
 * kernel on this index (the front would fail there in mid-call; on a small index this binds first, near 900 colours under the default seeds): GM_E_RANGE.  The column
 * scratch of one post_sw thread holds 59 918 colours; the LDS tests admit no read of more than a few thousand, so that bound is subsumed by them (the entry still checks it).
 * n_reads <= 0: GM_OK, no hits.  After any failure *out holds nothing to free. */
typedef struct gm_read_mappings_cs {
  int32_t  n_reads, has_edit;                  /* reads of the call; 1: edit / edit_off are there (the session's extra_sam_fields) */
  uint64_t n_hits, n_maps, cigar_len, edit_len, ops_len;      /* entries of hits / recs / post, of maps; bytes of cigar, of edit, of ops and of qralign */
  gm_pass1_hit_t   *hits;  uint64_t *hit_off;  /* as gm_read_hits returns them; hit_off[n_reads + 1] */
  int32_t          *score_vector;              /* [n_hits] pass 1's score (ZV) */
  gm_sw_full_rec_t *recs;                      /* [n_hits] sw_full_cs's records (ZH = score) */
  gm_mapping_t     *maps;  uint64_t *map_off;  /* as gm_select_pass2 returns them; map_off[n_reads + 1] */
  char *cigar; uint64_t *cigar_off;            /* cigar_off[n_hits + 1] */
  char *edit;  uint64_t *edit_off;             /* has_edit: edit_off[n_hits + 1] */
  uint8_t *ops;                                /* want_ops: ops_len bytes */
  uint64_t post_quals_len;                     /* bytes of post_quals */
  gm_post_rec_t *post;                         /* [n_hits], or NULL without post_sw */
  char *post_quals;                            /* post_quals_len bytes */
  char *qralign;                               /* ops_len bytes */
} gm_read_mappings_cs_t;
int  gm_read_mappings_cs_size(void);     /* sizeof(gm_read_mappings_cs_t), for the Python mirror */
int  gm_read_mappings_cs(gm_session_t *s, int n_reads, int n_colours, const uint32_t *colours_packed, const uint8_t *initbp,
                         const char *quals, int qual_delta,       /* NULL, or '\n' separated QV strings as gm_map_reads_cs_fastq takes them */
                         int want_ops, gm_read_mappings_cs_t *out, gm_map_stats_t *stats);
void gm_read_mappings_cs_free(gm_read_mappings_cs_t *out);

/* gm_pair_mappings: paired pass 2 as a seam -- a chunk of read pairs to mapping arrays in one call; the paired counterpart of gm_read_mappings.  A caller who wants the
 * mappings of read pairs as data (to write BAM, filter by insert size, count, feed a variant caller) makes this call instead of gm_map_pairs and a SAM parser.  Letter
 * space; all four pair modes; half_paired 1 and 0; match_mode 4 and 3.  The mapping entries gm_map_pairs* do not use it and print what they printed.
 * The entry drives the call object of gm_map_pairs through its own stages and launches what gm_map_pairs launches: the front (lookup, the mate-pair region counts of
 * --no-half-paired and -n 3, anchors), pair-up, pass 1 over the paired windows, the pair top-K, the full alignment of the windows of the selected pairs at half the
 * threshold per mate (ref: gmapper.c:2677), the half-paired rescue (pass 1 over all windows with the windows of the final pairs saved, top-K, the full alignment at the
 * full threshold; ref: mapping.c:2598-2625), with the same sub-batch walk, capacity growth, re-dos and buffer-set pairs.  Two things differ from gm_map_pairs.
 *   The pair selection runs on the device, a wave a pair, a lane a candidate pair of the pair heap's list (at most 64), where gm_map_pairs runs a host loop.  Its rules
 *   are readpair_pass2's (ref: mapping.c:2181-2314):
 *     1. a candidate stays when both its windows were aligned (score_full != 0, :2243-2245) and score_full of mate 1 + score_full of mate 2 >= the pair threshold:
 *        -sw_full_threshold for an absolute threshold, else (int)(sum of the two score_max * (sw_full_threshold / 100.0)) -- evaluated by the host in that double
 *        expression, once per possible sum; the kernel reads the table (:2246-2262).  score_full is hit_run_post_sw's, from the host's libm as in gm_read_mappings.
 *     2. readpair_remove_duplicate_hits (:2113-2175): four passes of readpair_push_dominant_single_hits (:2083-2110) -- mate 1 by (cn, gen_st, genome_start), mate 1 by
 *        (cn, gen_st, -genome_start - rmapped + deletions - insertions), mate 2 by the first, mate 2 by the second.  A pass sorts the pairs stably by that key of that
 *        mate's window; within every run of equal keys each pair takes the window of the run's FIRST maximum score_full for that mate, and compute_paired_hit
 *        (:2053-2080) is evaluated again for it.
 *     3. a stable sort by (sort_idx of mate 1's window, sort_idx of mate 2's window) -- the comparator of :2004-2050 -- and of every run of equal neighbours only the
 *        first stays (removedups, common/util.c:1240-1255).
 *     4. a stable sort by descending key: pct_score = (1000 * 100 * score) / score_max of the sums, or the score for an absolute threshold.
 *     5. the cut to num_outputs, strata (the leading run of equal score), max_alignments (more than that many leaves none) (:2264-2284).
 *   And instead of text the call returns arrays.  The mapping qualities are compute_paired_mqv's (ref: output.c:811-942) and the records named are plan_pair_output's
 *   (ref: output.c:1086-1235, --single-best-mapping with the one improper pair of two unpaired winners included): the host functions gm_map_pairs prints through, called
 *   on the same objects -- erf, log and pow go through the host's libm, and the reference's bytes hang on their last bits.
 * Result: ONE struct, released by ONE call, gm_pair_mappings_free (frees the buffers and zeroes the struct; the struct itself is the caller's).  m = 0 / 1: mate 1 / 2.
 * Offset arrays are always there (n_pairs + 1 / n_hits[m] + 1 entries); an array of records or bytes is NULL when it would be empty.
 *   hits[m], hit_off[m][n_pairs + 1]   every window of mate m that went through the full alignment for the pair: the hits of the paired pass in the order of the pair
 *                     heap's window list, then the hits of the half-paired rescue in its heap's array order.  gm_pass1_hit_t as gm_read_hits fills it, with read = the
 *                     pair, score_vector / pct_score_vector = pass 2's second vector score (ZV), win = -1 and the anchor box 0 (the call has no window list to name).
 *   hit_kind[m][i]    0: a hit of the paired pass; 1: a hit of the rescue.
 *   recs[m][i]        the record as the pipeline's pass 2 leaves it; a window under its threshold -- half the threshold in the paired pass, the full one in the rescue
 *                     -- has the zero record.  genome_start counts on strand gen_st of the contig; ops_off / n_ops point into ops[m] whether or not it was asked for.
 *   pmaps, pmap_off[n_pairs + 1]   the paired mappings of each pair in the reference's output order, gm_pair_mapping_t below.
 *   umaps[m], umap_off[m][n_pairs + 1]   the unpaired (half-paired) mappings of mate m in output order, gm_mapping_t: read = the pair, hit = the index in hits[m] /
 *                     recs[m] (the call's, not the pair's), mqv from compute_paired_mqv's unpaired branch, z0 / z1 the Z0 / Z1 tags' values;
 *   umap_z45[m]       two doubles a mapping of umaps[m]: the values of its Z4 (pr_top_random) and Z5 (pr_missed_mp) tags.
 *                     In the SAM text a pair's records are: its paired mappings, then mate 1's unpaired ones (each with mate 2's unmapped record), then mate 2's.
 *   cigar[m], cigar_off[m][n_hits[m] + 1]  and, when has_edit (the session's extra_sam_fields), edit[m], edit_off[m]: the text of every hit that some mapping names, clip
 *                     character 'S', reverse = gen_st, made on the device over those hits only; every other hit has an empty slice.
 *   ops[m], ops_len[m]   want_ops != 0 only: the edit operations of all records of mate m, compacted in hit order (else NULL; ops_len is still their total).
 * stats (or NULL): as gm_map_pairs fills it; sam_records stays 0.
 * Refusals, on the host before anything is uploaded, the session usable afterwards: s or out NULL, n_pairs < 0, a length < 1, a missing mate array: GM_E_ARG; a
 * colour-space session, output_format 1 / 2, match_mode 2: GM_E_ARG with a message; num_tmp_outputs > 64: GM_E_RANGE (as gm_select_pass2); then every refusal of
 * gm_map_pairs by the same functions with the same codes: pair_mode outside 1..4 and match_mode outside 2..4 GM_E_ARG, a read length out of range or a window beyond
 * pass 2's LDS for either mate GM_E_RANGE.  n_pairs == 0: GM_OK, no hits.  After any failure *out holds nothing to free. */
typedef struct gm_pair_mapping {     /* 12 x 32 bits + 8 doubles = 112 bytes, no padding */
  int32_t pair;
  int32_t hit[2];                    /* the mates' hits, as indices into the PAIR's OWN slices: hits[m][hit_off[m][pair] + hit[m]] */
  int32_t score, pct_score, key;     /* compute_paired_hit's sums; an improper pair: score = the sum of the two AS, pct_score = key = 0 */
  int32_t insert_size;               /* signed as compute_paired_hit signs it; an improper pair: 0 */
  int32_t mapq[2], as[2];            /* MAPQ and AS of the two records */
  int32_t improper;                  /* 1: the pair of two unpaired winners --single-best-mapping --all-contigs prints (FLAG without 0x2); hit[] then name rescue hits */
  double  z[2][4];                   /* per mate, the values of the Z tags its record prints: proper Z2 Z3 Z4 Z6; improper Z0 Z1 Z4 Z5.  0 without mapping qualities */
} gm_pair_mapping_t;
typedef struct gm_pair_mappings {
  int32_t  n_pairs, has_edit;
  uint64_t n_hits[2], n_pmaps, n_umaps[2], cigar_len[2], edit_len[2], ops_len[2];
  gm_pass1_hit_t    *hits[2];  uint64_t *hit_off[2];  uint8_t *hit_kind[2];
  gm_sw_full_rec_t  *recs[2];
  gm_pair_mapping_t *pmaps;    uint64_t *pmap_off;
  gm_mapping_t      *umaps[2]; uint64_t *umap_off[2]; double *umap_z45[2];
  char *cigar[2]; uint64_t *cigar_off[2];
  char *edit[2];  uint64_t *edit_off[2];
  uint8_t *ops[2];
} gm_pair_mappings_t;
int  gm_pair_mapping_size(void);         /* sizeof(gm_pair_mapping_t), for the Python mirror */
int  gm_pair_mappings_size(void);        /* sizeof(gm_pair_mappings_t), for the Python mirror */
int  gm_pair_mappings(gm_session_t *s, int n_pairs, int len1, const uint32_t *mates1_packed, int len2, const uint32_t *mates2_packed,
                      const gm_pair_opts_t *opts, int want_ops, gm_pair_mappings_t *out, gm_map_stats_t *stats);
void gm_pair_mappings_free(gm_pair_mappings_t *out);
/* test hook: the device pair selection of gm_pair_mappings beside the host loop of gm_map_pairs on hand-made candidate lists, under the session's num_outputs, strata,
 * max_alignments and sw_full_threshold.  wins0 / wins1: 9 x int32 a window (cn, gen_st, genome_start, rmapped, deletions, insertions, score_full, score_max, sort_idx),
 * pair pr's cnt0[pr] / cnt1[pr] windows one after the other; plist[pr * 64 ..]: its pcnt[pr] candidates (window of mate 1 << 8) | window of mate 2.  dev_out / host_out:
 * n_pairs x 64 words in the same form, dev_cnt / host_cnt: n_pairs counts. */
int  gm_debug_pair_select(gm_session_t *s, int pair_mode, int n_pairs, const uint32_t *cnt0, const int32_t *wins0, const uint32_t *cnt1, const int32_t *wins1,
                          const uint32_t *plist, const uint32_t *pcnt, uint32_t *dev_out, uint32_t *dev_cnt, uint32_t *host_out, uint32_t *host_cnt);

/* time of the dominant kernel (seed lookup) during the last gm_map_* call, from HIP events on the
 * session's own stream, and the algorithmic bytes it moved */
int gm_last_lookup_timing(gm_session_t *s, double *ms, uint64_t *alg_bytes, int *launches);
/* name of the seed-lookup kernel the last mapping call launched (k_lookup_bkt / k_lookup_v4 / k_lookup_v3 / k_lookup): what the roofline figures refer to */
const char *gm_last_lookup_kernel(void);
/* name of the pass-2 (full alignment) kernel the calling thread's last launch chose: letter space k_pass2_g4<16,int> (four windows a wave), k_pass2_g4<8,int16_t> (tuning
 * builds) or k_pass2 (one window); colour space k_pass2_cs_g4<8,int16_t>, k_pass2_cs_g4<16,int> or k_pass2_cs.  "" before the first launch. */
const char *gm_last_pass2_kernel(void);

#ifdef __cplusplus
}
#endif
#endif
