// The seed lookup's plan on the CPU: shrimp_amd/csrc/gm_lookup_plan.h decides which K1 kernel runs for a batch and in what shape, on plain numbers, before anything
// is allocated or launched.  This program pins that decision for the shapes DESIGN.md section 5 argues from -- 100-base, 50-colour and 2 x 150-base reads on 3 Gbp, a
// bucket-sized genome, few entries on many slabs, the forced variants of tests/test_gpu_parity.py, the switches of a call, both sides of the two entry thresholds.
// The rows were recorded from the launch code as it stood before the plan existed (its if / else chain and the two "try" launchers, run with the device calls
// stubbed out), not from this header: a change of a threshold, of an arm's place in the order or of a shape formula shows here, without a GPU.
//
// An index is described as gm_index_build leaves it for an i.i.d. genome of `len` bases under the default seeds (both spaces use them): one list entry a position
// and seed, the automatic cutoff, slabs of min(2^29, the genome) positions unless GM_SLAB_BITS says otherwise, buckets and strip lists where the two predicates of
// the plan header grant them.  A call with the fuse request offers the prune rules with a window of 1.4 read lengths and e_max = 0.55 read lengths - 20.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include "gm_lookup_plan.h"

struct Row {
  const char* what; double len; int colour, hflag, region_bits, read_len, n_reads, fuse, mode;      // mode: 1 .. 7 the mate-pair mode, 8 no region counts
  const char* env;                                                                                   // knobs of the tuning build, NAME=value,...
  const char* kernel; const char* shape; int redo_mp;                                               // what gm_last_lookup_kernel names, the shape, MP of the heavy tier's re-run
  const char* seeds;                                                                                 // a seed set of SEED_SETS below, comma separated strings, or null: the three defaults
};
// the seed sets of tests/oracle_api.py SEED_SETS that have rows here
#define SEEDS_REF_W16H "111111101110111111,1111100101101101011111,11110011001010100011011111,111101001100000100110011010111"
#define SEEDS_ONE "11110111101111"
#define SEEDS_SIXTEEN "110111111111,1010111111111,11101010111111,1110011011101011,11110110011100101,111010110011010011,11011010011110100001,100001011110010011101," \
                      "1100100011110001011001,111010011101000010000011,1010100011101000000110011,11100100000100011110100001,1001000010101011010000010101," \
                      "10000001100001000000011111011,110001100111000001000000001011,10001001100001010010001010010001"
static const Row ROWS[] = {
  {"100-base reads on 3 Gbp: v5, full shape, one round, prune rules fused", 3000000000, 0, 0, 11, 100, 131072, 1, 0, "", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=1464844 grid=256 lds=156056 prune=1 D=140 e_max=35", 0},
  {"the same without a fuse request", 3000000000, 0, 0, 11, 100, 131072, 0, 0, "", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=1464844 grid=256 lds=156056 prune=0 D=100 e_max=-1", 0},
  {"a small batch: the grid is the read-strands", 3000000000, 0, 0, 11, 100, 100, 1, 0, "", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=1464844 grid=200 lds=156056 prune=1 D=140 e_max=35", 0},
  {"50-colour reads on 3 Gbp: v5, the small shape (512 threads, two workgroups a CU)", 3000000000, 1, 0, 11, 50, 131072, 1, 0, "", "k_lookup_v5", "v5 lsw=14 ltw=11 hbits=12 cand_cap=2720 cand_limit=2712 xrec=64 threads=512 half=0 small=1 rounds=1 round_regs=1464844 grid=512 lds=78632 prune=1 D=70 e_max=7", 0},
  {"... GM_K5_SMALL=0: the full shape", 3000000000, 1, 0, 11, 50, 131072, 1, 0, "GM_K5_SMALL=0", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=1464844 grid=256 lds=152360 prune=1 D=70 e_max=7", 0},
  {"... GM_K5_HALF=1: k_lookup_v5_half", 3000000000, 1, 0, 11, 50, 131072, 1, 0, "GM_K5_HALF=1", "k_lookup_v5_half", "v5 lsw=14 ltw=11 hbits=12 cand_cap=2720 cand_limit=2712 xrec=64 threads=512 half=1 small=1 rounds=1 round_regs=1464844 grid=512 lds=78632 prune=1 D=70 e_max=7", 0},
  {"75-colour reads on 3 Gbp: too many candidates for the small shape", 3000000000, 1, 0, 11, 75, 131072, 1, 0, "", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=1464844 grid=256 lds=154192 prune=1 D=105 e_max=21", 0},
  {"150-base reads on 3 Gbp (pairs): k_lookup_v5_rounds, two rounds", 3000000000, 0, 0, 11, 150, 131072, 1, 0, "", "k_lookup_v5_rounds", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=16 threads=1024 half=0 small=0 rounds=2 round_regs=732422 grid=256 lds=158600 prune=1 D=210 e_max=62", 0},
  {"200-base reads on 3 Gbp: four rounds", 3000000000, 0, 0, 11, 200, 4096, 1, 0, "", "k_lookup_v5_rounds", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=16 threads=1024 half=0 small=0 rounds=4 round_regs=366211 grid=256 lds=162296 prune=1 D=280 e_max=90", 0},
  {"300-base reads on 3 Gbp: more lists than threads, v5 declines, v4", 3000000000, 0, 0, 11, 300, 4096, 1, 0, "", "k_lookup_v4", "v4 tab_bits=19 cbits=29 SC=6 wcap=4096 bin_cap=4096 threads=1024 grid=256 lds=156832", 0},
  {"280-base reads on 300 Mbp, regions of 512 positions: the prune rules (392 + 134 positions) do not fit a region, v5 without them", 300000000, 0, 0, 9, 280, 4096, 1, 0, "GM_SLAB_BITS=27", "k_lookup_v5", "v5 lsw=14 ltw=11 hbits=12 cand_cap=2720 cand_limit=2712 xrec=16 threads=1024 half=0 small=0 rounds=1 round_regs=585938 grid=256 lds=94488 prune=0 D=392 e_max=-1", 0},
  {"... regions of 1 024: they fit", 300000000, 0, 0, 10, 280, 4096, 1, 0, "GM_SLAB_BITS=27", "k_lookup_v5", "v5 lsw=14 ltw=11 hbits=12 cand_cap=2720 cand_limit=2712 xrec=16 threads=1024 half=0 small=0 rounds=1 round_regs=292969 grid=256 lds=94488 prune=1 D=392 e_max=134", 0},
  {"a bucket-sized genome: the persistent bucket kernel", 2000000, 0, 0, 11, 100, 4096, 1, 0, "", "k_lookup_bkt", "bkt persistent=1 threads=320 lds=368 lds_p=480", 0},
  {"... GM_BKT_V1: one workgroup a read-strand", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_BKT_V1=1", "k_lookup_bkt", "bkt persistent=0 threads=320 lds=368 lds_p=480", 0},
  {"... region size 256: the persistent form's LDS", 2000000, 0, 0, 8, 100, 4096, 1, 0, "", "k_lookup_bkt", "bkt persistent=1 threads=320 lds=2080 lds_p=2192", 0},
  {"... 200-base reads: more than 512 lists, no bucket kernel", 2000000, 0, 0, 11, 200, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=11680", 0},
  {"... GM_NO_BUCKETS (the index has none): v3", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_NO_BUCKETS=1", "k_lookup_v3", "v3 threads=768 lds=5584", 0},
  {"460 Mbp, one slab, too many entries a list for buckets, no strip lists: v3", 460000000, 0, 0, 11, 100, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=61488", 0},
  {"few entries on many slabs: v3", 1000000000, 0, 0, 11, 25, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=66528", 0},
  {"2 Mbp cut into 8 slabs: v3", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18", "k_lookup_v3", "v3 threads=768 lds=16352", 0},
  {"... v4 forced", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18,GM_K1_V4=1", "k_lookup_v4", "v4 tab_bits=19 cbits=18 SC=8 wcap=4096 bin_cap=4096 threads=1024 grid=256 lds=144656", 0},
  {"... v4 forced, small table, 128 threads", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=13,GM_K1_V4=1,GM_K4_TABBITS=12,GM_K1_THREADS=128", "k_lookup_v4", "v4 tab_bits=12 cbits=13 SC=245 wcap=4096 bin_cap=4096 threads=128 grid=256 lds=15552", 0},
  {"... v4 forced, small bins", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18,GM_K1_V4=1,GM_K4_BINCAP=16,GM_K4_WCAP=8", "k_lookup_v4", "v4 tab_bits=19 cbits=18 SC=8 wcap=8 bin_cap=16 threads=1024 grid=256 lds=136480", 0},
  {"... v5 forced", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18,GM_K1_V5=1", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=977 grid=256 lds=156056 prune=1 D=140 e_max=35", 0},
  {"... v5 forced, tiny tables", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18,GM_K1_V5=1,GM_K5_LSW=9", "k_lookup_v5", "v5 lsw=9 ltw=6 hbits=7 cand_cap=80 cand_limit=72 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=977 grid=256 lds=10904 prune=1 D=140 e_max=35", 0},
  {"... v5 forced, three rounds", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18,GM_K1_V5=1,GM_K5_ROUNDS=3", "k_lookup_v5_rounds", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=3 round_regs=326 grid=256 lds=156056 prune=1 D=140 e_max=35", 0},
  {"... v5 forced, half-size shape without the Bloom bits, four rounds", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18,GM_K1_V5=1,GM_K5_HALF=2,GM_K5_ROUNDS=4", "k_lookup_v5_half", "v5 lsw=14 ltw=11 hbits=12 cand_cap=2720 cand_limit=2712 xrec=25 threads=512 half=2 small=0 rounds=4 round_regs=245 grid=512 lds=81392 prune=1 D=140 e_max=35", 0},
  {"... the slab-sweep kernel forced", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18,GM_K1_V2=1", "k_lookup", "sweep mp=0 threads=320 lds=6416", 0},
  {"v4 forced on 3 Gbp", 3000000000, 0, 0, 11, 100, 131072, 1, 0, "GM_K1_V4=1", "k_lookup_v4", "v4 tab_bits=19 cbits=29 SC=6 wcap=4096 bin_cap=4096 threads=1024 grid=256 lds=144640", 0},
  {"3 Gbp, 31-base reads: 7 868 expected entries, below v5's 8 000", 3000000000, 0, 0, 11, 31, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=68304", 0},
  {"3 Gbp, 32-base reads: 8 404 expected entries, v5", 3000000000, 0, 0, 11, 32, 4096, 1, 0, "", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=1464844 grid=256 lds=151000 prune=1 D=44 e_max=-3", 0},
  {"3 Gbp without v5, 72-base reads: 29 861 expected entries, below v4's 30 000", 3000000000, 0, 0, 11, 72, 4096, 1, 0, "GM_NO_V5=1", "k_lookup_v3", "v3 threads=768 lds=74496", 0},
  {"3 Gbp without v5, 73-base reads: 30 398 expected entries, v4", 3000000000, 0, 0, 11, 73, 4096, 1, 0, "GM_NO_V5=1", "k_lookup_v4", "v4 tab_bits=19 cbits=29 SC=6 wcap=4096 bin_cap=4096 threads=1024 grid=256 lds=142992", 0},
  {"hashed seeds on 3 Gbp", 3000000000, 0, 1, 11, 100, 4096, 1, 0, "", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=1464844 grid=256 lds=156056 prune=1 D=140 e_max=35", 0},
  {"no region counts (-n 1): the slab-sweep kernel, MP 6", 3000000000, 0, 0, 11, 100, 4096, 0, 8, "", "k_lookup", "sweep mp=6 threads=320 lds=71920", 6},
  {"... on a bucket-sized genome", 2000000, 0, 0, 11, 60, 4096, 0, 8, "", "k_lookup", "sweep mp=6 threads=192 lds=3712", 6},
  {"mate-pair mode 1", 3000000000, 0, 0, 11, 150, 4096, 0, 1, "", "k_lookup", "sweep mp=1 threads=448 lds=141120", 0},
  {"mate-pair mode 2", 3000000000, 0, 0, 11, 150, 4096, 0, 2, "", "k_lookup", "sweep mp=2 threads=448 lds=141120", 2},
  {"mate-pair mode 3", 3000000000, 0, 0, 11, 150, 4096, 0, 3, "", "k_lookup", "sweep mp=3 threads=448 lds=141120", 0},
  {"mate-pair mode 4", 3000000000, 0, 0, 11, 150, 4096, 0, 4, "", "k_lookup", "sweep mp=4 threads=448 lds=141120", 4},
  {"mate-pair mode 5", 3000000000, 0, 0, 11, 150, 4096, 0, 5, "", "k_lookup", "sweep mp=5 threads=448 lds=141120", 5},
  {"mate-pair mode 7 runs as 2", 3000000000, 0, 0, 11, 150, 4096, 0, 7, "", "k_lookup", "sweep mp=2 threads=448 lds=141120", 0},
  {"mate-pair mode 2, 60-base reads on 2 Mbp: at least 256 threads", 2000000, 0, 0, 11, 60, 4096, 0, 2, "", "k_lookup", "sweep mp=2 threads=256 lds=69248", 2},  // Other seed sets (tests/oracle_api.py SEED_SETS), recorded from the plan as it stood when tests/test_seed_sets.py was written and read against gm_lookup_plan.h:
  // NL = seeds x (read length - shortest span + 1).  sixteen: no bucket kernel (NL > 512); on 3 Gbp v5 would need more than four rounds and declines, at 70 bases v4
  // takes over, at 100 bases v4's LDS does not fit and the automatic cutoff (71 525) is past v3's 65 535: the slab sweep.
  {"the reference's weight-16 -H set (spans 18 to 30), 100-base reads, a bucket-sized genome", 2000000, 0, 1, 11, 100, 4096, 1, 0, "", "k_lookup_bkt", "bkt persistent=1 threads=384 lds=368 lds_p=480", 0, SEEDS_REF_W16H},
  {"the reference's weight-16 -H set (spans 18 to 30), 100-base reads, 2 Mbp in 8 slabs", 2000000, 0, 1, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18", "k_lookup_v3", "v3 threads=768 lds=20752", 0, SEEDS_REF_W16H},
  {"the reference's weight-16 -H set (spans 18 to 30), 100-base reads, 3 Gbp", 3000000000, 0, 1, 11, 100, 4096, 1, 0, "", "k_lookup_v5_rounds", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=2 round_regs=732422 grid=256 lds=157760 prune=1 D=140 e_max=35", 0, SEEDS_REF_W16H},
  {"sixteen seeds, 70-base reads: 944 lists, a bucket-sized genome", 2000000, 0, 0, 11, 70, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=19216", 0, SEEDS_SIXTEEN},
  {"sixteen seeds, 70-base reads: 944 lists, 2 Mbp in 8 slabs", 2000000, 0, 0, 11, 70, 4096, 1, 0, "GM_SLAB_BITS=18", "k_lookup_v3", "v3 threads=768 lds=58672", 0, SEEDS_SIXTEEN},
  {"sixteen seeds, 70-base reads: 944 lists, 3 Gbp", 3000000000, 0, 0, 11, 70, 4096, 1, 0, "", "k_lookup_v4", "v4 tab_bits=19 cbits=29 SC=6 wcap=4096 bin_cap=4096 threads=1024 grid=256 lds=158272", 0, SEEDS_SIXTEEN},
  {"sixteen seeds, 100-base reads: 1 424 lists, more than a workgroup has threads, a bucket-sized genome", 2000000, 0, 0, 11, 100, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=28848", 0, SEEDS_SIXTEEN},
  {"sixteen seeds, 100-base reads: 1 424 lists, more than a workgroup has threads, 2 Mbp in 8 slabs", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18", "k_lookup_v3", "v3 threads=768 lds=88464", 0, SEEDS_SIXTEEN},
  {"sixteen seeds, 100-base reads: 1 424 lists, more than a workgroup has threads, 3 Gbp", 3000000000, 0, 0, 11, 100, 4096, 1, 0, "", "k_lookup", "sweep mp=0 threads=1024 lds=99840", 0, SEEDS_SIXTEEN},
  {"one seed, 100-base reads: 87 lists, a bucket-sized genome", 2000000, 0, 0, 11, 100, 4096, 1, 0, "", "k_lookup_bkt", "bkt persistent=1 threads=128 lds=368 lds_p=480", 0, SEEDS_ONE},
  {"one seed, 100-base reads: 87 lists, 2 Mbp in 8 slabs", 2000000, 0, 0, 11, 100, 4096, 1, 0, "GM_SLAB_BITS=18", "k_lookup_v3", "v3 threads=768 lds=5568", 0, SEEDS_ONE},
  {"one seed, 100-base reads: 87 lists, 3 Gbp", 3000000000, 0, 0, 11, 100, 4096, 1, 0, "", "k_lookup_v5", "v5 lsw=15 ltw=12 hbits=13 cand_cap=5456 cand_limit=5448 xrec=64 threads=1024 half=0 small=0 rounds=1 round_regs=1464844 grid=256 lds=151880 prune=1 D=140 e_max=35", 0, SEEDS_ONE},
  {"default seeds, 183-base reads on a bucket-sized genome: 510 lists (3 x 170), the last length with the bucket kernel", 2000000, 0, 0, 11, 183, 4096, 1, 0, "", "k_lookup_bkt", "bkt persistent=1 threads=512 lds=448 lds_p=640", 0, nullptr},
  {"default seeds, 184-base reads on a bucket-sized genome: 513 lists: no bucket kernel", 2000000, 0, 0, 11, 184, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=10704", 0, nullptr},
  {"default seeds, 187-base reads on a bucket-sized genome: 522 lists", 2000000, 0, 0, 11, 187, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=10896", 0, nullptr},
  {"default seeds, 188-base reads on a bucket-sized genome: 525 lists", 2000000, 0, 0, 11, 188, 4096, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=10960", 0, nullptr},
  // Long reads on the 148 323 bases of tests/golden/long_genome.npz (tests/test_long_reads.py), recorded through the query mode below: the bucket kernel up to 183 bases
  // (3 x 170 = 510 lists), v3 from 184 on -- 2 961 lists at 1 000 bases, 3 932 under the weight-16 -H set -- and the slab sweep where no region counts or mate-pair counts run
  {"long genome, 128 bases", 148323, 0, 0, 11, 128, 200, 1, 0, "", "k_lookup_bkt", "bkt persistent=1 threads=384 lds=160 lds_p=288", 0, nullptr},
  {"long genome, 129 bases", 148323, 0, 0, 11, 129, 200, 1, 0, "", "k_lookup_bkt", "bkt persistent=1 threads=384 lds=176 lds_p=320", 0, nullptr},
  {"long genome, 183 bases: the last length with the bucket kernel", 148323, 0, 0, 11, 183, 200, 1, 0, "", "k_lookup_bkt", "bkt persistent=1 threads=512 lds=224 lds_p=416", 0, nullptr},
  {"long genome, 184 bases: 513 lists, v3", 148323, 0, 0, 11, 184, 200, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=10480", 0, nullptr},
  {"long genome, 184 bases, -n 1: the slab sweep", 148323, 0, 0, 11, 184, 200, 1, 8, "", "k_lookup", "sweep mp=6 threads=576 lds=12544", 6, nullptr},
  {"long genome, 257 bases", 148323, 0, 0, 11, 257, 200, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=14944", 0, nullptr},
  {"long genome, 257 bases, the weight-16 -H set: 960 lists", 148323, 0, 1, 11, 257, 200, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=19504", 0, SEEDS_REF_W16H},
  {"long genome, 400 bases: 1 161 lists", 148323, 0, 0, 11, 400, 100, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=23664", 0, nullptr},
  {"long genome, 400 bases, -n 1", 148323, 0, 0, 11, 400, 100, 1, 8, "", "k_lookup", "sweep mp=6 threads=1024 lds=28304", 6, nullptr},
  {"long genome, 1 000 bases: 2 961 lists", 148323, 0, 0, 11, 1000, 40, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=60256", 0, nullptr},
  {"long genome, 1 000 bases, the weight-16 -H set: 3 932 lists", 148323, 0, 1, 11, 1000, 40, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=79680", 0, SEEDS_REF_W16H},
  {"long genome, 204 colours", 148323, 1, 0, 11, 204, 200, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=11712", 0, nullptr},
  {"long genome, 205 colours", 148323, 1, 0, 11, 205, 200, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=11776", 0, nullptr},
  {"long genome, 1 000 colours", 148323, 1, 0, 11, 1000, 30, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=60256", 0, nullptr},
  {"long genome, mates of 250 bases, unpaired form", 148323, 0, 0, 11, 250, 100, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=14512", 0, nullptr},
  {"long genome, mates of 250 bases, mate-pair mode 1", 148323, 0, 0, 11, 250, 100, 1, 1, "", "k_lookup", "sweep mp=1 threads=768 lds=82896", 0, nullptr},
  {"long genome, mates of 700 bases, unpaired form", 148323, 0, 0, 11, 700, 40, 1, 0, "", "k_lookup_v3", "v3 threads=768 lds=41968", 0, nullptr},
  {"long genome, mates of 700 bases, mate-pair mode 1", 148323, 0, 0, 11, 700, 40, 1, 1, "", "k_lookup", "sweep mp=1 threads=1024 lds=115744", 0, nullptr},
};

static std::map<std::string, std::string> g_env;
static const char* env_get(const char* name) { auto it = g_env.find(name); return it == g_env.end() ? nullptr : it->second.c_str(); }

static K1PlanIn plan_in(const Row& r, const K1Tune& t) {
  const std::string set = r.seeds && *r.seeds ? r.seeds : "11110111101111,1111011100100001111,1111000011001101111";
  K1PlanIn in = K1PlanIn();
  in.total_len = (uint64_t)r.len; in.colour = r.colour; in.hflag = r.hflag; in.region_bits = r.region_bits; in.region_overlap = 50;
  in.n_seeds = 0; in.min_seed_span = 64;
  int max_weight = 0;
  for (size_t a = 0; a < set.size() && in.n_seeds < K1P_MAX_SEEDS;) {
    size_t e = set.find(',', a); if (e == std::string::npos) e = set.size();
    const std::string sd = set.substr(a, e - a); a = e + 1;
    int w = 0; for (char c : sd) w += c == '1';
    const int i = in.n_seeds++;
    in.seed[i].span = (int)sd.size(); in.seed[i].weight = w; in.seed[i].n_pos = (uint32_t)(r.len - in.seed[i].span + 1);
    in.min_seed_span = std::min(in.min_seed_span, in.seed[i].span); max_weight = std::max(max_weight, w);
  }
  // the automatic cutoff and the lists of a seed: 4^weight, 4^12 with -H (index_tables, add_seed of gm_host.hip)
  const int cut_bits = 2 * (r.hflag ? K1P_HASH_TABLE_POWER : max_weight), list_bits = 2 * (r.hflag ? K1P_HASH_TABLE_POWER : in.seed[0].weight);
  in.list_cutoff = std::max<uint32_t>(1000u, (uint32_t)((100ull * in.total_len) >> cut_bits));
  int bits = 12; while ((1ull << bits) < in.total_len) bits++;
  in.slab_bits = std::min(bits, 29);
  if (const char* e = env_get("GM_SLAB_BITS")) in.slab_bits = std::max(r.region_bits + 2, std::min(31, atoi(e)));
  in.n_slabs = std::max(1, (int)((in.total_len + (1ull << in.slab_bits) - 1) >> in.slab_bits));
  in.has_buckets = k1_buckets_allowed(in.n_slabs, t) && (double)in.seed[0].n_pos / (double)(1ull << list_bits) <= 12.0;
  in.has_strips = k1_strips_wanted(in.n_slabs, in.region_bits, t);
  in.no_region_counts = r.mode == 8; in.mp_mode = r.mode < 8 ? r.mode : 0;
  in.n_reads = r.n_reads; in.read_len = r.read_len;
  in.want_fuse = r.fuse != 0; in.window_len = r.fuse ? r.read_len * 14 / 10 : 0; in.e_max = r.fuse ? r.read_len * 55 / 100 - 20 : -1;
  in.cus = 256;
  return in;
}

static std::string shape_of(const K1Plan& p, K1Variant v) {
  char b[512];
  switch (v) {
    case K1_V5: { const K5Shape& s = p.v5;
      snprintf(b, sizeof b, "v5 lsw=%d ltw=%d hbits=%d cand_cap=%d cand_limit=%d xrec=%d threads=%d half=%d small=%d rounds=%d round_regs=%u grid=%d lds=%zu prune=%d D=%u e_max=%d",
               s.lsw, s.ltw, s.hbits, s.cand_cap, s.cand_limit, s.xrec, s.threads, s.half, (int)s.small_shape, s.rounds, s.round_regs, s.grid, s.lds, (int)s.prune, s.D, s.e_max);
      break; }
    case K1_V4: { const K4Shape& s = p.v4;
      snprintf(b, sizeof b, "v4 tab_bits=%d cbits=%d SC=%d wcap=%d bin_cap=%d threads=%d grid=%d lds=%zu", s.tab_bits, s.cbits, s.SC, s.wcap, s.bin_cap, s.threads, s.grid, s.lds);
      break; }
    case K1_V3: snprintf(b, sizeof b, "v3 threads=%d lds=%zu", p.threads3, p.lds3); break;
    case K1_BKT: snprintf(b, sizeof b, "bkt persistent=%d threads=%d lds=%zu lds_p=%zu", (int)p.bkt.persistent, p.bkt.threads, p.bkt.lds, p.bkt.lds_p); break;
    default: snprintf(b, sizeof b, "sweep mp=%d threads=%d lds=%zu", p.sweep_mp, p.sweep_threads, p.sweep_lds); break;
  }
  return b;
}

static void read_env(const char* env) {
  g_env.clear();
  for (std::string e = env; !e.empty();) {
    const size_t q = e.find(','); const std::string kv = e.substr(0, q); const size_t eq = kv.find('=');
    g_env[kv.substr(0, eq)] = kv.substr(eq + 1);
    e = q == std::string::npos ? "" : e.substr(q + 1);
  }
}

// query <bases> <colour> <hflag> <read_len> <n_reads> <mode> <NAME=value;...|-> <seeds,...>: the kernel the plan names for one shape, for the tests that hold
// gm_last_lookup_kernel() to it (tests/test_seed_sets.py)
static int query(char** a) {
  std::string env = a[6]; if (env == "-") env = ""; for (char& c : env) if (c == ';') c = ',';
  read_env(env.c_str());
  const Row r = {"query", atof(a[0]), atoi(a[1]), atoi(a[2]), 11, atoi(a[3]), atoi(a[4]), 1, atoi(a[5]), "", "", "", 0, a[7]};
  const K1Tune t = k1_tune_read(env_get);
  const K1PlanIn in = plan_in(r, t);
  const K1Plan p = k1_plan(in, t);
  printf("%s | %s | NL=%d slabs=%d\n", p.n ? k1_variant_name(p, p.order[0]) : "", p.n ? shape_of(p, p.order[0]).c_str() : "", p.g.NL, in.n_slabs);
  return p.n ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc == 10 && !strcmp(argv[1], "query")) return query(argv + 2);
  int bad = 0, n = 0;
  for (const Row& r : ROWS) {
    read_env(r.env);
    const K1Tune t = k1_tune_read(env_get);
    const K1PlanIn in = plan_in(r, t);
    const K1Plan p = k1_plan(in, t);
    n++;
    bool ok = p.n >= 1 && p.n <= 3 && (p.order[p.n - 1] == K1_SWEEP || p.order[p.n - 1] == K1_V3 || p.order[p.n - 1] == K1_BKT);      // the last variant of a plan needs no scratch
    for (int i = 0; ok && i + 1 < p.n; i++) ok = p.order[i] == K1_V5 || p.order[i] == K1_V4;                                            // ... the ones before it may fail to get theirs
    const std::string kernel = p.n ? k1_variant_name(p, p.order[0]) : "", shape = p.n ? shape_of(p, p.order[0]) : "";
    if (!ok || kernel != r.kernel || shape != r.shape || k1_redo_mp(in.no_region_counts, in.mp_mode) != r.redo_mp) {
      bad++;
      printf("FAIL %s [%s]\n  want %s | %s | redo MP %d\n  got  %s | %s | redo MP %d (%d variants)\n", r.what, r.env, r.kernel, r.shape, r.redo_mp, kernel.c_str(), shape.c_str(),
             k1_redo_mp(in.no_region_counts, in.mp_mode), p.n);
    }
  }
  // the release build: no knob is set whatever the environment says
  { const K1Tune t = k1_tune_read([](const char*) -> const char* { return nullptr; });
    if (t.v2 || t.v3 || t.v4 || t.v5 || t.no_v5 || t.no_buckets || t.bkt_v1 || t.threads.set || t.ablate.set || t.ablate.v || t.k5_half.set || t.k4_tabbits.set) { bad++; printf("FAIL defaults\n"); } }
  printf("%d rows, %d failed\n", n, bad);
  if (!bad) printf("lookup plan ok\n");
  return bad ? 1 : 0;
}
