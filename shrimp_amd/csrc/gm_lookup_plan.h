// gm_lookup_plan.h -- which seed-lookup kernel (K1) runs for a batch, and in what shape: decided here, on plain numbers, before anything is allocated or launched.
// Nothing of HIP in this file: tests/host/lookup_plan_main.cpp pins the plan with plain g++, no GPU.  gm_launch_lookup (gm_lookup.hip) fills K1PlanIn from the index and
// the call, reads K1Tune, calls k1_plan and launches what it says; the kernels and their LDS layouts are described where they are (gm_lookup.hip, gm_lookup5.hip).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#define K1P_MAX_SEEDS 16            // = GM_MAX_SEEDS
#define K1P_HASH_TABLE_POWER 12     // = GM_HASH_TABLE_POWER
#define K1P_MP_CAP 8192             // = GM_MP_CAP
#define K1P_LDS (160 * 1024)        // LDS of a CU
#define K1_THREADS 256              // threads of the slab-sweep kernel in redo and list mode
#define K5_MAX_ROUNDS 4
#define K5_CTRL_WORDS 16            // = C_WORDS of gm_lookup5.hip

// what the decision reads
struct K1PlanIn {
  uint64_t total_len; int slab_bits, n_slabs, region_bits, region_overlap; uint32_t list_cutoff; int colour, hflag, no_region_counts, mp_mode;
  int n_seeds, min_seed_span; struct { int span, weight; uint32_t n_pos; } seed[K1P_MAX_SEEDS];
  bool has_buckets, has_strips;       // seed[0].bkt / seed[0].sdir of the index view
  int n_reads, read_len, cus;
  bool want_fuse; int window_len, e_max;      // the caller allows K1b's prune rules inside the lookup (GmFusePrune with scap2 > 0)
};

// A knob of the tuning build: set or not, and atoi of its text.  The release build leaves every knob unset.
struct K1Knob { bool set = false; int v = 0; };
struct K1Tune {
  bool v2 = false, v3 = false, v4 = false, v5 = false, no_v5 = false, no_buckets = false, bkt_v1 = false;      // GM_K1_V2 .. GM_K1_V5, GM_NO_V5, GM_NO_BUCKETS, GM_BKT_V1
  K1Knob threads, ablate, bkt_per_cu;                                                                        // GM_K1_THREADS, GM_K1_ABLATE, GM_BKT_PER_CU
  K1Knob k4_tabbits, k4_wcap, k4_bincap, k4_lds_pad, k4_wgs, k4_grid;                                        // GM_K4_*
  K1Knob k5_lsw, k5_small, k5_half, k5_half_threads, k5_rounds, k5_candlimit, k5_grid, k5_wlist;             // GM_K5_*
};
// get(name): the knob's text or null (gm_tune).  Read at the top of every call, never kept: the variant tests change the environment between the sessions of a process.
template <class Get> static inline K1Tune k1_tune_read(Get get) {
  K1Tune t;
  auto flag = [&](const char* name) { return get(name) != nullptr; };
  auto knob = [&](const char* name) { K1Knob k; if (const char* e = get(name)) { k.set = true; k.v = atoi(e); } return k; };
  t.v2 = flag("GM_K1_V2"); t.v3 = flag("GM_K1_V3"); t.v4 = flag("GM_K1_V4"); t.v5 = flag("GM_K1_V5"); t.no_v5 = flag("GM_NO_V5"); t.no_buckets = flag("GM_NO_BUCKETS"); t.bkt_v1 = flag("GM_BKT_V1");
  t.threads = knob("GM_K1_THREADS"); t.ablate = knob("GM_K1_ABLATE"); t.bkt_per_cu = knob("GM_BKT_PER_CU");
  t.k4_tabbits = knob("GM_K4_TABBITS"); t.k4_wcap = knob("GM_K4_WCAP"); t.k4_bincap = knob("GM_K4_BINCAP"); t.k4_lds_pad = knob("GM_K4_LDS_PAD"); t.k4_wgs = knob("GM_K4_WGS"); t.k4_grid = knob("GM_K4_GRID");
  t.k5_lsw = knob("GM_K5_LSW"); t.k5_small = knob("GM_K5_SMALL"); t.k5_half = knob("GM_K5_HALF"); t.k5_half_threads = knob("GM_K5_HALF_THREADS");
  t.k5_rounds = knob("GM_K5_ROUNDS"); t.k5_candlimit = knob("GM_K5_CANDLIMIT"); t.k5_grid = knob("GM_K5_GRID"); t.k5_wlist = knob("GM_K5_WLIST");
  return t;
}
// The two decisions made outside the lookup that must agree with it: an index gets its 64-byte buckets only on one slab (gm_index.hip adds: and a mean list of at
// most 12 entries), and its strip lists when k_lookup_v5 may run on it (gm_session_create).
static inline bool k1_buckets_allowed(int n_slabs, const K1Tune& t) { return n_slabs == 1 && !t.no_buckets; }
static inline bool k5_may_run(int region_bits, const K1Tune& t) { return !t.no_v5 && region_bits >= 9 && region_bits <= 16; }
static inline bool k1_strips_wanted(int n_slabs, int region_bits, const K1Tune& t) { return (n_slabs > 1 || t.v5) && k5_may_run(region_bits, t); }
// ---- geometry of a read-strand: lists, region counters of a slab, dynamic LDS of the slab-sweep kernel ----
struct K1Geom { int max_n_kmers, NL, bm_words; size_t lds; };
static inline K1Geom k1_geometry(const K1PlanIn& in) {
  K1Geom g; g.max_n_kmers = std::max(0, in.read_len - in.min_seed_span + 1); g.NL = in.n_seeds * g.max_n_kmers;
  const uint64_t regions = (((in.n_slabs == 1) ? in.total_len : (1ull << in.slab_bits)) >> in.region_bits) + 3;      // of a slab: +1 region before, +1 partial, +1 slack
  g.bm_words = ((int)((regions + 15) / 16) + 3) & ~3;
  g.lds = (size_t)((((in.read_len + 3) / 4) + 6 * g.NL + 1 + 3) & ~3) * 4 + (size_t)g.bm_words * 4;
  return g;
}
static inline size_t k1_mp_lds(size_t lds) { return lds + (size_t)2 * K1P_MP_CAP * 4; }      // the mate-pair modes: the mate's row and this read-strand's own behind the counters

// expected list entries per read-strand
static inline double k1_expected_entries(const K1PlanIn& in) {
  double entries = 0;
  for (int sn = 0; sn < in.n_seeds; sn++) {
    const double lists = std::max(0, in.read_len - in.seed[sn].span + 1 - in.colour);
    entries += lists * (double)in.seed[sn].n_pos / (double)(1ull << (in.hflag ? 2 * K1P_HASH_TABLE_POWER : 2 * in.seed[sn].weight));
  }
  return entries;
}
// Expected candidates of k_lookup_v5 per read-strand with a seen[] table of 2^(seen_lsw + 5) bits and twice[] of 2^(lsw + 2): the reference's survivors (entries
// sharing a region; ~2x the independence estimate with the strip and the echoes of a real hit) + later arrivals on a shared seen[] bit + first arrivals that meet
// a set twice[] bit.  (The Bloom bits of the half-size shape: seen_lsw = lsw + 1, the rate of a table of twice the size.)
static inline double k5_expected_candidates(const K1PlanIn& in, double entries, int lsw, int seen_lsw) {
  const double lam = entries * (double)((1u << in.region_bits) + in.region_overlap) / std::max(1.0, (double)in.total_len);
  const double memb = 2.0 * entries * std::min(1.0, lam), late = 0.5 * entries * std::min(1.0, entries / (double)(32ull << seen_lsw));
  const double first = entries * std::min(1.0, (late + 0.5 * memb) / (double)(32ull << (lsw - 3)));
  return memb + late + first;
}
// ---- k_lookup_v5 (gm_lookup5.hip): its shape, or ok == false when it declines ----
struct K5Shape {
  bool ok;
  int lsw, ltw, hbits, cand_cap, cand_limit, xrec, threads;      // lsw, ltw: log2(words) of seen[] and twice[]
  int half; bool small_shape;                                    // half: 0, 1: k_lookup_v5_half, 2: the same without the Bloom bits (tuning builds)
  int rounds; uint32_t round_regs; int grid; size_t lds;
  bool prune; uint32_t D; int e_max;                             // K1b's rules inside the kernel, over bins of one region
};
static inline K5Shape k5_shape(const K1PlanIn& in, const K1Geom& g, const K1Tune& t, bool prune) {
  K5Shape s = K5Shape(); const int NL = g.NL, read_len = in.read_len;
  if (!in.has_strips || !k5_may_run(in.region_bits, t) || NL <= 0) return s;
  const bool forced = t.v5;
  const double entries = k1_expected_entries(in);
  if (!forced && entries < 8000.0) return s;      // the fixed cost per read-strand (144 KB of table clears, the barriers) pays off from several thousand entries
  // LDS: twice (1/8 of seen) | seen | 32 B per list | codes | control words
  // chunk records beyond one per list: 64, or what is left beside full-size tables when the lists alone nearly fill the rest (150 bp reads: 417 lists)
  const size_t budget = K1P_LDS - 512;
  const size_t fixed0 = (size_t)24 * NL + 2 * (size_t)((read_len + 15) & ~15) + K5_CTRL_WORDS * 4 + K1P_MAX_SEEDS * 32;      // (one record per list: 16 + 8 bytes, + the seed table)
  const size_t full_tables = (size_t)(4u << 15) + (size_t)(4u << 12);
  // (long reads -- two stripes in the vector filter, 450 B of LDS a wave -- keep the extra records few: what the tables leave of a CU's LDS is what pass 1 runs in beside this kernel)
  int xrec = read_len > 128 ? 16 : 64;
  if (fixed0 + 24 * (size_t)xrec + full_tables > budget && fixed0 + 24 * 16 + full_tables <= budget) xrec = (int)((budget - full_tables - fixed0) / 24);
  const size_t fixed = fixed0 + 24 * (size_t)xrec;
  int lsw = 15, threads = 1024;                                // waves per workgroup: a power of two
  // Colour space with few list entries per read-strand (50-colour reads on 3 Gbp: 17 k): the small shape -- tables of 2^19 + 2^16 bits (72 KB) and 512 threads.  The kernel
  // itself is slower that way, but it leaves half of a CU's LDS and 320 of a SIMD's 512 registers to the colour-space pass 2, which cannot run beside the full shape.
  bool small_shape = false;
  if (!forced && in.colour && NL <= 512 && !t.k5_lsw.set && !t.threads.set && !(t.k5_small.set && t.k5_small.v == 0)) {
    const double cap14 = (double)(((4u << 14) / 4u / 6u) & ~15u);
    if (k5_expected_candidates(in, entries, 14, 14) <= 0.5 * cap14 && fixed + (size_t)(4u << 14) + (size_t)(4u << 11) <= 96 * 1024) { small_shape = true; lsw = 14; threads = 512; }
  }
  // The half-size shape with rounds (k_lookup_v5_half): two 512-thread workgroups per CU, 80 KB of LDS each.  GM_K5_HALF=1 forces it, =2 takes the variant without the
  // Bloom bits (tuning builds), =0 switches it off.
  int half = t.k5_half.set ? t.k5_half.v : 0;
  const size_t half_budget = 80 * 1024 - 512, half_tables = (size_t)(4u << 14) + (size_t)(4u << 11);
  if (half && (in.region_bits < 11 || NL > 512 || fixed0 + 24 * 8 + half_tables > half_budget)) half = 0;
  if (half) { lsw = 14; threads = 512; xrec = (int)std::min<size_t>(64, (half_budget - half_tables - fixed0) / 24); }
  if (half && t.k5_half_threads.set) threads = std::max(64, std::min(1024, t.k5_half_threads.v & ~63));      // (probe: 640 = ten waves a workgroup, five a SIMD with two workgroups)
  const size_t fixed_h = fixed0 + 24 * (size_t)xrec;
  if (!half && t.k5_lsw.set) lsw = std::max(8, std::min(15, t.k5_lsw.v));
  while (!half && lsw >= 8 && fixed + (size_t)(4u << lsw) + (size_t)(4u << (lsw - 3)) > budget) lsw--;
  if (lsw < 8) return s;
  if (!half && t.threads.set) { const int v = std::max(64, std::min(1024, t.threads.v)); threads = 64; while (threads * 2 <= v) threads *= 2; }
  // twice[] = an eighth of seen[]; the region table (12 B per slot) takes three quarters of the seen[] area, the candidates (6 B each) the rest
  const int ltw = lsw - 3, hbits = lsw - 2, cand_cap = (int)(((4u << lsw) / 4u / 6u) & ~15u);
  if (cand_cap < 16) return s;
  int cand_limit = cand_cap - 8, rounds = 1;
  if (!forced) {
    // Read-strands beyond the candidate array fall back to the slab-sweep kernel: when that would be the rule (2 x 150 bp reads on 3 Gbp: ~9 k), k_lookup_v4 is the
    // better kernel -- unless more than one round (pass B and the exact stages per part of the genome) holds them, as long as the passes over the lists stay cheaper
    // than the separate kernels: up to four.
    // (The estimate is generous for long reads -- 12.8 k against 9.2 k counted for 150-base reads on 3 Gbp -- and a round costs 10 % of the kernel: two parts there, 4.6 k
    // candidates each against 5 456 slots, no read-strand of 262 144 fell back; one that does is redone exactly by the fall-back kernels.)
    const double cands = k5_expected_candidates(in, entries, lsw, lsw + (half == 1 ? 1 : 0));
    if (cands > 0.85 * cand_cap) {
      rounds = std::max((int)std::ceil(cands / ((half ? 0.95 : 1.25) * cand_cap)), 2);
      if (rounds > K5_MAX_ROUNDS || NL > threads || lsw != (half ? 14 : 15)) return s;
    }
  }
  if (t.k5_rounds.set) { rounds = std::max(1, std::min(K5_MAX_ROUNDS, t.k5_rounds.v)); if (rounds > 1 && (NL > threads || lsw != (half ? 14 : 15))) return s; }
  // the genome's regions dealt evenly to the rounds (positions are 32 bits; the last round takes what is left)
  const uint32_t n_regs = (uint32_t)((in.total_len + (1ull << in.region_bits) - 1) >> in.region_bits);
  if (t.k5_candlimit.set) cand_limit = std::max(1, std::min(cand_limit, t.k5_candlimit.v));
  s.prune = prune; s.D = (uint32_t)std::max(in.want_fuse ? in.window_len : 0, read_len); s.e_max = prune ? std::min(in.e_max, read_len) : -1;
  if (prune && (s.D + (uint32_t)std::max(0, s.e_max) > (1u << in.region_bits) || s.D > 0xFFFFu)) return s;   // the prune rules need bins (= regions) of at least D + e_max positions
  s.lsw = lsw; s.ltw = ltw; s.hbits = hbits; s.cand_cap = cand_cap; s.cand_limit = cand_limit; s.xrec = xrec; s.threads = threads; s.half = half; s.small_shape = small_shape;
  s.rounds = rounds; s.round_regs = std::max(1u, (n_regs + (uint32_t)rounds - 1u) / (uint32_t)rounds);
  s.lds = (half ? fixed_h : fixed) + (size_t)(4u << lsw) + (size_t)(4u << ltw);
  // (the half-size shapes: two workgroups a CU -- the lookup takes 7.1 instead of 11.5 ms per launch, 190 -> 179 ms per 1 M 50-colour reads, tools/k5_shape_cfg4.sh)
  s.grid = std::min(2 * in.n_reads, (half || small_shape) ? 2 * in.cus : in.cus);
  if (t.k5_grid.set) s.grid = std::max(1, std::min(2 * in.n_reads, t.k5_grid.v));
  s.ok = true; return s;
}
// ---- k_lookup_v4: its shape, or ok == false when it declines ----
struct K4Shape { bool ok; int tab_bits, cbits, SC, wcap, bin_cap, threads, grid; size_t lds; };
static inline K4Shape k4_shape(const K1PlanIn& in, const K1Geom& g, const K1Tune& t) {
  K4Shape s = K4Shape();
  // v4's fixed cost per read-strand (two 128 KB table clears, per-bin passes) pays off from ~30 k list entries per read-strand
  // (measured: 45 k at 100 bp / 3 Gbp 7 % faster than the slab sweep, 17 k at 50 colours 40 % slower)
  if (k1_expected_entries(in) < 30000.0 && !t.v4) return s;
  s.tab_bits = t.k4_tabbits.set ? std::max(6, std::min(19, t.k4_tabbits.v)) : 19;
  // pass C keeps the exact counters of one bin of 2^cbits positions (+2) in the table's LDS; bins nest inside the index slabs
  s.cbits = std::min(in.slab_bits, s.tab_bits + in.region_bits - 1);
  if (s.cbits < in.region_bits + 1) return s;
  s.SC = (int)((in.total_len + (1ull << s.cbits) - 1) >> s.cbits);
  if (s.SC < 1 || s.SC > 4096) return s;
  s.wcap = t.k4_wcap.set ? std::max(2, std::min(4096, t.k4_wcap.v & ~1)) : 4096;   // windows with a direct window -> list entry (the rest: binary search)
  s.bin_cap = 4096; if (t.k4_bincap.set) { const int v = std::max(16, std::min(1 << 20, t.k4_bincap.v)); s.bin_cap = 16; while (s.bin_cap < v) s.bin_cap <<= 1; }
  const int code_words = (in.read_len + 3) / 4;
  s.lds = (size_t)(((((code_words + 3) & ~3) + 4 * g.NL + g.NL + 1 + s.SC + (s.wcap + 1) / 2 + 3) & ~3) + (1 << (s.tab_bits - 4)) + 4) * 4;
  if (t.k4_lds_pad.set) s.lds += (size_t)std::max(0, t.k4_lds_pad.v);   // experiment: what the LDS footprint does to the co-residency with pass 1 / pass 2
  if (s.lds > K1P_LDS - 64) return s;
  const int wgs_per_cu = t.k4_wgs.set ? std::max(1, std::min(8, t.k4_wgs.v)) : 1;
  s.grid = std::min(2 * in.n_reads, in.cus * wgs_per_cu);
  if (t.k4_grid.set) s.grid = std::max(1, std::min(2 * in.n_reads, t.k4_grid.v));
  s.threads = t.threads.set ? std::max(64, std::min(1024, t.threads.v & ~63)) : 1024;
  s.ok = true; return s;
}
// k_lookup_v3: its dynamic LDS (long reads on many slabs: the per-slab window maps outgrow the LDS and the slab-sweep kernel takes over)
static inline size_t k3_lds(const K1PlanIn& in, const K1Geom& g) {
  return (size_t)((((in.read_len + 3) / 4) + 3 * g.NL + in.n_slabs * g.NL + (in.n_slabs + 1) / 2 + (g.NL * (in.n_slabs + 1) + 1) / 2 + 3) & ~3) * 4 + (size_t)g.bm_words * 4;
}
// The bucket kernels: the persistent form (k_lookup_bkt_p probes one read-strand ahead) unless GM_BKT_V1 asks for one workgroup per read-strand (k_lookup_bkt) or
// the persistent form does not fit.  The persistent grid is what fits a CU (the occupancy query at launch, at most bkt_per_cu) times the CUs.
struct K1BktForm { bool persistent; int threads; size_t lds, lds_p; };
static inline K1BktForm k1_bkt_form(const K1PlanIn& in, const K1Geom& g, const K1Tune& t) {
  K1BktForm b; const size_t codes = (size_t)((((in.read_len + 3) / 4) + 3) & ~3) * 4;
  b.lds = codes + (size_t)g.bm_words * 4; b.lds_p = b.lds + codes; b.threads = (g.NL + 63) & ~63;
  b.persistent = !(t.bkt_v1 || b.threads > 512 || b.lds_p > 64 * 1024);
  return b;
}
// ---- the plan: the variants to try, in order.  One after the first runs only when the one before it could not allocate its scratch. ----
enum K1Variant { K1_SWEEP = 0, K1_BKT, K1_V3, K1_V4, K1_V5 };
struct K1Plan {
  K1Geom g; int n; K1Variant order[3];
  int sweep_mp, sweep_threads; size_t sweep_lds;      // K1_SWEEP: the kernel's MP mode
  K5Shape v5; K4Shape v4; K1BktForm bkt; size_t lds3; int threads3;
};
static inline K1Plan k1_plan(const K1PlanIn& in, const K1Tune& t) {
  K1Plan p = K1Plan(); p.g = k1_geometry(in); p.sweep_lds = p.g.lds;
  const int NL = p.g.NL;
  if (in.mp_mode) {   // paired -n 3: the slab-sweep kernel in one of its mate-pair modes (GmMpDev); any mode other than 1, 3, 4, 5 runs as 2
    p.sweep_mp = (in.mp_mode == 1 || in.mp_mode == 3 || in.mp_mode == 4 || in.mp_mode == 5) ? in.mp_mode : 2;
    p.sweep_threads = std::min(1024, std::max(256, (NL + 63) & ~63)); p.sweep_lds = k1_mp_lds(p.g.lds);
    p.order[p.n++] = K1_SWEEP; return p;
  }
  const bool all = in.no_region_counts != 0;      // every list entry survives: the slab-sweep kernel carries that switch (MP 6), the filtering kernels do not apply
  const bool bkt = !all && in.has_buckets && k1_buckets_allowed(in.n_slabs, t) && NL <= 512;
  // k_lookup_v5: wave-per-list streaming, candidates and the exact rule in LDS, K1b's prune rules fused when the caller allows.  It takes the read-strands with many
  // list entries (k5_shape declines the others: small genomes, too many candidates) -- 2.09 M reads/s against 1.90 M with v4 + K1b on the 3 Gbp workload.
  if (!all && !bkt && NL < 65536 && !t.v2 && !t.v3 && !t.v4) {      // (GM_NO_V5: k5_may_run inside k5_shape)
    p.v5 = k5_shape(in, p.g, t, in.want_fuse);
    if (!p.v5.ok && in.want_fuse) p.v5 = k5_shape(in, p.g, t, false);   // the prune rules do not fit region-sized bins (very long reads): v5 without them, K1b afterwards
    if (p.v5.ok) p.order[p.n++] = K1_V5;
  }
  if (bkt) { p.bkt = k1_bkt_form(in, p.g, t); p.order[p.n++] = K1_BKT; return p; }
  if (!all && in.n_slabs > 1 && NL < 65536 && !t.v2 && !t.v3) {      // k_lookup_v4: hashed pre-count + exact count on the candidates
    p.v4 = k4_shape(in, p.g, t);
    if (p.v4.ok) p.order[p.n++] = K1_V4;
  }
  p.lds3 = k3_lds(in, p.g);
  if (!all && in.list_cutoff < 65536u && !t.v2 && p.lds3 <= K1P_LDS) {
    p.threads3 = t.threads.set ? std::max(64, std::min(768, t.threads.v & ~63)) : 768;
    p.order[p.n++] = K1_V3; return p;
  }
  p.sweep_mp = all ? 6 : 0;
  // one list per lane when the read-strand's lists fit a workgroup: every list slice is in flight at once
  p.sweep_threads = t.threads.set ? std::max(64, std::min(1024, t.threads.v & ~63)) : std::min(1024, (NL + 63) & ~63);
  p.order[p.n++] = K1_SWEEP; return p;
}
// The heavy tier's re-run (gm_launch_lookup_redo), always the slab-sweep kernel: MP 6 without region counts, else the mate-pair mode when that is 2, 4 or 5 (1 and 3 run MP 0)
static inline int k1_redo_mp(int no_region_counts, int mp_mode) { return no_region_counts ? 6 : (mp_mode == 5 || mp_mode == 4 || mp_mode == 2) ? mp_mode : 0; }
// the name gm_last_lookup_kernel reports for a variant of the plan
static inline const char* k1_variant_name(const K1Plan& p, K1Variant v) {
  if (v == K1_V5) return p.v5.half ? "k_lookup_v5_half" : p.v5.rounds > 1 ? "k_lookup_v5_rounds" : "k_lookup_v5";
  return v == K1_V4 ? "k_lookup_v4" : v == K1_V3 ? "k_lookup_v3" : v == K1_BKT ? "k_lookup_bkt" : "k_lookup";
}
