// gm_lookup5_kernel.inc -- the body of k_lookup_v5, compiled twice by gm_lookup5.hip (which documents it): as the kernel template k_lookup_v5<LSWC> (one round) and as
// k_lookup_v5_rounds (MULTI: pass B and the exact stages once per part of the genome, with its own register target).  Two kernels from one text rather than a shared
// __device__ function: through a function the index and the arguments arrive by reference, the loads from the kernel-argument segment lose their "constant" property, and the
// allocator needs 20 registers more.  The includer defines K5_KERNEL_HEAD (the kernel's declarator), K5_KERNEL_MULTI and, where LSWC is not a template parameter, K5_KERNEL_LSWC.
K5_KERNEL_HEAD {
  constexpr bool MULTI = K5_KERNEL_MULTI;
#ifdef K5_KERNEL_BLOOM
  constexpr bool BLOOM = K5_KERNEL_BLOOM;
#else
  constexpr bool BLOOM = false;
#endif
#ifdef K5_KERNEL_LSWC
  constexpr int LSWC = K5_KERNEL_LSWC;
#endif
  if (a.start_flags && threadIdx.x == 0) __hip_atomic_store(&a.start_flags[blockIdx.x], a.start_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __builtin_amdgcn_s_setprio(3);
  extern __shared__ __align__(16) uint32_t smem[];
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & (GM_WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nwv = nthr >> 6;
  const int S = ix.n_slabs, rb = ix.region_bits, lsw = LSWC ? LSWC : a.lsw, ltw = lsw - 3, hbits = lsw - 2;
  const int cand_cap = LSWC ? (int)(((4u << LSWC) / 4u / 6u) & ~15u) : a.cand_cap;
  const uint32_t rmask = (1u << rb) - 1u, ovl = (uint32_t)ix.region_overlap;
  const uint32_t wmask = (1u << lsw) - 1u, tmask = (1u << ltw) - 1u;
  // LDS: twice | seen (later: candidates | region table) | rec[NL] (4 words) | srec[NL] (2 words) | codes | ctrl
  // Byte offsets into the tables come straight from the position: twice word of p at (p >> (rb - 2)) & tmask4 (twice[] starts at 0: no base to add), its
  // seen word at swb + ((p >> (rb - 2)) & smask4) (swb = the size of twice[]: an instruction offset when the sizes are compile-time), bit (p >> (rb + lsw)) & 31.
  if ((uint32_t)(uintptr_t)(k5_lds_u32*)smem != 0u) __builtin_trap();      // no static LDS in this kernel: the dynamic segment starts at 0
  uint32_t* twice = smem;
  uint32_t* seen = smem + (1u << ltw);
  // after pass A the seen[] area is re-used: candidate positions (cand_cap words) | candidate y / seed (u16) -- cand_cap = the first quarter / 6 bytes; with the
  // production sizes both arrays lie below 64 KB, so that pass B's stores carry their base in the LDS instruction's offset field -- then htag | hmin | hmax
  // (2^hbits = 2^(lsw - 2) words each: the other three quarters)
  uint32_t* candp = seen;
  uint16_t* candy = (uint16_t*)(candp + cand_cap);
  uint32_t* htag = seen + (1u << hbits);
  uint32_t* hmin = htag + (1u << hbits);
  uint32_t* hmax = hmin + (1u << hbits);
  uint32_t* rec = seen + (1u << lsw);
  const int RC = a.NL + a.xrec;                                  // records: one per chunk of at most 256 positions (a longer list takes several)
  uint32_t* srec = rec + 4 * RC;                                // strip list of a record's list: offset inside its seed's strip array, length (the seed is in the record's y word)
  // The lists of exact stage 1 live in rec[] / srec[] (6 * RC words, dead since pass B), a segment per wave: wseg words, of which the wave uses wcap (see stage 1)
  const uint32_t wseg = 6u * (uint32_t)RC / (uint32_t)nwv;
  uint32_t* const wlist = rec + (uint32_t)wv * wseg;
#ifdef GM_TUNING
  const uint32_t wcap = min(wseg, (uint32_t)__builtin_amdgcn_readfirstlane(a.wlist));      // (GM_K5_WLIST: a shorter list, down to none)
  // (a wave's items, listed and taken on the spot, go to two control words; thread 0 hands them on with the read-strand's other counts: gm_debug_k5_wave_lists)
#define K5_WL_COUNT(listed, spot) do { if (lane == 0) { atomicAdd(&ctrl[C_WLISTED], (listed)); atomicAdd(&ctrl[C_WSPOT], (spot)); } } while (0)
#else
  const uint32_t wcap = wseg;
#define K5_WL_COUNT(listed, spot) do { } while (0)
#endif
  uint8_t* codes = (uint8_t*)(srec + 2 * RC);
  uint32_t* ctrl = (uint32_t*)(codes + 2 * ((a.read_len + 15) & ~15));           // two code buffers (this read-strand's and the next one's)
  const uint32_t smask4 = wmask << 2, tmask4 = tmask << 2, swb = 4u << ltw;
  const int sh_a = rb - 2, sh_b = rb + lsw;
  const uint32_t hmask = (1u << hbits) - 1u; const int hshift = 32 - hbits;
  // Where pass B puts its candidates (absolute LDS byte addresses; instruction offsets when the sizes are compile-time).  One round: the arrays of the exact stages.  MULTI: the
  // candidates of ALL parts go to the region table's area, which is idle during pass B -- 2 << hbits of them, 6 bytes each -- and are dealt to the parts afterwards (part 0 to the
  // arrays of the exact stages, the others to the workgroup's rows in global memory).  No global store sits in the streaming loop that way: on gfx9 stores count in vmcnt like
  // loads, and a store behind every step's hits made each counted wait for the oldest chunk wait for the younger chunks too (round 4: pass B 107 k -> see DESIGN).
  const uint32_t pb_cap = MULTI ? (2u << hbits) : (uint32_t)cand_cap;
  const uint32_t pb_pos = MULTI ? swb + (4u << hbits) : swb, pb_y = pb_pos + 4u * pb_cap;
  uint32_t* const sb_pos = MULTI ? htag : candp; uint16_t* const sb_y = (uint16_t*)(sb_pos + pb_cap);      // (the same arrays as pointers, for the strip loop)
  const int hclr_q = (int)(3u << hbits) >> 2;                         // uint4 words of the region table (cleared during pass B)
  const int tab_q = (int)(((1u << ltw) + (1u << lsw)) >> 2);             // uint4 words of twice + seen
  const uint32_t* __restrict__ pos0 = ix.seed[0].pos;
  const uint32_t* __restrict__ spos0 = ix.seed[0].spos;
  unsigned long long my_lookups = 0, my_entries = 0;
  // the prune rules' arguments as opaque scalars, fixed here in uniform control flow (see stage 2a)
  uint32_t k_prune = __builtin_amdgcn_readfirstlane(a.prune != 0 ? 1u : 0u), k_D = __builtin_amdgcn_readfirstlane(a.D);
  uint32_t k_emax_on = __builtin_amdgcn_readfirstlane(a.e_max >= 0 ? 1u : 0u), k_emax = __builtin_amdgcn_readfirstlane((uint32_t)max(a.e_max, 0));
  asm volatile("" : "+s"(k_prune), "+s"(k_D), "+s"(k_emax_on), "+s"(k_emax));

  { uint4* t4 = (uint4*)smem; for (int w = tid; w < tab_q; w += nthr) t4[w] = make_uint4(0, 0, 0, 0); }
  if (tid < C_WORDS) ctrl[tid] = 0;                            // thread 0 re-zeroes them at the end of every read-strand

  // BLOOM (the half-size shape): a region sets TWO bits of its seen[] word -- bit t & 31 and bit t + 1 + 4 * ((t >> 5) & 3), t = region >> lsw -- and counts as seen when both are
  // there.  The regions that share a word differ in t, and the (unordered) bit pairs of different t below 128 are all different (distances 1, 5, 9, 13 and their complements
  // 31, 27, 23, 19): no two regions alias exactly, a false "seen" needs two other regions' bits -- at 2^19 bits the rate of a single bit per region at 2^20.
  auto bloom_mask = [&](const uint32_t t) -> uint32_t { return (1u << (t & 31u)) | (2u << ((t + (((t >> 5) & 3u) << 2)) & 31u)); };
  auto mark = [&](const uint32_t p) {                          // one mark of region p >> rb (strip loop; the main loop has its own batched form)
    const uint32_t av = p >> sh_a, t = p >> sh_b, m1 = 1u << (t & 31u), m = BLOOM ? bloom_mask(t) : m1;
    const uint32_t old = K5_LDS_OR(swb + (av & smask4), m);
    if ((old & m) == m) K5_LDS_OR(av & tmask4, m1);
  };
  auto has2 = [&](const uint32_t p) -> bool { return (*K5_LDS((p >> sh_a) & tmask4) >> ((p >> sh_b) & 31u)) & 1u; };
  // The twice[] bit of region r as a FILTER for the neighbour-region look-ups of the exact stages (stage 2b, the prune_only tail): twice[] is written by pass A only and
  // cleared at the very end of a read-strand, behind both, so it still holds pass A's answer there.  What a clear bit of region x proves:
  //  (M) pass A marked x at most once.  A mark of x is a list entry inside x (main loop) or a strip entry inside x + 1 (strip loop).  The second mark of a region always finds
  //      what the first one left in seen[] -- its one bit, or with BLOOM both of its bits; LDS atomics on one word are serialised, also within one instruction -- and sets the
  //      region's twice[] bit.  Aliasing regions, the words a lane marks past its chunk and Bloom collisions only ever set more bits.
  //  (B) x does not carry flag B in the region table of any round.  The table counts one mark of x per candidate inside x (first-slot CAS, probe_on) and one per candidate in the
  //      strip of x + 1 (the mark-only k5_insert(r - 1, false), listed or inside probe_on).  Candidates are distinct list entries -- a strip entry is a candidate of the strip
  //      loop only when its own region fails the main loop's test -- and pass A marked x for each of them on the same grounds, so the table's count is at most pass A's: <= 1.
  //      A round of k_lookup_v5_rounds sees a subset of the candidates (its part and the halo), which lowers the count only.
  //  (C) x holds no candidate of pass B's main loop (they pass has2 of their own region).  It may hold candidates of the strip loop -- entries in the strip of x whose region
  //      BEFORE, x - 1, has its bit set; they sit in x's own slot with flags C / D / E and min / max.  So only with the bits of x AND x - 1 both clear is x free of flag C; a
  //      slot of x may still exist then (mark-only, or a halo region), with flag A alone.
  // Hence: a look-up that reads flag B only may answer "absent, tag 0" on a clear bit of x (2b's membership through the region before, the tail); one that reads flag C and
  // min / max needs x and x - 1 clear (2b's prune look-up of the region BEFORE the candidate's).  The prune look-up of the region BEHIND, r + 1, gets no filter: its second bit
  // is the candidate's own region r, which is set for every member that did not come in through the region before, and strip candidates in r + 1 are exactly what that look-up
  // is for.  Region 0 has no strip candidates (the strip lists leave region 0 out); has2r(0 - 1) reads some other word of the table and can only let a look-up through.
  // Every case where the flags could be there goes through the full probe sequence as before, so the tag words read, and with them the survivors, are the same bit for bit.
  auto has2r = [&](const uint32_t r) -> bool {
#ifdef K5_NO_TWICE_FILTER     // (diagnostic builds: the look-ups as before the filter)
    return true;
#else
    return (*K5_LDS((r << 2) & tmask4) >> ((r >> lsw) & 31u)) & 1u;
#endif
  };

#ifdef K5_STAMPS
  unsigned long long t_prev = __builtin_amdgcn_s_memtime();
#endif
  // Set-up of a read-strand (k-mers -> map indexes -> directory entries) one read-strand ahead: while the passes of read-strand n run, the
  // directory words of read-strand n + 1 are already on their way (two dependent HBM round trips and a 19-step loop per k-mer off the critical
  // path).  One k-mer per thread (NL <= threads); longer reads take the plain path.
  const bool ahead = a.NL <= nthr;
  const uint32_t cpad = (uint32_t)((a.read_len + 15) & ~15);     // (code buffer b = codes + b * cpad: pointer arithmetic keeps the LDS address space, a pointer array does not)
  uint32_t pf_b = 0, pf_e = 0, pf_sb = 0, pf_se = 0; bool pf_ok = false;
  auto fill_codes = [&](const int r, uint8_t* cb) {
    if (r >= 2 * a.n_reads) return;
    const uint32_t* rw = a.reads + (size_t)(r >> 1) * a.read_words;
    for (int i = tid; i < a.read_len; i += nthr) cb[i] = (uint8_t)gm_read_code(rw, a.read_len, (r & 1) ^ ix.cs_flip, ix.colour, i, GM_READ_RNA(ix, r >> 1));
  };
  // A thread keeps the same k-mer slot (seed, offset in the read) for every read-strand: its seed's span and mask stay in registers, the seed's
  // pointers in a small LDS table.  (ix.seed[sn] with a run-time sn is a chain of loads from the kernel-argument segment -- a memory round trip
  // per field and use: 4 k cycles per read-strand before.)
  uint32_t* stab = ctrl + C_WORDS;                             // per seed: dir, sdir (pointers), pos - pos0, spos - spos0 (elements)
  if (tid < ix.n_seeds) {
    const GmSeedDev& sd = ix.seed[tid];
    const uint64_t d = (uint64_t)(uintptr_t)sd.dir, sdp = (uint64_t)(uintptr_t)sd.sdir, po = (uint64_t)(sd.pos - pos0), so = (uint64_t)(sd.spos - spos0);
    *(uint4*)&stab[8 * tid] = make_uint4((uint32_t)d, (uint32_t)(d >> 32), (uint32_t)sdp, (uint32_t)(sdp >> 32));
    *(uint4*)&stab[8 * tid + 4] = make_uint4((uint32_t)po, (uint32_t)(po >> 32), (uint32_t)so, (uint32_t)(so >> 32));
  }
  int k_sn = 0, k_i = 0, k_span = 0; uint64_t k_mask = 0; bool k_ok = false;
  // The k-mer slots sit on the first threads: ceil(NL / 64) waves ("set-up waves", 4 of 16 at 100 bp) work out the map indexes of the next read-strand, the
  // other waves skip that arithmetic (their directory loads are dummies) and go straight to pass A, where they take one list each ahead of the rota
  // (see the step generator) -- the set-up costs a quarter of the vector instructions it took when every stride-th thread of all the waves held a slot.
  const int k_stride = 1, k_slot = tid;
  const int nsw = ahead ? min(nwv, (a.NL + GM_WAVE - 1) / GM_WAVE) : nwv;      // set-up waves
  if (ahead && k_slot < a.NL) {
    k_sn = k_slot / a.max_n_kmers; k_i = k_slot - k_sn * a.max_n_kmers;
    k_span = ix.seed[k_sn].span; k_mask = ix.seed[k_sn].mask;
    k_ok = k_i >= ix.colour && k_i + k_span <= a.read_len;
    if (!k_ok) { k_span = 0; k_mask = 0; }
  }
  // One record per chunk of at most 256 positions (the list's address + the chunk's, its length, y / seed), so that the step generator of the two passes is
  // "next record": a list longer than 256 takes several; its strip list rides on the first one.  Records beyond the array are dropped, the read-strand then
  // falls back (rec_over below).  `cnl` is this read-strand's counter word.
  uint32_t* cnl_w = nullptr;
  // the strip list of record j0: (pointer, length) -- the offset inside the seed's strip array from srec[], the array's own offset from the seed table
  auto strip_of = [&](const int j0, uint32_t& slen) -> const uint32_t* {
    const uint2 sr = *(const uint2*)&srec[2 * j0];
    const uint4 st = *(const uint4*)&stab[8 * (rec[4 * j0 + 3] & 15u) + 4];
    slen = sr.y;
    return spos0 + ((((uint64_t)st.w << 32) | st.z) + sr.x);
  };
  auto put_records = [&](const uint64_t la, const uint32_t len, const uint32_t ysn, const uint32_t sb, const uint32_t slen) {
    const uint32_t nch = (len + 255u) >> 8;
    const uint32_t j = atomicAdd(cnl_w, nch);
    for (uint32_t c = 0; c < nch && j + c < (uint32_t)RC; c++) {
      const uint64_t ca = la + ((uint64_t)c << 10);
      *(uint4*)&rec[4 * (j + c)] = make_uint4((uint32_t)ca, (uint32_t)(ca >> 32), min(256u, len - (c << 8)), ((ysn >> 12) & 0xFFF0u) | (ysn & 0xFu));   // y << 4 | seed: as the candidates carry it
      *(uint2*)&srec[2 * (j + c)] = c ? make_uint2(0u, 0u) : make_uint2(sb, slen);
    }
  };
  auto put_list = [&](const uint32_t b, const uint32_t n, const uint32_t sb, const uint32_t sn) {      // this thread's list (set-up ahead: the thread's k-mer slot is fixed)
    const uint4 so = *(const uint4*)&stab[8 * k_sn + 4];
    const uint64_t ptr = (((uint64_t)so.y << 32) | so.x) + b;
    put_records((uint64_t)(uintptr_t)(pos0 + ptr), n, ((uint32_t)k_i << 16) | (uint32_t)k_sn, sb, sn);
  };
  auto kmer_ahead = [&](const int r, const uint8_t* cb) {      // the four directory words of this thread's k-mer of read-strand r: loads issued, used at the next top
    pf_ok = k_ok && r < 2 * a.n_reads;
    uint32_t mapidx = 0;
    if (wv >= nsw) {}                                        // (no slot in this wave: wave-uniform)
    else if (!ix.hflag) {
      // KMER_TO_MAPIDX (ref: gmapper.h:349-368) without a branch per base: eight code bytes per LDS round trip, the mask bit selects
      for (int t0 = 0; t0 < ix.max_seed_span; t0 += 8) {
        uint32_t c[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const int x = k_i + k_span - 1 - t0 - u; c[u] = cb[min(max(x, 0), a.read_len - 1)]; }
#pragma unroll
        for (int u = 0; u < 8; u++) mapidx = ((k_mask >> (t0 + u)) & 1ull) ? ((mapidx << 2) | (c[u] & 3u)) : mapidx;
      }
    } else if (pf_ok) mapidx = gm_mapidx(ix, k_mask, k_span, cb + k_i);
    if (!pf_ok) mapidx = 0;
    // (unconditional loads and, at the next top, an unconditional use: conditional ones leave the compiler's counter model with "maybe pending" loads
    // and it then waits for vmcnt(0) inside the streaming loops)
    const uint4 sp = *(const uint4*)&stab[8 * k_sn];
    // (pointers rebuilt from integers must name the global address space: a flat load also counts as an LDS operation, and every LDS wait
    // behind it would wait for the memory round trip)
    typedef const uint32_t __attribute__((address_space(1)))* k5_gptr;
    const k5_gptr dir = (k5_gptr)(((uint64_t)sp.y << 32) | sp.x) + (size_t)mapidx * (uint32_t)S;
    const k5_gptr sdir = (k5_gptr)(((uint64_t)sp.w << 32) | sp.z) + mapidx;
    pf_b = dir[0]; pf_e = dir[S]; pf_sb = sdir[0]; pf_se = sdir[1];
  };
  // MULTI: the position ranges of the rounds with their halo (one region either side), and this workgroup's rows for the candidates set aside
  uint32_t rf_lo[K5_MAX_ROUNDS], rf_m1[K5_MAX_ROUNDS];
#pragma unroll
  for (int d = 0; d < K5_MAX_ROUNDS; d++) {
    const uint64_t rsz64 = 1ull << rb, lo = (uint64_t)d * a.round_regs * rsz64, hi = d >= a.rounds - 1 ? (1ull << 32) : lo + (uint64_t)a.round_regs * rsz64;
    const uint64_t flo = lo >= rsz64 ? lo - rsz64 : 0ull, fhi = hi + rsz64 < (1ull << 32) ? hi + rsz64 : (1ull << 32);
    rf_lo[d] = (uint32_t)std::min<uint64_t>(flo, 0xFFFFFFFFull); rf_m1[d] = MULTI && d < a.rounds && flo < (1ull << 32) ? (uint32_t)(fhi - 1ull - flo) : 0u;
  }
  uint2* const spill_wg = MULTI ? a.spill + (size_t)blockIdx.x * (size_t)(a.rounds - 1) * a.spill_cap : nullptr;
  __syncthreads();
  if (ahead) { fill_codes(blockIdx.x, codes); __syncthreads(); kmer_ahead(blockIdx.x, codes); }
  int it = 0;
  for (int rs = blockIdx.x; rs < 2 * a.n_reads; rs += gridDim.x, it++) {
    // (the list counter alternates between two words: with the set-up ahead there is no barrier between thread 0's reset at the end of a
    // read-strand and the first additions of the next one; the other word was reset a whole read-strand earlier)
    uint32_t* const cnl = &ctrl[C_NLISTS + (it & 1)];
    cnl_w = cnl;
    if (ahead) {
      fill_codes(rs + (int)gridDim.x, codes + (uint32_t)((it + 1) & 1) * cpad);
      const uint32_t b = pf_b, e = pf_e, sb = pf_sb, se = pf_se;
      if ((b ^ e ^ sb ^ se) == 0x9E3779B9u && e - b == 0x7F4A7C15u) ctrl[C_SINK] = 1u;        // never true for list bounds: pins the use of all four words here
      const bool has_list = pf_ok && e != b && e - b <= ix.list_cutoff;      // ref: mapping.c:497 (longer lists are skipped, not deleted)
      if (pf_ok) my_lookups++;
      if (has_list) { my_entries += (e - b); put_list(b, e - b, sb, se - sb); }
      __syncthreads();                                         // rec[] of this read-strand and the codes of the next one are in; the tables are clear
      K5_STAMP(8);
      kmer_ahead(rs + (int)gridDim.x, codes + (uint32_t)((it + 1) & 1) * cpad);
      K5_STAMP(9);
    } else {
    const int rd = rs >> 1, st = rs & 1;
    const uint32_t* rw = a.reads + (size_t)rd * a.read_words;
    for (int i = tid; i < a.read_len; i += nthr) codes[i] = (uint8_t)gm_read_code(rw, a.read_len, st ^ ix.cs_flip, ix.colour, i, GM_READ_RNA(ix, rd));
    __syncthreads();                                           // also: the tables and the control words are clear
    // ---- map indexes, list bounds, strip-list bounds (ref: mapping.c:53-66, KMER_TO_MAPIDX gmapper.h:349-368) ----
    for (int off = tid; off < a.NL; off += nthr) {
      const int sn = off / a.max_n_kmers, i = off - sn * a.max_n_kmers;
      const int span = ix.seed[sn].span;
      if (i < ix.colour || i + span > a.read_len) continue;
      const uint32_t mapidx = gm_mapidx(ix, ix.seed[sn].mask, span, codes + i);
      const uint32_t* dir = ix.seed[sn].dir + (size_t)mapidx * (uint32_t)S;
      my_lookups++;
      const uint32_t b = dir[0], e = dir[S];
      if (e == b || e - b > ix.list_cutoff) continue;          // ref: mapping.c:497 (longer lists are skipped, not deleted)
      const uint32_t sb = ix.seed[sn].sdir[mapidx], se = ix.seed[sn].sdir[mapidx + 1];
      my_entries += (e - b);
      put_records((uint64_t)(uintptr_t)(ix.seed[sn].pos + b), e - b, ((uint32_t)i << 16) | (uint32_t)sn, sb, se - sb);
    }
    __syncthreads();
    }
    // (no barrier behind the k-mers ahead: they read the next read-strand's codes and the seed table only, and their scattered loads -- 64 cache
    // lines per instruction -- queue up in the address unit; the waves go on to pass A as they get through)
    K5_STAMP(0);
    const int nl_raw = (int)*cnl, nl = min(nl_raw, RC);
    const bool rec_over = nl_raw > RC;                          // more chunks than records: the read-strand is redone by the fall-back kernels

    // One chunk of a list: n <= 256 entries from src, W = ceil(n / 64) per lane.  Wave-uniform (SGPRs).
    struct Step { uint32_t n, ysn; const uint32_t* src; };
    // generator: the next record of this wave.  The waves without k-mer slots reach pass A earlier than the set-up waves: each of them takes one record of
    // the first `xh` ahead of the rota (record wv - nsw), then every wave strides through the rest (xh + wv, xh + wv + nwv, ...).
    const int xh = min(nl, nwv - nsw);
    int gj = wv, gnext = wv;
    uint4 gr = make_uint4(0, 0, 0, 0);                         // that record, read one step ahead of its use (an LDS round trip off the critical path)
    auto gen_reset = [&]() { gnext = xh + wv; gj = (wv >= nsw && wv - nsw < xh) ? wv - nsw : gnext; if (gj == gnext) gnext += nwv; if (gj < nl) gr = *(const uint4*)&rec[4 * gj]; };
    auto gen = [&](Step& s) {
      s.n = 0; s.ysn = 0; s.src = pos0;
      if (gj < nl) {
        const uint64_t o = ((uint64_t)__builtin_amdgcn_readfirstlane(gr.y) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane(gr.x);
        s.n = __builtin_amdgcn_readfirstlane(gr.z); s.ysn = __builtin_amdgcn_readfirstlane(gr.w);
        s.src = (const uint32_t*)(const uint32_t __attribute__((address_space(1)))*)(uintptr_t)o;   // (rebuilt from integers: it has to name the global address space, else the loads become flat loads)
        gj = gnext; gnext += nwv; if (gj < nl) gr = *(const uint4*)&rec[4 * gj];
      }
    };
#undef K5_GEN_B
#undef K5_GEN_RESET_B
#ifdef K5_REV_B
    // Diagnostic builds only (-DK5_REV_B, tools/k5_rev_probe.sh): pass B takes the wave's records in the OPPOSITE order -- what a wave streamed last in pass A is asked for first,
    // in case those lines still sat in the XCD's L2.  Measured in round 4 and NOT adopted: 68.1 against 67.7 ms per 262 144 reads, L2 hits 18.0 -> 19.4 %, fabric reads -2.5 %
    // (profiles/r04c, r04d): the L2 keeps next to nothing of a pass across the ~20 us between the two reads of a list, in either order.
    // The record sequence of a wave is [its record ahead of the rota,] xh + wv, xh + wv + nwv, ...: backwards that is the rota downwards, then the record ahead.
    const int g_first = xh + wv, g_ahead = (wv >= nsw && wv - nsw < xh) ? wv - nsw : -1;
    auto gen_reset_rev = [&]() {
      gj = g_first < nl ? g_first + ((nl - 1 - g_first) / nwv) * nwv : g_ahead;
      if (gj >= 0) gr = *(const uint4*)&rec[4 * gj];
    };
    auto gen_rev = [&](Step& s) {
      s.n = 0; s.ysn = 0; s.src = pos0;
      if (gj >= 0) {
        const uint64_t o = ((uint64_t)__builtin_amdgcn_readfirstlane(gr.y) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane(gr.x);
        s.n = __builtin_amdgcn_readfirstlane(gr.z); s.ysn = __builtin_amdgcn_readfirstlane(gr.w);
        s.src = (const uint32_t*)(const uint32_t __attribute__((address_space(1)))*)(uintptr_t)o;
        gj = gj >= g_first ? (gj - nwv >= g_first ? gj - nwv : g_ahead) : -1;
        if (gj >= 0) gr = *(const uint4*)&rec[4 * gj];
      }
    };
#define K5_GEN_B gen_rev
#define K5_GEN_RESET_B gen_reset_rev
#else
#define K5_GEN_B gen
#define K5_GEN_RESET_B gen_reset
#endif
    // EVERY step issues exactly one dwordx4 per lane -- lanes past the chunk re-read its last entry, an exhausted generator reads the first
    // words of pos[] -- so that the loads form one straight pipeline of depth K5_Q.  The last lane may read up to 3 words past the chunk
    // (next list / tail pad).  (Hand-issued inline-asm loads with a manual s_waitcnt vmcnt(K5_Q - 1) returned stale registers now and then on
    // gfx950 -- tools/probes/vmcnt_order.hip -- so the loads are left to the compiler, which places the counted waits itself.)
    auto issue = [&](const Step& s, k5_u32x4& v) {
      const uint32_t W = (s.n + 63u) >> 6, x = k5_lane_times(lane, W), lim = max(s.n, 1u) - 1u;      // (lim on the scalar side)
      const uint32_t e = (x < lim ? x : lim) << 2;
#ifdef K5_ASM_LOADS
      asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"(v) : "v"(e), "s"(s.src) : "memory");
#else
      v = *(const k5_u32x4*)((const char*)s.src + e);
#endif
    };
#ifndef K5_ASM_LOADS
// (compiler-tracked loads: the empty statement only pins the four words to one register tuple at the point of use, which keeps the register
// allocator from copying them out of a shared temporary right behind the load -- and waiting for vmcnt(0) there)
#define K5_WAIT_OLDEST(v) asm volatile("" : "+v"(v))
#elif defined(K5_DEBUG_WAIT0)
#define K5_WAIT_OLDEST(v) asm volatile("s_waitcnt vmcnt(0)" : "+v"(v) :: "memory")
#else
#define K5_WAIT_OLDEST(v) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "n"(K5_Q - 1) : "memory")
#endif
#ifdef K5_TWICE_BRANCH
#define K5_TWICE(av, t) do { if (t) K5_LDS_OR((av) & tmask4, (t)); } while (0)
#else
#define K5_TWICE(av, t) K5_LDS_OR((av) & tmask4, (t))
#endif

    // ================= pass A: marks =================
#ifdef K5_ABL_A_TWICE      // (timing probe, diagnostic builds only, WRONG results: pass A runs twice -- stamp 12 takes the first run, whose lists come from HBM, the "pass A" stamp the second,
    for (int a_rep = 0; a_rep < 2; a_rep++)      //  whose lists sit in the caches: what pass A costs when its memory side is as cheap as a prefetch could make it)
#endif
    {
      // strip entries mark the region before theirs (region 0's strip entries are not in the strip lists)
#ifndef K5_ABL_NOSTRIP     // (timing ablation, diagnostic builds only: no strip loops -- wrong results, the upper bound of what folding the strips into the main loops could give)
      for (int j0 = tid >> 2; j0 < nl; j0 += nthr >> 2) {
        uint32_t slen; const uint32_t* sp = strip_of(j0, slen);
        for (uint32_t e = (uint32_t)(tid & 3) * 4u; e < slen; e += 16u) {
          const k5_u32x4 v = *(const k5_u32x4*)(sp + e);
          const uint32_t nv = min(4u, slen - e);
          mark(v.x - (1u << rb));
          if (nv > 1) mark(v.y - (1u << rb));
          if (nv > 2) mark(v.z - (1u << rb));
          if (nv > 3) mark(v.w - (1u << rb));
        }
      }
#endif
      // (the first K5_Q loads go out behind the strip loop, so that the compiler's counter model sees the same six pending loads on both
      // ways into the main loop and waits with vmcnt(K5_Q - 1), not vmcnt(0))
      gen_reset();
      Step sd[K5_Q]; k5_u32x4 sv[K5_Q];
#pragma unroll
      for (int q = 0; q < K5_Q; q++) { gen(sd[q]); issue(sd[q], sv[q]); }
      // No exit from the middle of a round: a step with n == 0 (generator exhausted) is a no-op, so the loop tests sd[0] once per round.  (An
      // exit per step merges, in the structurized loop, the counter states behind each of the K5_Q loads at the loop header, and the compiler
      // then waits for vmcnt(0) at every step: one memory round trip per step instead of a K5_Q-deep pipeline.)
      while (sd[0].n) {
#pragma unroll
        for (int q = 0; q < K5_Q; q++) {
          K5_WAIT_OLDEST(sv[q]);
          // Marks only have to cover every real entry (pass B and the region table apply the exact rule): the last active lane also
          // marks the up-to-3 words it read past the chunk.
          const uint32_t W = (sd[q].n + 63u) >> 6;
          if (k5_lane_times(lane, W) < sd[q].n) {
            // all seen[] updates of the step first, then the twice[] updates (old & m is 0 or m: the update is unconditional, a no-op for
            // first marks -- cheaper than a branch per entry): one LDS round trip per step, not per entry
            const uint32_t a0 = sv[q].x >> sh_a, a1 = sv[q].y >> sh_a, a2 = sv[q].z >> sh_a, a3 = sv[q].w >> sh_a;
            // slots 1 and 2 without a branch: a slot beyond W ORs a zero mask (a no-op that returns the word) -- two scalar selects and two ANDs instead of
            // a compare, a select and a branch per slot and table (the scalar unit, one per CU, is the busier one in this loop); the fourth slot is rare
            const uint32_t k1 = W > 1u ? 0xFFFFFFFFu : 0u, k2 = W > 2u ? 0xFFFFFFFFu : 0u;
            const uint32_t t0 = sv[q].x >> sh_b, t1 = sv[q].y >> sh_b, t2 = sv[q].z >> sh_b, t3 = sv[q].w >> sh_b;
            const uint32_t b0 = 1u << (t0 & 31u), b1 = (1u << (t1 & 31u)) & k1, b2 = (1u << (t2 & 31u)) & k2, b3 = 1u << (t3 & 31u);      // the twice[] bits
            const uint32_t m0 = BLOOM ? bloom_mask(t0) : b0, m1 = BLOOM ? bloom_mask(t1) & k1 : b1, m2 = BLOOM ? bloom_mask(t2) & k2 : b2, m3 = BLOOM ? bloom_mask(t3) : b3;
            uint32_t o3 = 0;
#ifdef K5_ABL_A_NOLDS      // (timing ablation, diagnostic builds only: the marks dropped, the address arithmetic kept -- what pass A costs as a pure stream)
            const uint32_t sink = (swb + (a0 & smask4)) ^ m0 ^ (swb + (a1 & smask4)) ^ m1 ^ (swb + (a2 & smask4)) ^ m2 ^ a3 ^ m3;
            asm volatile("" :: "v"(sink));
            (void)o3; (void)b0; (void)b1; (void)b2; (void)b3;
#else
            const uint32_t o0 = K5_LDS_OR(swb + (a0 & smask4), m0);
            const uint32_t o1 = K5_LDS_OR(swb + (a1 & smask4), m1);
            const uint32_t o2 = K5_LDS_OR(swb + (a2 & smask4), m2);
            if (W > 3) o3 = K5_LDS_OR(swb + (a3 & smask4), m3);
            if (BLOOM) {
              K5_TWICE(a0, (o0 & m0) == m0 ? b0 : 0u);
              K5_TWICE(a1, (o1 & m1) == m1 ? b1 : 0u);
              K5_TWICE(a2, (o2 & m2) == m2 ? b2 : 0u);
              if (W > 3) K5_TWICE(a3, (o3 & m3) == m3 ? b3 : 0u);
            } else {
            K5_TWICE(a0, o0 & m0);
            K5_TWICE(a1, o1 & m1);
            K5_TWICE(a2, o2 & m2);
            if (W > 3) K5_TWICE(a3, o3 & m3);
            }
#endif
          }
          gen(sd[q]); issue(sd[q], sv[q]);
        }
      }
      // (the dummy loads of the exhausted generator stay in flight: nothing reads their registers)
#ifdef K5_ABL_A_TWICE
      if (a_rep == 0) { __syncthreads(); K5_STAMP(12); }
#endif
    }
    // Pass B streams the same lists again: its first K5_Q loads go out here, before the barrier, so that the wait for the slowest wave, the clear of
    // the region table and the strip loop hide the fill of its load pipeline (~2 us per pass otherwise).
    Step sdB[K5_Q]; k5_u32x4 svB[K5_Q];
    K5_GEN_RESET_B();
#pragma unroll
    for (int q = 0; q < K5_Q; q++) { K5_GEN_B(sdB[q]); issue(sdB[q], svB[q]); }
    __syncthreads();
    K5_STAMP(1);
    bool fallback = false;
    uint32_t nc = 0;
    const int nrounds = MULTI ? a.rounds : 1;
      {
      // ================= pass B: candidates (into the dead seen[] area) =================
      if (!MULTI) { uint4* h4 = (uint4*)htag; for (int w = tid; w < hclr_q; w += nthr) h4[w] = make_uint4(0, 0, 0, 0); }      // (MULTI: the table's area takes the candidates of all parts first)
      {
        // Candidates are appended to one dense array (positions + y/seed) through a counter in LDS: one atomic per wave and step.  (Per-wave segments
        // with a wave-uniform counter -- no atomic at all -- were measured and dropped: pass B gained 2 %, the two exact stages lost 20 % to the
        // segment -> slot mapping and to half-empty iterations.)
        // a strip entry whose own region stays below 2 is a candidate when the region before reaches 2
        for (int j0 = tid >> 2; j0 <
#ifdef K5_ABL_NOSTRIP
             0
#else
             nl
#endif
             ; j0 += nthr >> 2) {
          uint32_t slen; const uint32_t* sp = strip_of(j0, slen);
          const uint32_t ysn = rec[4 * j0 + 3];
          for (uint32_t e = (uint32_t)(tid & 3) * 4u; e < slen; e += 16u) {
            const k5_u32x4 v = *(const k5_u32x4*)(sp + e);
            const uint32_t nv = min(4u, slen - e);               // >= 1
            // (entry 0 is tested unconditionally: a load whose result is only used under a condition keeps the compiler's counter model
            // "pending" into the main loop below, which then waits for vmcnt(0) at every step)
            const bool a0 = !has2(v.x) && has2(v.x - (1u << rb));
            const bool a1 = nv > 1 && !has2(v.y) && has2(v.y - (1u << rb));
            const bool a2 = nv > 2 && !has2(v.z) && has2(v.z - (1u << rb));
            const bool a3 = nv > 3 && !has2(v.w) && has2(v.w - (1u << rb));
            const bool c0 = a0, c1 = a1, c2 = a2, c3 = a3;
            if (c0 | c1 | c2 | c3) {
              uint32_t idx = atomicAdd(&ctrl[C_NCAND], (uint32_t)c0 + (uint32_t)c1 + (uint32_t)c2 + (uint32_t)c3);
              if (idx + 4u <= pb_cap) {
                const uint16_t y16 = (uint16_t)ysn;
                if (c0) { sb_pos[idx] = v.x; sb_y[idx++] = y16; }
                if (c1) { sb_pos[idx] = v.y; sb_y[idx++] = y16; }
                if (c2) { sb_pos[idx] = v.z; sb_y[idx++] = y16; }
                if (c3) { sb_pos[idx] = v.w; sb_y[idx++] = y16; }
              }
            }
          }
        }
        Step (&sd)[K5_Q] = sdB; k5_u32x4 (&sv)[K5_Q] = svB;
        while (sd[0].n) {                                                 // (no exit inside a round, as in pass A)
  #pragma unroll
          for (int q = 0; q < K5_Q; q++) {
            const Step& s = sd[q];
            K5_WAIT_OLDEST(sv[q]);
            const uint32_t W = (s.n + 63u) >> 6;
            const uint32_t e0 = k5_lane_times(lane, W);
            // the four twice[] words unconditionally (no branch per entry slot; a lane's words past its own entries -- min(W, n - e0) of them --
            // belong to the next lane / list and are masked), the four answers as one bit mask
            const uint32_t mine = min(W, __builtin_elementwise_sub_sat(s.n, e0));
  #ifdef K5_ABL_B
            const uint32_t t0 = 0, t1 = 0, t2 = 0, b3 = ((sv[q].x ^ sv[q].y ^ sv[q].z ^ sv[q].w) == 0x12345678u) << 3;
  #else
            const uint32_t t0 = *K5_LDS((sv[q].x >> sh_a) & tmask4), t1 = *K5_LDS((sv[q].y >> sh_a) & tmask4);
            const uint32_t t2 = *K5_LDS((sv[q].z >> sh_a) & tmask4);
            // (the fourth slot only in steps of more than 192 entries -- one wave-uniform branch; lists of the default seeds on 3 Gbp hold ~180)
            uint32_t b3 = 0;
            if (W > 3u) b3 = __builtin_amdgcn_ubfe(*K5_LDS((sv[q].w >> sh_a) & tmask4), __builtin_amdgcn_ubfe(sv[q].w, sh_b, 5), 1) << 3;
  #endif
            uint32_t hits = (__builtin_amdgcn_ubfe(t0, __builtin_amdgcn_ubfe(sv[q].x, sh_b, 5), 1) | (__builtin_amdgcn_ubfe(t1, __builtin_amdgcn_ubfe(sv[q].y, sh_b, 5), 1) << 1) |
                             (__builtin_amdgcn_ubfe(t2, __builtin_amdgcn_ubfe(sv[q].z, sh_b, 5), 1) << 2) | b3) &
                            ((1u << mine) - 1u);
            // one reservation per lane with hits (8 % of the entries are candidates: a dozen lanes per step add to the same LDS word, which the
            // LDS serialises in as many cycles -- cheaper than four ballots, their counts and a prefix per entry)
            const uint32_t cnt = (uint32_t)__popc(hits);
            if (cnt) {
              const uint32_t ci = atomicAdd(&ctrl[C_NCAND], cnt);
              if (ci + cnt <= pb_cap) {
                // slot k of a lane goes to ci + (hits below k): no running index (and no register copy) between the four predicated store pairs,
                // the list's y / seed word in one register for all of them
                uint32_t y16 = s.ysn;
                asm volatile("" : "+v"(y16));
                const uint32_t c1 = ci + (hits & 1u), c2 = ci + (uint32_t)__popc(hits & 3u), c3 = ci + (uint32_t)__popc(hits & 7u);
                // (absolute LDS addresses: with compile-time sizes both bases are instruction offsets, a store pair costs two shifts)
                if (hits & 1u) { *K5_LDS(pb_pos + (ci << 2)) = sv[q].x; *K5_LDS16(pb_y + (ci << 1)) = (uint16_t)y16; }
                if (hits & 2u) { *K5_LDS(pb_pos + (c1 << 2)) = sv[q].y; *K5_LDS16(pb_y + (c1 << 1)) = (uint16_t)y16; }
                if (hits & 4u) { *K5_LDS(pb_pos + (c2 << 2)) = sv[q].z; *K5_LDS16(pb_y + (c2 << 1)) = (uint16_t)y16; }
                if (hits & 8u) { *K5_LDS(pb_pos + (c3 << 2)) = sv[q].w; *K5_LDS16(pb_y + (c3 << 1)) = (uint16_t)y16; }
              }
            }
            K5_GEN_B(sd[q]); issue(sd[q], sv[q]);
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      }
      __syncthreads();
      if (MULTI) {
        // The candidates of all parts sit in the table's area: part 0 (with its halo) moves to the arrays of the exact stages, every later part to its row in global memory
        // (one reservation per wave and part; a candidate in a region next to a seam belongs to both neighbours), then the table is cleared.
        const uint32_t na_raw = ctrl[C_NCAND];
        if (na_raw + 8u > pb_cap) fallback = true;
        const uint32_t na = min(na_raw, pb_cap);
        const unsigned long long below = (1ull << lane) - 1ull;
        for (uint32_t i0 = 0; i0 < na; i0 += nthr) {
          const uint32_t i = i0 + tid;
          const bool live = i < na;
          const uint32_t p = *K5_LDS(pb_pos + ((live ? i : 0u) << 2)), ys = *K5_LDS16(pb_y + ((live ? i : 0u) << 1));
#pragma unroll
          for (int d = 0; d < K5_MAX_ROUNDS; d++) if (d < nrounds) {
            const bool in = live && p - rf_lo[d] <= rf_m1[d];
            const unsigned long long bi = __ballot(in);
            if (bi) {
              uint32_t base = 0;
              if (lane == 0) base = atomicAdd(&ctrl[d == 0 ? C_NCAND0 : C_SPILL + d - 1], (uint32_t)__popcll(bi));
              base = __builtin_amdgcn_readfirstlane(base);
              const uint32_t j = base + (uint32_t)__popcll(bi & below);
              if (in) {
                if (d == 0) { if (j < (uint32_t)cand_cap) { candp[j] = p; candy[j] = (uint16_t)ys; } }
                else if (j < (uint32_t)a.spill_cap) spill_wg[(size_t)(d - 1) * a.spill_cap + j] = make_uint2(p, ys);
              }
            }
          }
        }
        __syncthreads();
        { uint4* h4 = (uint4*)htag; for (int w = tid; w < hclr_q; w += nthr) h4[w] = make_uint4(0, 0, 0, 0); }
        __syncthreads();
      }
    for (int rd = 0; rd < nrounds; rd++) {
      // this round's part of the genome as position ranges: [c_lo, c_lo + c_m1] the part itself, [f_lo, f_lo + f_m1] with one region either side
      uint32_t c_lo = 0, c_m1 = 0xFFFFFFFFu, f_lo = 0, f_m1 = 0xFFFFFFFFu;
      if (MULTI) {
        const uint64_t rsz64 = 1ull << rb, lo = (uint64_t)rd * a.round_regs * rsz64, hi = rd == nrounds - 1 ? (1ull << 32) : lo + (uint64_t)a.round_regs * rsz64;     // [lo, hi)
        const uint64_t flo = lo >= rsz64 ? lo - rsz64 : 0ull, fhi = hi + rsz64 < (1ull << 32) ? hi + rsz64 : (1ull << 32);
        c_lo = (uint32_t)lo; c_m1 = (uint32_t)(hi - 1ull - lo); f_lo = (uint32_t)flo; f_m1 = (uint32_t)(fhi - 1ull - flo);
      }
      auto in_core = [&](const uint32_t p) -> bool { return !MULTI || p - c_lo <= c_m1; };
      if (MULTI && rd > 0) {
        // a later round: its candidates were set aside in global memory by pass B (agent-scope loads: the lines may sit in this CU's L1 from the read-strand before);
        // the per-round counters back to zero, the region table cleared
        const uint32_t ns_raw = ctrl[C_SPILL + rd - 1];
        if (ns_raw > (uint32_t)a.spill_cap || ns_raw > (uint32_t)a.cand_limit) fallback = true;
        const uint32_t nsp = min(ns_raw, (uint32_t)min(a.spill_cap, cand_cap));
        const unsigned long long* src = (const unsigned long long*)(spill_wg + (size_t)(rd - 1) * a.spill_cap);
        for (uint32_t i0 = 0; i0 < nsp; i0 += 6u * (uint32_t)nthr) {        // (six loads per thread in flight: the whole row of a 1024-thread workgroup in one round trip)
          unsigned long long v[6];
#pragma unroll
          for (int k = 0; k < 6; k++) { const uint32_t i = i0 + (uint32_t)k * (uint32_t)nthr + (uint32_t)tid; v[k] = __hip_atomic_load(src + min(i, nsp - 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#pragma unroll
          for (int k = 0; k < 6; k++) { const uint32_t i = i0 + (uint32_t)k * (uint32_t)nthr + (uint32_t)tid; if (i < nsp) { candp[i] = (uint32_t)v[k]; candy[i] = (uint16_t)(v[k] >> 32); } }
        }
        { uint4* h4 = (uint4*)htag; for (int w = tid; w < hclr_q; w += nthr) h4[w] = make_uint4(0, 0, 0, 0); }
        if (tid == 0) { ctrl[C_NCAND] = ns_raw; ctrl[C_NEDGE] = 0; }
      }
      if (rd > 0) __syncthreads();          // (part 0: the barrier behind pass B / the dealing of the candidates)
      K5_STAMP(2);
      // Every count the device produced is clamped to the capacity of what it indexes before it bounds a loop: the reservation counter runs past cand_cap when a
      // read-strand has more candidates than slots (the stores are skipped, the read-strand falls back), so it is never used as it stands.
      const uint32_t nc_raw = ctrl[(MULTI && rd == 0) ? C_NCAND0 : C_NCAND];
      if (nc_raw > (uint32_t)a.cand_limit) fallback = true;
      nc = min(nc_raw, (uint32_t)cand_cap);
      // ================= exact stage 1: region table over the candidates =================
      // A wave pays the longest chain of LDS round trips among its lanes, so the rare cases are taken out of the main loops and worked off
      // densely afterwards: the overlap-strip marks here (2 % of the candidates, but some lane of most waves), the neighbour-region look-ups of
      // stage 2 below.  Their lists (region numbers, then candidate indexes) live in rec[] / srec[], dead since pass B.
      uint32_t* const elist = rec; const uint32_t ecap = 6u * (uint32_t)RC;                 // (stage 2's list: the whole area, one list for the workgroup)
      // Stage 1 in two steps.  (a) every candidate tries the FIRST slot of its region's probe sequence, in straight-line code: one compare-and-swap, and when the slot holds the
      // region already, the flag update -- the same three LDS round trips for every lane.  Two thirds of the candidates are done with that (the table is a third full).
      // (b) the others -- another region sits in their first slot -- are listed and probed on from the second slot, densely, together with the strip marks: a probing loop
      // costs a wave the longest sequence among its lanes (five at this load), and it now pays that once per 64 LISTED candidates, not once per 64 candidates.
      // The lists are PER WAVE (wlist: this wave's wcap words of rec[] / srec[], its count a scalar): no counter in LDS, and no barrier between the two steps -- a wave
      // works its own list off right behind its own iterations of (a), next to the waves still in (a).  Nothing orders the table's updates: a slot's tag never changes once
      // set, a region's probe sequence is fixed, and the flags and min / max are OR / MAX (tests/test_k5_table_order.py runs the interleavings on a host model).
      // A word of the list is a candidate index (below 2^16) or, with bit 31 set, the region a strip mark goes to.  An item beyond wcap is worked off on the spot by its
      // own lane: a full list costs a wave one divergent chain, never the read-strand a trip through the fall-back kernels.
      auto settle = [&](const uint32_t i, const uint32_t h, const uint32_t off) {      // candidate i sits in slot h
        atomicMax(&hmin[h], 0x10000u - off); atomicMax(&hmax[h], off + 1u);
        candp[i] = (h << 16) | off;                              // slot and offset: stage 2 reads the region back from the tag (no second probe sequence)
      };
      auto probe_on = [&](const uint32_t i) {                        // step (b) for candidate i, its strip mark included
        const uint32_t p = candp[i], r = p >> rb, off = p & rmask;
        const uint32_t h = k5_insert(htag, hmask, hshift, r, true, true);
        if (h != 0xFFFFFFFFu) {
          settle(i, h, off);
          if (off < ovl && r > 0 && k5_insert(htag, hmask, hshift, r - 1u, false) == 0xFFFFFFFFu) ctrl[C_OVERFLOW] = 1u;
        } else ctrl[C_OVERFLOW] = 1u;
      };
      if (!fallback) {
        uint32_t wn = 0;                                         // items of this wave so far (a scalar; it runs past wcap: those were taken on the spot)
        for (uint32_t i0 = 0; i0 < nc; i0 += nthr) {
          const uint32_t i = i0 + tid;
          const bool live = i < nc;
          const uint32_t p = candp[live ? i : 0u], r = p >> rb, off = p & rmask, r1 = r + 1u;
          const uint32_t h0 = k5_hash(r1, hshift);
          uint32_t prev = 0xFFFFFFFFu;
          if (live) prev = atomicCAS(&htag[h0], 0u, (r1 << 8) | K5_FA | K5_FC);
          const bool hit = live && (prev == 0u || (prev >> 8) == r1);
          if (hit) {
            if (prev != 0u) k5_again(htag, h0, prev, true);
            settle(i, h0, off);
          }
          const bool strip = hit && off < ovl && r > 0, later = live && !hit;      // the overlap strip also counts for the region before (ref: mapping.c:521-533)
          const unsigned long long bi = __ballot(strip | later);                  // (a lane has at most one item: a strip mark needs the hit)
          if (bi) {
            const uint32_t j = wn + (uint32_t)__popcll(bi & ((1ull << lane) - 1ull));
            wn += (uint32_t)__popcll(bi);
            if (strip | later) {
              if (j < wcap) wlist[j] = later ? i : (0x80000000u | (r - 1u));
              else if (later) probe_on(i);
              else if (k5_insert(htag, hmask, hshift, r - 1u, false) == 0xFFFFFFFFu) ctrl[C_OVERFLOW] = 1u;
            }
          }
        }
        K5_STAMP(10);
        // (b) ONE probing loop for both kinds (a lane's kind is data: which flags it sets, where its sequence starts).  The words were stored by other lanes of this wave:
        // a wave's LDS operations execute in order, so nothing but the compiler has to be told.
        __builtin_amdgcn_wave_barrier();
        const uint32_t nw = min(wn, wcap);
        K5_WL_COUNT(nw, wn - nw);
        for (uint32_t j = lane; j < nw; j += GM_WAVE) {
          const uint32_t w = wlist[j];
          const bool own = (w >> 31) == 0u;
          const uint32_t v = w & 0x7FFFFFFFu;                    // candidate index / region number
          const uint32_t p = candp[own ? v : 0u], r = own ? p >> rb : v, off = p & rmask;
          const uint32_t h = k5_insert(htag, hmask, hshift, r, own, own);
          if (h == 0xFFFFFFFFu) ctrl[C_OVERFLOW] = 1u;
          else if (own) {
            settle(v, h, off);
            if (off < ovl && r > 0 && k5_insert(htag, hmask, hshift, r - 1u, false) == 0xFFFFFFFFu) ctrl[C_OVERFLOW] = 1u;
          }
        }
      }
      __syncthreads();                                        // stage 2 needs every insert
      K5_STAMP(3);
      fallback = fallback || rec_over || ctrl[C_OVERFLOW] != 0u;
      // ================= exact stage 2: the reference's rule (ref: mapping.c:733-742), prune rules (gm_prune.hip), output =================
      if (!fallback) {
        unsigned long long* out = (unsigned long long*)a.out + (size_t)rs * a.out_cap;
        // The neighbour regions only matter near the region's ends: a candidate at least D + e_max away from both has no neighbour-region
        // candidate within D of it or of anything within e_max of it, so both rules see the same with the neighbours left out (83 % of the
        // members at 2 048-base regions; each look-up of an absent region is a full probe sequence).
        const uint32_t edge = a.D + (uint32_t)max(a.e_max, 0);
        auto emit = [&](const bool memb, const bool keep, const uint32_t p, const uint32_t i) {      // (called by whole waves)
          const unsigned long long bm = __ballot(memb), bk = __ballot(keep);
          if (bm) {
            uint32_t base = 0;
            // (C_NMEMB in front of the reservation the stores wait for: a member count kept per wave in a scalar and added once behind stage 2b was measured and dropped --
            // stage 2a 5 977 against 6 029 ticks, as much as the build without it moved: profiles/r08a_k5_exact_stage_stamps.txt)
            if (lane == 0) { atomicAdd(&ctrl[C_NMEMB], (uint32_t)__popcll(bm)); if (bk) base = atomicAdd(&ctrl[C_NKEEP], (uint32_t)__popcll(bk)); }
            base = __builtin_amdgcn_readfirstlane(base);
            if (keep) {
              const uint32_t slot = base + (uint32_t)__popcll(bk & ((1ull << lane) - 1ull));
              const uint32_t y16 = candy[i];
              if (slot < (uint32_t)a.out_cap) out[slot] = ((unsigned long long)p << 32) | ((unsigned long long)(y16 >> 4) << 16) | (y16 & 15u);
            }
          }
        };
        // (2a) every candidate: its region's tag; members away from the region's ends are decided here, the rest goes to the list.  Straight-line code: the three
        // table words of a candidate are read together, the cases are predicates, the list is appended to once per wave (the branchy form of this loop spent more
        // scalar instructions on its control flow than vector instructions on the work, and reloaded kernel arguments inside it).
  #ifndef K5_2A_BRANCHY
        {
          // (the kernel arguments of the rules as opaque scalars: left to itself the compiler re-loads them from the argument segment inside the loop, a memory
          // round trip per iteration; predicates combined with & and |, not && and ||: no branch per clause)
          const uint32_t do_prune = k_prune, Dv = k_D, emax_on = k_emax_on, emax = k_emax;
          const uint32_t rsz = 1u << rb;
          for (uint32_t i0 = 0; i0 < nc; i0 += nthr) {
            const uint32_t i = i0 + tid;
            const uint32_t valid = i < nc ? 1u : 0u;
            const uint32_t w = candp[valid ? i : 0u], h = w >> 16, off = w & 0xFFFFu;
            const uint32_t town = htag[h], mn = hmin[h], mx = hmax[h];
            const uint32_t r = (town >> 8) - 1u, p = (r << rb) | off;
            const uint32_t is_m = (town >> 1) & 1u /* K5_FB */, r_pos = r > 0u ? 1u : 0u;
            const uint32_t nb_m = do_prune & (((off < edge ? 1u : 0u) & r_pos) | (off + edge >= rsz ? 1u : 0u)), nb_o = (off < ovl ? 1u : 0u) & r_pos;
            const uint32_t core = in_core(p) ? 1u : 0u;                                      // (candidates of the halo regions are in the table, nothing more)
            const uint32_t nbv = valid & core & (is_m ? nb_m : nb_o);
            const bool nb = nbv != 0u;
            const unsigned long long bn = __ballot(nb);
            if (bn) {
              uint32_t base = 0;
              if (lane == 0) base = atomicAdd(&ctrl[C_NEDGE], (uint32_t)__popcll(bn));
              base = __builtin_amdgcn_readfirstlane(base);
              if (nb) {
                const uint32_t j = base + (uint32_t)__popcll(bn & ((1ull << lane) - 1ull));
                if (j < ecap) elist[j] = i; else ctrl[C_OVERFLOW] = 1u;
              }
            }
            const uint32_t fe = (town >> 4) & 1u /* K5_FE */, fd = (town >> 3) & 1u /* K5_FD */;
            const uint32_t span = (mx - 1u) - (0x10000u - mn);
            const uint32_t iso = fe | (fd & (span <= Dv ? 1u : 0u));                          // (1) isolation: three or more inside, or two at most D apart
            const uint32_t tight = emax_on & (span <= emax ? 1u : 0u);                        // (2) tight cluster
            const uint32_t membv = valid & core & is_m & (nbv ^ 1u), keepv = membv & ((iso & (tight ^ 1u)) | (do_prune ^ 1u));
            emit(membv != 0u, keepv != 0u, p, i);
          }
        }
  #else
        // (2a) every candidate: its region's tag; members away from the region's ends are decided here, the rest goes to the list
        for (uint32_t i0 = 0; i0 < nc; i0 += nthr) {
          const uint32_t i = i0 + tid;
          bool memb = false, keep = false; uint32_t p = 0;
          if (i < nc) {
            const uint32_t w = candp[i], h = w >> 16, off = w & 0xFFFFu, town = htag[h], r = (town >> 8) - 1u;
            p = (r << rb) | off;
            const bool is_m = (town & K5_FB) != 0u;
            const bool nb = is_m ? (a.prune && ((off < edge && r > 0) || off + edge >= (1u << rb))) : (off < ovl && r > 0);
            if (nb) {
              const uint32_t j = atomicAdd(&ctrl[C_NEDGE], 1u);
              if (j < ecap) elist[j] = i; else ctrl[C_OVERFLOW] = 1u;
            } else if (is_m) {
              memb = true; keep = true;
              if (a.prune) {
                const uint32_t co = (town & K5_FE) ? 3u : ((town & K5_FD) ? 2u : 1u);
                const uint32_t span = (hmax[h] - 1u) - (0x10000u - hmin[h]);
                keep = co >= 3u || (co == 2u && span <= a.D);                         // (1) isolation
                if (keep && a.e_max >= 0 && span <= (uint32_t)a.e_max) keep = false;    // (2) tight cluster
              }
            }
          }
          emit(memb, keep, p, i);
        }
  #endif
        __syncthreads();
        K5_STAMP(11);
        // (2b) the listed candidates, with the regions before / behind theirs
        const uint32_t ne = min(ctrl[C_NEDGE], ecap);
        for (uint32_t j0 = 0; j0 < ne; j0 += nthr) {
          const uint32_t j = j0 + tid;
          bool memb = false, keep = false; uint32_t p = 0, i = 0;
          if (j < ne) {
            i = elist[j];
            const uint32_t w = candp[i], hown = w >> 16, off = w & 0xFFFFu, town = htag[hown], r = (town >> 8) - 1u;
            p = (r << rb) | off;
            uint32_t tlf = 0, trt = 0;
            memb = (town & K5_FB) != 0u;
            uint32_t hlf = 0xFFFFFFFFu; bool have_lf = false;
            // (the filter: see has2r.  Flag B of the region before needs its own bit, flag C and min / max that bit and the one of the region before it)
            if (!memb && off < ovl && r > 0) { hlf = k5_find_maybe(htag, hmask, hshift, r - 1u, has2r(r - 1u), tlf); have_lf = true; memb = (tlf & K5_FB) != 0u; }
            if (memb) {
              keep = true;
              if (a.prune) {
                uint32_t hrt = 0xFFFFFFFFu; trt = 0;
                if (off < edge) { if (!have_lf && r > 0) hlf = k5_find_maybe(htag, hmask, hshift, r - 1u, has2r(r - 1u) | has2r(r - 2u), tlf); } else tlf = 0;
                if (off + edge >= (1u << rb)) hrt = k5_find(htag, hmask, hshift, r + 1u, trt);
                const uint32_t co = (town & K5_FE) ? 3u : ((town & K5_FD) ? 2u : 1u);
                const uint32_t omin = 0x10000u - hmin[hown], omax = hmax[hown] - 1u;
                const bool cl = (tlf & K5_FC) != 0u, cr = (trt & K5_FC) != 0u;
                const uint32_t rbase = r << rb;
                // (1) isolation: another candidate within D (two in the region: the other one is max - min away; three or more: keep)
                keep = co >= 3u || (co == 2u && omax - omin <= a.D);
                uint32_t lmin = 0, lmax = 0, rmin = 0, rmax = 0;
                if (cl) { lmin = 0x10000u - hmin[hlf]; lmax = hmax[hlf] - 1u; }
                if (cr) { rmin = 0x10000u - hmin[hrt]; rmax = hmax[hrt] - 1u; }
                if (!keep && cl) keep = p - (rbase - (1u << rb) + lmax) <= a.D;
                if (!keep && cr) keep = (rbase + (1u << rb) + rmin) - p <= a.D;
                // (2) tight cluster: everything in the three regions (which cover p -+ (D + e_max)) spans at most e_max positions
                if (keep && a.e_max >= 0) {
                  uint32_t gmin = rbase + omin, gmax = rbase + omax;
                  if (cl) gmin = rbase - (1u << rb) + lmin;
                  if (cr) gmax = rbase + (1u << rb) + rmax;
                  if (gmax - gmin <= (uint32_t)a.e_max) keep = false;
                }
              }
            }
          }
          emit(memb, keep, p, i);
        }
      }
      if (MULTI && rd + 1 < nrounds) { __syncthreads(); if (ctrl[C_OVERFLOW] != 0u) fallback = true; }
    }
    __syncthreads();
    if (ctrl[C_OVERFLOW] != 0u) fallback = true;                    // (the list of stage 2 ran over)
    // More kept than K2's LDS tier takes (1 read-strand in 8 000 on the benchmark genome): k_prune's finer bins get the last word before the heavy tier.  The members are
    // all here, so they go to the read-strand's raw row as K1 without the fused rules would have left them, and only k_prune runs for it (list pl_list).  (Sending these
    // read-strands back through the lane-per-list kernel cost 1-6 ms per launch: its few large-LDS workgroups queue behind the other stream's pass-1 workgroups.)
    bool prune_only = false;
    if (!fallback && a.prune && ctrl[C_NKEEP] > (uint32_t)a.out_cap) {
      if (!(MULTI && nrounds > 1) && a.raw_out && ctrl[C_NMEMB] <= (uint32_t)a.raw_cap) {      // (the members of earlier rounds have left the LDS)
        prune_only = true;
        unsigned long long* raw = (unsigned long long*)a.raw_out + (size_t)rs * a.raw_cap;
        // slab by slab, as the sweep kernels leave them (K1b prunes a long row per slab segment: surv_seg)
        for (int sl = 0; sl < a.n_slabs; sl++) {
        for (uint32_t i0 = 0; i0 < nc; i0 += nthr) {
          const uint32_t i = i0 + tid;
          bool memb = false; uint32_t p = 0;
          if (i < nc) {
            const uint32_t w = candp[i], h = w >> 16, off = w & 0xFFFFu, town = htag[h], r = (town >> 8) - 1u;
            p = (r << rb) | off;
            if ((int)(p >> ix.slab_bits) == sl || (sl == a.n_slabs - 1 && (int)(p >> ix.slab_bits) >= a.n_slabs)) {
              memb = (town & K5_FB) != 0u;
              if (!memb && off < ovl && r > 0) { uint32_t tlf; k5_find_maybe(htag, hmask, hshift, r - 1u, has2r(r - 1u), tlf); memb = (tlf & K5_FB) != 0u; }
            }
          }
          const unsigned long long bm = __ballot(memb);
          if (bm) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&ctrl[C_NRAW], (uint32_t)__popcll(bm));
            base = __builtin_amdgcn_readfirstlane(base);
            if (memb) {
              const uint32_t slot = base + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull)), y16 = candy[i];
              if (slot < (uint32_t)a.raw_cap) raw[slot] = ((unsigned long long)p << 32) | ((unsigned long long)(y16 >> 4) << 16) | (y16 & 15u);
            }
          }
        }
        __syncthreads();
        if (tid == 0 && a.surv_seg) { if (sl == 0) a.surv_seg[(size_t)rs * (a.n_slabs + 1)] = 0u; a.surv_seg[(size_t)rs * (a.n_slabs + 1) + sl + 1] = ctrl[C_NRAW]; }
        }
      } else fallback = true;
    }
    K5_STAMP(4);
#ifdef K5_STAMPS
    if (tid == 0) { atomicAdd(&k5_stamps[6], (unsigned long long)nc); if (fallback) atomicAdd(&k5_stamps[7], 1ull); }
#endif
#ifdef GM_TUNING
    if (tid == 0 && (fallback || prune_only)) atomicAdd(&k5_paths[fallback ? 1 : 2], 1ull);      // (the read-strands taken: once per workgroup, behind the loop)
    if (tid == 0) { atomicAdd(&k5_wave_lists[0], (unsigned long long)ctrl[C_WLISTED]); atomicAdd(&k5_wave_lists[1], (unsigned long long)ctrl[C_WSPOT]); ctrl[C_WSPOT] = 0; }      // (C_WLISTED: zeroed below)
#endif
    if (tid == 0) {
      if (fallback) {                                          // candidates beyond the LDS tiers: the slab-sweep kernel redoes this read-strand
        const uint32_t f = atomicAdd(a.fb_cnt, 1u);
        if (f < (uint32_t)a.fb_cap) a.fb_list[f] = (uint32_t)rs; else GS_ADD(a.stats, GS_OVERFLOW_SURV, 1ull);
      } else if (prune_only) {                                 // members in the raw row, segment ends written above
        const uint32_t nm = ctrl[C_NRAW];
        a.surv_cnt[rs] = nm;
        GS_ADD(a.stats, GS_SURVIVORS, (unsigned long long)nm);
        const uint32_t f = atomicAdd(a.pl_cnt, 1u);
        if (f < (uint32_t)a.pl_cap) a.pl_list[f] = (uint32_t)rs; else GS_ADD(a.stats, GS_OVERFLOW_SURV, 1ull);
      } else {
        const uint32_t nm = ctrl[C_NMEMB], nk = ctrl[C_NKEEP];
        a.surv_cnt[rs] = nm;
        GS_ADD(a.stats, GS_SURVIVORS, (unsigned long long)nm);
        if (a.prune) GS_ADD(a.stats, GS_PRUNED, (unsigned long long)(nm - nk));
        const bool heavy = nk > (uint32_t)a.out_cap;
        if (a.prune) a.out_cnt[rs] = heavy ? 0xFFFFFFFFu : nk;
        if (heavy) {
          const uint32_t hs = atomicAdd(a.heavy_cnt, 1u);
          if (hs < (uint32_t)a.heavy_cap) a.heavy_list[hs] = (uint32_t)rs; else GS_ADD(a.stats, GS_OVERFLOW_SURV, 1ull);
        }
      }
      for (int c = 0; c < C_NLISTS; c++) ctrl[c] = 0;
      *cnl = 0; ctrl[C_NRAW] = 0; if (MULTI) ctrl[C_NCAND0] = 0;
      if (MULTI) for (int d = 0; d < K5_MAX_ROUNDS - 1; d++) ctrl[C_SPILL + d] = 0;
    }
    { uint4* t4 = (uint4*)smem; for (int w = tid; w < tab_q; w += nthr) t4[w] = make_uint4(0, 0, 0, 0); }
    K5_STAMP(5);
  }
#ifdef GM_TUNING
  if (tid == 0 && it > 0) atomicAdd(&k5_paths[0], (unsigned long long)it);
#endif
  for (int d = GM_WAVE / 2; d > 0; d >>= 1) { my_lookups += __shfl_down(my_lookups, d); my_entries += __shfl_down(my_entries, d); }
  if (lane == 0) { GS_ADD(a.stats, GS_LOOKUPS, my_lookups); GS_ADD(a.stats, GS_ENTRIES, my_entries); }
}
#undef K5_WL_COUNT
