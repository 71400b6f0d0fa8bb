"""k_lookup_v5's exact stages with the shortened LDS chains: neighbour-region look-ups filtered by twice[], stage 1(b) as one loop over the deferred candidates
and the strip marks.  The GPU tests force the shapes where those paths can go wrong (a small region table, rounds with halo regions
and seams, the Bloom / half shape, the prune_only tail, wide overlap strips) and ask for the reference's SAM byte for byte; the host test restates the filter's
proof on a model of the two passes."""
import os
import numpy as np
import pytest
from tests import oracle_api as oa


@pytest.fixture(scope="module")
def gm():
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    from shrimp_amd import gmapper
    if gmapper.lib().gm_device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return gmapper


def _paths(gm):
    """read-strands k_lookup_v5 took since the last call, those handed to the fall-back kernels, those handed to k_prune alone (tuning builds count them)"""
    import ctypes as C
    out = (C.c_ulonglong * 3)()
    assert gm.lib().gm_debug_k5_paths(out) == 0
    return [int(x) for x in out]


def _run(gm, env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        _paths(gm)
        got, st = fn()
        kern = gm.lib().gm_last_lookup_kernel().decode()
        n, fb, po = _paths(gm)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    print("kernel %s: %d read-strands, %d fell back, %d to k_prune alone, survivors %d, pruned %d" % (kern, n, fb, po, st["survivors"], st["survivors_pruned"]))
    return got, st, kern, n, fb, po


def _first_diff(a, b):
    for i, (x, y) in enumerate(zip(a.split(b"\n"), b.split(b"\n"))):
        if x != y: return i, x[:300], y[:300]
    return -1, b"<length>", b"<length>"


V5 = {"GM_SLAB_BITS": "18", "GM_K1_V5": "1"}
LS_CASES = [
    # a small region table (k_lookup_v5<0>): long probe sequences, absent neighbour regions at every look-up
    (dict(V5, GM_K5_LSW="12"), None, "k_lookup_v5"),
    # halo regions and seams next to the filter: the exact stages per half / per third of the genome
    ({"GM_NO_BUCKETS": "1", "GM_K1_V5": "1", "GM_K5_ROUNDS": "2"}, None, "k_lookup_v5_rounds"),
    (dict(V5, GM_K5_ROUNDS="3"), None, "k_lookup_v5_rounds"),
    # the half shape: twice[] set from the Bloom test
    (dict(V5, GM_K5_HALF="1", GM_K5_ROUNDS="2"), None, "k_lookup_v5_half"),
    # overlap strips of 200 bases in 4 096-base regions: many strip candidates, strip marks and look-ups of the region before; small table, then three parts
    (dict(V5, GM_K5_LSW="12"), "regions_12_200", "k_lookup_v5"),
    (dict(V5, GM_K5_ROUNDS="3"), "regions_12_200", "k_lookup_v5_rounds"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("env,tag,want_kern", LS_CASES, ids=lambda v: ",".join("%s=%s" % kv for kv in v.items() if kv[0] != "GM_K1_V5") if isinstance(v, dict) else str(v))
def test_letter_space_small_tables_rounds_and_half_shape(gm, env, tag, want_kern):
    contigs, reads, sam = oa.load_golden("cfg2s_100bp_2Mbp")
    p = gm.default_params()
    if tag:
        sam = oa.load_option_sam("cfg2s_100bp_2Mbp", tag)
        for k, v in oa.OPTION_CASES[tag][2].items(): setattr(p, k, v)

    def fn():
        ix = gm.Index(contigs, params=p)
        s = gm.Session(ix, params=p, max_batch_reads=4096)
        got = oa.sam_header(contigs) + s.map_reads(reads)
        st = s.stats
        s.close(); ix.close()
        return got, st
    got, st, kern, n, fb, po = _run(gm, env, fn)
    assert kern == want_kern, kern
    assert n >= 2 * len(reads) and 10 * fb <= n, (n, fb)          # the exact stages decided at least nine read-strands in ten
    assert got == sam, (_first_diff(got, sam), st)


@pytest.mark.gpu
def test_prune_only_tail_filters_the_region_before(gm):
    """a K2 tier of 64: read-strands that keep more leave their members in the raw row through the prune_only tail (its look-up of the region before is filtered)"""
    contigs, reads, sam = oa.load_golden("cfg2s_100bp_2Mbp")

    def fn():
        ix = gm.Index(contigs)
        s = gm.Session(ix, max_batch_reads=4096)
        got = oa.sam_header(contigs) + s.map_reads(reads)
        st = s.stats
        s.close(); ix.close()
        return got, st
    got, st, kern, n, fb, po = _run(gm, dict(V5, GM_SCAP="1024", GM_SCAP2="64"), fn)
    assert kern == "k_lookup_v5", kern
    assert po >= 1 and 10 * fb <= n, (n, fb, po)
    assert got == sam, (_first_diff(got, sam), st)


@pytest.mark.gpu
def test_paired_long_reads_through_the_rounds_kernel(gm):
    g = oa.load_golden_pairs("cfg5s_2x150_1Mbp")

    def fn():
        ix = gm.Index(g["contigs"], names=g["contig_names"])
        s = gm.Session(ix, max_batch_reads=4096)
        got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs(g["m1"], g["m2"], g["names1"], g["names2"], mode=g["mode"],
                                                                            min_insert=g["ins"][0], max_insert=g["ins"][1])
        st = s.stats
        s.close(); ix.close()
        return got, st
    got, st, kern, n, fb, po = _run(gm, dict(V5, GM_K5_ROUNDS="2"), fn)
    assert kern == "k_lookup_v5_rounds", kern
    assert n > 0 and 10 * fb <= n, (n, fb)
    assert got == g["sam"], (_first_diff(got, g["sam"]), st)


@pytest.mark.gpu
def test_colour_space_small_table(gm):
    contigs, reads, sam = oa.load_golden("cfg4s_50col_2Mbp")

    def fn():
        p = gm.default_params_cs()
        ix = gm.Index(contigs, params=p)
        s = gm.Session(ix, params=p, max_batch_reads=4096)
        got = oa.sam_header(contigs) + s.map_reads_cs(reads)
        st = s.stats
        s.close(); ix.close()
        return got, st
    got, st, kern, n, fb, po = _run(gm, dict(V5, GM_K5_LSW="12"), fn)
    assert kern == "k_lookup_v5", kern
    assert n >= 2 * len(reads) and 10 * fb <= n, (n, fb)
    assert got == sam, (_first_diff(got, sam), st)


@pytest.mark.parametrize("bloom", [False, True])
def test_twice_bit_filter_on_a_model_of_the_two_passes(bloom):
    """The proof above has2r in gm_lookup5_kernel.inc, restated on the host: pass A's marks into folded seen[] / twice[] bit tables, pass B's candidates (own bit set, or
    a strip entry whose own bit is clear and whose region before has it set), the region table's mark counts.  A region with flag B has its twice[] bit set; a region
    with a candidate inside has its own bit or the bit of the region before set -- so a clear bit answers the membership look-up, two clear bits the prune look-up."""
    rng = np.random.Generator(np.random.PCG64(5))
    rb, ovl, lsw = 6, 9, 5                                      # 64-base regions, 9-base strips; seen[]: 2^5 words, twice[]: 2^2 words -- every bit aliases many regions
    nreg = 1 << 13
    for trial in range(20):
        # clustered entries (a "mapping" region, its neighbours) over a background of single ones
        centre = rng.integers(1, nreg - 1, size=6)
        pos = np.concatenate([rng.integers(0, nreg << rb, size=300), (np.repeat(centre, 40) << rb) + rng.integers(-70, 134, size=240)]).astype(np.int64)
        pos = np.unique(np.clip(pos, 0, (nreg << rb) - 1))       # list entries are distinct positions
        rng.shuffle(pos)
        reg, off = pos >> rb, pos & ((1 << rb) - 1)
        strip = (off < ovl) & (reg > 0)
        seen = np.zeros(1 << lsw, dtype=np.uint32); twice = np.zeros(1 << (lsw - 3), dtype=np.uint32)

        def masks(r):
            t = r >> lsw
            m1 = 1 << (t & 31)
            return m1, (m1 | (2 << ((t + (((t >> 5) & 3) << 2)) & 31))) & 0xFFFFFFFF if bloom else m1

        def has2(r):
            return bool((int(twice[r & ((1 << (lsw - 3)) - 1)]) >> ((r >> lsw) & 31)) & 1)
        marks = {}
        for r in list(reg[strip] - 1) + list(reg):              # strip loop, then the main loop
            r = int(r); m1, m = masks(r)
            old = int(seen[r & ((1 << lsw) - 1)]); seen[r & ((1 << lsw) - 1)] = old | m
            if (old & m) == m: twice[r & ((1 << (lsw - 3)) - 1)] |= np.uint32(m1)
            marks[r] = marks.get(r, 0) + 1
        cand = np.array([has2(int(r)) or (bool(s) and has2(int(r) - 1)) for r, s in zip(reg, strip)])
        tab_marks, tab_inside = {}, {}
        for r, s in zip(reg[cand], strip[cand]):
            r = int(r)
            tab_marks[r] = tab_marks.get(r, 0) + 1; tab_inside[r] = tab_inside.get(r, 0) + 1
            if s: tab_marks[r - 1] = tab_marks.get(r - 1, 0) + 1
        assert any(v >= 2 for v in tab_marks.values()) and any(not has2(r) for r in tab_inside)     # (the model reaches both flags, and strip candidates in regions with a clear bit)
        for r, c in tab_marks.items():
            assert c <= marks[r]
            if c >= 2: assert has2(r), (trial, r)                                      # flag B
            if marks[r] >= 2: assert c == marks[r], (trial, r)                         # (exactness: every entry of a region with count >= 2 is a candidate)
        for r in tab_inside:
            assert has2(r) or (r > 0 and has2(r - 1)), (trial, r)                       # flags C / D / E, min / max
