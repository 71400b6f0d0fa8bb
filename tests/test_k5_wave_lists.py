"""k_lookup_v5's exact stage 1 with per-wave lists and no barrier between its two steps (first-slot tries; probe-ons and strip marks).  A wave's list is a segment of rec[] whose
size depends on the number of waves; GM_K5_WLIST caps it (tuning builds), so that nearly every wave fills its list and the items beyond it are worked off on the spot by their own lanes.  Every case
asks for the reference's SAM byte for byte, for the survivor counts and the fall-backs of the same case with full lists -- a full wave list never sends a read-strand
to the fall-back kernels -- and for the listed / on-the-spot counts the cap implies."""
import os
import ctypes as C
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
    out = (C.c_ulonglong * 3)()
    assert gm.lib().gm_debug_k5_paths(out) == 0
    return [int(x) for x in out]


def _wave_lists(gm):
    """items of exact stage 1 that went through a wave's list, items taken on the spot, since the last call"""
    out = (C.c_ulonglong * 2)()
    assert gm.lib().gm_debug_k5_wave_lists(out) == 0
    return [int(x) for x in out]


def _run(gm, env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        _paths(gm); _wave_lists(gm)
        got, st = fn()
        kern = gm.lib().gm_last_lookup_kernel().decode()
        n, fb, po = _paths(gm)
        listed, spot = _wave_lists(gm)
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    print("%s kernel %s: %d read-strands, %d fell back, %d to k_prune alone, survivors %d, pruned %d, items listed %d, on the spot %d"
          % (env, kern, n, fb, po, st["survivors"], st["survivors_pruned"], listed, spot))
    return dict(sam=got, survivors=st["survivors"], pruned=st["survivors_pruned"], kern=kern, n=n, fb=fb, po=po, listed=listed, spot=spot)


def _letters(gm, tag):
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
    return fn, sam, 2 * len(reads)


def _colours(gm, tag):
    contigs, reads, sam = oa.load_golden("cfg4s_50col_2Mbp")

    def fn():
        p = gm.default_params_cs()
        ix = gm.Index(contigs, params=p)
        s = gm.Session(ix, params=p, max_batch_reads=4096)
        got = oa.sam_header(contigs) + s.map_reads_cs(reads)
        st = s.stats
        s.close(); ix.close()
        return got, st
    return fn, sam, 2 * len(reads)


def _pairs(gm, tag):
    g = oa.load_golden_pairs("cfg5s_2x150_1Mbp")

    def fn():
        ix = gm.Index(g["contigs"], names=g["contig_names"])
        s = gm.Session(ix, max_batch_reads=4096)
        got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs(g["m1"], g["m2"], g["names1"], g["names2"], mode=g["mode"],
                                                                            min_insert=g["ins"][0], max_insert=g["ins"][1])
        st = s.stats
        s.close(); ix.close()
        return got, st
    return fn, g["sam"], 1


V5 = {"GM_SLAB_BITS": "18", "GM_K1_V5": "1"}
# (workload, environment beside V5, option golden, GM_K5_WLIST or None for the full segment, kernel)
CASES = [
    (_letters, {}, None, "4", "k_lookup_v5"),                                        # nearly every wave's list overflows
    (_letters, {}, None, "0", "k_lookup_v5"),                                        # no list at all
    (_letters, {"GM_K1_THREADS": "64"}, None, "4", "k_lookup_v5"),                   # one wave: the whole of rec[] is its segment
    (_letters, {"GM_K1_THREADS": "256"}, None, "4", "k_lookup_v5"),                  # four waves
    (_letters, {"GM_K5_LSW": "12"}, None, None, "k_lookup_v5"),                      # a small table, long probe sequences: most candidates are deferred
    (_letters, {"GM_K5_LSW": "12"}, None, "4", "k_lookup_v5"),
    (_letters, {"GM_K5_LSW": "12"}, "regions_12_200", "4", "k_lookup_v5"),           # 4 096-base regions, 200-base strips: many strip marks and edge items
    (_letters, {"GM_K5_ROUNDS": "3"}, "regions_12_200", "4", "k_lookup_v5_rounds"),
    (_letters, {"GM_NO_BUCKETS": "1", "GM_K5_ROUNDS": "2"}, None, "4", "k_lookup_v5_rounds"),      # the counts start at zero in every round; halo regions
    (_letters, {"GM_K5_ROUNDS": "3"}, None, "4", "k_lookup_v5_rounds"),
    (_letters, {"GM_K5_HALF": "1", "GM_K5_ROUNDS": "2"}, None, "4", "k_lookup_v5_half"),           # eight waves, the Bloom shape
    (_letters, {"GM_SCAP": "1024", "GM_SCAP2": "64"}, None, "4", "k_lookup_v5"),     # the prune_only tail
    (_colours, {"GM_K5_LSW": "12"}, None, "4", "k_lookup_v5"),
    (_pairs, {"GM_K5_ROUNDS": "2"}, None, "4", "k_lookup_v5_rounds"),
]
_full = {}            # the same case with GM_K5_WLIST unset: mapped once per (workload, environment, option golden)


def _id(case):
    load, extra, tag, wlist, _ = case
    return "-".join([load.__name__.strip("_")] + ["%s=%s" % kv for kv in extra.items()] + ([tag] if tag else []) + ["wlist=%s" % (wlist if wlist is not None else "full")])


@pytest.mark.gpu
@pytest.mark.parametrize("load,extra,tag,wlist,want_kern", CASES, ids=[_id(c) for c in CASES])
def test_short_wave_lists_change_nothing_but_the_counts(gm, load, extra, tag, wlist, want_kern):
    fn, sam, n_min = load(gm, tag)
    env = dict(V5, **extra)
    key = (load.__name__, tuple(sorted(extra.items())), tag)
    assert "GM_K5_WLIST" not in os.environ
    if key not in _full: _full[key] = _run(gm, env, fn)
    full = _full[key]
    got = full if wlist is None else _run(gm, dict(env, GM_K5_WLIST=wlist), fn)
    for r in (full, got):
        assert r["kern"] == want_kern, r["kern"]
        assert r["n"] >= n_min and 10 * r["fb"] <= r["n"], (r["n"], r["fb"])      # the exact stages decided at least nine read-strands in ten
    assert got["sam"] == sam
    assert (got["survivors"], got["pruned"]) == (full["survivors"], full["pruned"])
    assert got["fb"] == full["fb"], (got["fb"], full["fb"])      # a full wave list never makes a read-strand fall back
    assert full["listed"] > 0
    if wlist == "0": assert got["listed"] == 0 and got["spot"] > 0, (got["listed"], got["spot"])
    if wlist == "4": assert got["listed"] > 0 and got["spot"] > 0, (got["listed"], got["spot"])
    if "GM_SCAP2" in extra: assert got["po"] >= 1, got["po"]
