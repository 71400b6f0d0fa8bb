"""Paired mode at its edges: pairs that sit ON the limits the paired kernels compare against (tools/make_golden.py pair_edges_cases).

  pair_edges_<mode>       mates of 40 and 60 bases under -I 200,400, cut from fragments of f bases: per fragment strand, f = t - 24 ... t + 24 about the lower and the upper
                          bound (the reference pairs a fragment iff 180 + s <= f <= 420 + s, s = 0 / 100 / 60 / 40 for opp-in / opp-out / col-fw / col-bw: the bound is one
                          base wide, and col-fw / col-bw differ only because the mates' lengths do), a series shifted by a 2-base deletion in mate 2, pairs whose mates
                          lie at matching offsets of two contigs, and pairs at the contigs' first and last bases (clipped windows).  Default, --no-half-paired, -n 3, both.
  pair_edges_cs_<mode>    the same as colour-space pairs (opp-in, col-bw), default and --no-half-paired
  pair_heap_tandem/_ties  60 pairs inside a tandem repeat under -I 0,2000: far more window pairs than the 30 slots of the pass-1 pair heap

Without a GPU: the oracle equals the reference on every run, and the fixtures are shown to discriminate from the reference's SAM alone.  With one: the product equals
the reference in one sub-batch, in sub-batches of 64 under both pipeline orders, on the exact mate-pair path (GM_MP_EXACT) and on the release build."""
import os, re, subprocess, sys
import numpy as np
import pytest
from tests import oracle_api as oa

PAIR_MODES = ["opp-in", "opp-out", "col-fw", "col-bw"]
SHIFT = {"opp-in": 0, "opp-out": 100, "col-fw": 60, "col-bw": 40}           # the reference pairs a fragment iff 180 + SHIFT <= f <= 420 + SHIFT
# tag -> (oracle options, gm_pair_opts_t fields, gm_params_t fields)
OPTS = {None: ("", {}, {}), "pe_nhp": ("half-paired=0", dict(half_paired=0), {}), "pe_n3": ("mp-match-mode=3", dict(match_mode=3), {}),
        "pe_n3_nhp": ("mp-match-mode=3;half-paired=0", dict(match_mode=3, half_paired=0), {}), "ph_o3_strata": ("strata=1;report=3", {}, dict(strata=1, num_outputs=3, num_tmp_outputs=23))}
LS_RUNS = [("pair_edges_" + m, t) for m in PAIR_MODES for t in (None, "pe_nhp", "pe_n3", "pe_n3_nhp")]
CS_RUNS = [("pair_edges_cs_" + m, t) for m in ("opp-in", "col-bw") for t in (None, "pe_nhp")]
HEAP_RUNS = [(b, t) for b in ("pair_heap_tandem", "pair_heap_ties") for t in (None, "ph_o3_strata")]
RUNS = LS_RUNS + CS_RUNS + HEAP_RUNS
run_id = lambda r: r[0] + ("@" + r[1] if r[1] else "")


def _first_diff(a: bytes, b: bytes):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y: return i, x[:300], y[:300]
    return min(len(la), len(lb)), b"<eof>", b"<eof>"


_GOLDEN = {}
def golden(base, tag=None):
    """the fixture's inputs and the reference's SAM of one run"""
    if base not in _GOLDEN: _GOLDEN[base] = oa.load_golden_pairs(base)
    g = _GOLDEN[base]
    return g, (g["sam"] if tag is None else oa.load_option_sam(base, tag))


_ORACLE = {}
def oracle_run(base, tag, swapped=False):
    """the oracle on one run, once per session: header + SAM, (anchors, windows), (pairs whose heap filled, evictions)"""
    key = (base, tag, swapped)
    if key not in _ORACLE:
        g, _ = golden(base, tag)
        cs = "_cs_" in base
        opts = ";".join(x for x in ("colour=1" if cs else "", OPTS[tag][0]) if x)
        o = oa.Session(g["contigs"], g["contig_names"], opts=opts or None)
        if cs: o.set(True, True)                                                  # --sam-unaligned, as the colour-space goldens were made
        o.set_pairing(g["mode"], *g["ins"])
        a, b, na, nb = (g["m2"], g["m1"], g["names2"], g["names1"]) if swapped else (g["m1"], g["m2"], g["names1"], g["names2"])
        sam = oa.sam_header(g["contigs"], g["contig_names"]) + o.map_pairs_sam(a, b, na, nb, nthreads=4)
        _ORACLE[key] = (sam, o.last_pair_counts(), o.last_pair_heap_counts())
        o.close()
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_oracle_equals_the_reference_on_the_pair_edge_goldens(oracle_lib, run):
    _, want = golden(*run)
    got = oracle_run(*run)[0]
    assert got == want, _first_diff(got, want)


def paired_names(sam):
    """names of the pairs the SAM holds as proper pairs (flag 0x2)"""
    return {l.split(b"\t")[0] for l in sam.split(b"\n") if l and not l.startswith(b"@") and int(l.split(b"\t")[1]) & 2}


def series_of(run):
    """{(series, strand): [(f, paired)] by rising f} of the sweep (lo / hi) and shifted (slo / shi) series, and {name: paired} of the cross-contig (x) and ends (e) pairs"""
    g, sam = golden(*run)
    got = paired_names(sam)
    sweep, other = {}, {}
    for n in g["names1"]:
        n = n[:-2]; t = n.split(b"_")
        if t[0] in (b"lo", b"hi", b"slo", b"shi"): sweep.setdefault((t[0].decode(), t[1].decode()), []).append((int(t[2]), n in got))
        else: other[n.decode()] = n in got
    for v in sweep.values(): v.sort()
    return sweep, other


def flips(v): return [i for i in range(len(v) - 1) if v[i][1] != v[i + 1][1]]
def has_hole(v): p = [i for i, (_, x) in enumerate(v) if x]; return bool(p) and (p[-1] - p[0] + 1) != len(p)


@pytest.mark.parametrize("run", [r for r in LS_RUNS + CS_RUNS if r[1] in (None, "pe_n3")], ids=run_id)
def test_fixture_sweeps_cross_each_bound_once_and_one_base_wide(run):
    """default and -n 3 runs: each plain series has >= 8 paired and >= 8 unpaired fragments on either side of exactly one transition, at the same f on both fragment
    strands (in letter space at the f the bound predicts); the shifted series changes at another f than the plain one (and once, in the default run)"""
    sweep, _ = series_of(run)
    for which in ("lo", "hi"):
        p, m = sweep[(which, "p")], sweep[(which, "m")]
        assert len(p) == len(m) == 49
        for v in (p, m):
            assert len(flips(v)) == 1, (which, v)
            assert sum(x for _, x in v) >= 8 and sum(not x for _, x in v) >= 8, (which, v)
        assert p == m, which
        if "_cs_" not in run[0]:
            s = SHIFT[run[0][len("pair_edges_"):]]
            inner = 180 + s if which == "lo" else 420 + s                              # the last f the reference pairs
            assert dict(p)[inner] and not dict(p)[inner + (-1 if which == "lo" else 1)], (which, inner)
        sh = sweep[("s" + which, "p")]
        assert [f for f, _ in sh] == [f for f, _ in p]
        assert flips(sh) and flips(sh)[0] != flips(p)[0], (which, sh)
        if run[1] is None: assert len(flips(sh)) == 1, (which, sh)


@pytest.mark.parametrize("run", LS_RUNS + CS_RUNS, ids=run_id)
def test_fixture_cross_contig_pairs_never_pair_and_contig_ends_decide(run):
    """mates at matching offsets of two contigs pair only if cn is ignored: the reference pairs none.  At the contigs' ends a window is clipped, which moves its start:
    at each end and strand some of the eight fragments just inside the bounds are paired and some are not"""
    _, other = series_of(run)
    x = {n: v for n, v in other.items() if n.startswith("x_")}; e = {n: v for n, v in other.items() if n.startswith("e_")}
    assert len(x) == 20 and not any(x.values()), x
    assert len(e) == 64
    for grp in sorted({n.rsplit("_", 2)[0] for n in e}):
        vals = [v for n, v in e.items() if n.startswith(grp + "_")]
        assert len(vals) == 8 and any(vals) and not all(vals), (grp, vals)


def test_fixture_no_half_paired_holes_of_col_fw_and_col_bw():
    """a stated reference behaviour: under --no-half-paired the mate-pair region counts work at region granularity, and in col-fw / col-bw the two mates'
    ranges are not each other's negation -- fragments INSIDE the bounds go unpaired, and one beyond the upper bound is paired.  opp-in / opp-out have neither."""
    hole = {m: any(has_hole(v) for v in series_of(("pair_edges_" + m, "pe_nhp"))[0].values()) for m in PAIR_MODES}
    assert hole == {"opp-in": False, "opp-out": False, "col-fw": True, "col-bw": True}, hole
    beyond = []
    for m in ("col-fw", "col-bw"):
        for tag in ("pe_nhp", "pe_n3_nhp"):
            sweep, _ = series_of(("pair_edges_" + m, tag))
            beyond += [(m, tag, st, f) for st in "pm" for f, x in sweep[("hi", st)] if x and f > 420 + SHIFT[m]]
    assert beyond


@pytest.mark.parametrize("base", ["pair_heap_tandem", "pair_heap_ties"])
def test_fixture_fills_the_pair_heap_and_evicts(oracle_lib, base):
    """by the oracle's counters (it equals the reference on these runs, above): the heap of readpair_get_vector_hits reaches num_tmp_outputs for at least three quarters
    of the pairs, and window pairs are evicted from it -- with distinct keys (3 % divergence between the repeat's copies) and with ties (none)"""
    g, _ = golden(base)
    full, evictions = oracle_run(base, None)[2]
    print(base, "pairs", len(g["m1"]), "heap filled for", full, "evictions", evictions)
    assert 4 * full >= 3 * len(g["m1"]), (full, len(g["m1"]))
    assert evictions > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
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


def product_run(gm, base, tag, max_batch_reads=4096):
    """the product on one run: header + SAM, the call's statistics"""
    g, _ = golden(base, tag)
    cs = "_cs_" in base
    p = gm.default_params_cs() if cs else gm.default_params()
    if cs: p.sam_unaligned = 1
    for k, v in OPTS[tag][2].items(): setattr(p, k, v)
    opts = gm.PairOpts.default(g["mode"], g["ins"][0], g["ins"][1])
    for k, v in OPTS[tag][1].items(): setattr(opts, k, v)
    ix = gm.Index(g["contigs"], names=g["contig_names"], params=p); s = gm.Session(ix, params=p, max_batch_reads=max_batch_reads)
    try:
        body = (s.map_pairs_cs if cs else s.map_pairs)(g["m1"], g["m2"], g["names1"], g["names2"], opts=opts)
        st = s.stats
    finally:
        s.close(); ix.close()
    return oa.sam_header(g["contigs"], g["contig_names"]) + body, st


class env_set:
    """environment variables for the length of a block, put back as they were"""
    def __init__(self, **kv): self.kv = kv
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)
    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def check_run(gm, run, exact=False, **kw):
    """One run of the product: its SAM == the reference's, no (pair, strand) item left unfiltered, and the stage counts against the oracle's last_pair_counts().  The
    window count equals it on every path.  The collapsed-anchor count equals it where no prune rules run (-n 3, the exact mate-pair path); the default paths drop
    inert survivors before the anchor kernel ("only stats.anchors changes"), so there the run is repeated with the prune rules off (GM_NO_PRUNE=1, which
    only the tuning library reads: not under GM_LIB_PATH) and must then give the same bytes and both counts."""
    _, want = golden(*run)
    want_counts = oracle_run(*run)[1]
    got, st = product_run(gm, *run, **kw)
    assert got == want, (_first_diff(got, want), st)
    assert st["mp_unfiltered"] == 0, st
    assert st["windows"] == want_counts[1], (st["anchors"], st["windows"], want_counts)
    if exact or (run[1] or "").startswith("pe_n3"):
        assert st["anchors"] == want_counts[0], (st["anchors"], st["windows"], want_counts)
    elif not os.environ.get("GM_LIB_PATH"):
        with env_set(GM_NO_PRUNE="1"):
            got, st = product_run(gm, *run, **kw)
        assert got == want, (_first_diff(got, want), st)
        assert st["mp_unfiltered"] == 0 and (st["anchors"], st["windows"]) == want_counts, (st["anchors"], st["windows"], want_counts)


@pytest.mark.gpu
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_pair_edges_match_reference_golden(gm, oracle_lib, run):
    """map_pairs / map_pairs_cs in one sub-batch == the reference, nothing left unfiltered, and the stage counts (collapsed anchors, windows) equal the oracle's"""
    check_run(gm, run)


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", ["1", "0"])
@pytest.mark.parametrize("run", [r for r in LS_RUNS if r[1] in (None, "pe_nhp")], ids=run_id)
def test_pair_edges_in_sub_batches_of_64_under_both_pipeline_orders(gm, oracle_lib, run, overlap):
    """the bounds hold in every sub-batch and on both buffer pairs: max_batch_reads=64, the overlapped pipeline (GM_OVERLAP=1) and the strict stage order (0)"""
    with env_set(GM_OVERLAP=overlap):
        check_run(gm, run, max_batch_reads=64)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", PAIR_MODES)
def test_pair_edges_on_the_exact_mate_pair_path(gm, oracle_lib, mode):
    """GM_MP_EXACT=1 (tuning library): --no-half-paired through the generic lookup kernel's mate-pair mode 5 instead of k_mp_filter -- the same bytes, the same counts"""
    with env_set(GM_MP_EXACT="1"):
        check_run(gm, ("pair_edges_" + mode, "pe_nhp"), exact=True)


@pytest.mark.gpu
def test_one_session_follows_the_mates_lengths(gm, oracle_lib):
    """one session maps pair_edges_col-fw (mates of 40 and 60), the same mates with the files swapped (60 and 40; against the oracle), then the first again: the
    ranges (col-fw adds the SECOND mate's length) and the buffers follow the lengths of the call in hand"""
    g, want = golden("pair_edges_col-fw")
    want_swapped = oracle_run("pair_edges_col-fw", None, swapped=True)
    hdr = oa.sam_header(g["contigs"], g["contig_names"])
    opts = gm.PairOpts.default(g["mode"], g["ins"][0], g["ins"][1])
    ix = gm.Index(g["contigs"], names=g["contig_names"]); s = gm.Session(ix, max_batch_reads=4096)
    try:
        a = hdr + s.map_pairs(g["m1"], g["m2"], g["names1"], g["names2"], opts=opts)
        b = hdr + s.map_pairs(g["m2"], g["m1"], g["names2"], g["names1"], opts=opts); st_b = s.stats
        c = hdr + s.map_pairs(g["m1"], g["m2"], g["names1"], g["names2"], opts=opts)
    finally:
        s.close(); ix.close()
    assert a == want, _first_diff(a, want)
    assert b == want_swapped[0], _first_diff(b, want_swapped[0])
    assert st_b["windows"] == want_swapped[1][1], (st_b["windows"], want_swapped[1])     # (anchors: the default path prunes, see check_run)
    assert paired_names(b) != paired_names(a)                                       # (the swap moves the bounds by 20 bases: other fragments pair)
    assert c == want, _first_diff(c, want)


@pytest.mark.gpu
def test_release_build_reproduces_the_pair_edge_goldens():
    """`make release` (no tuning knobs compiled in; the build bench.py measures): the golden tests of this file in a child interpreter with GM_LIB_PATH on
    libgmapper_hip_release.so"""
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    env = dict(os.environ, GM_LIB_PATH=rel); env.pop("GM_MP_EXACT", None)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "test_pair_edges_match_reference_golden", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, cwd=oa.ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) == len(RUNS), p.stdout[-500:]
