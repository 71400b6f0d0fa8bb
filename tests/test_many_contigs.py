"""Many and short contigs (tools/make_golden.py --contigs-only): one i.i.d. sequence S cut into consecutive contigs, so that global coordinates stay those of the
uncut S and only the contig table differs.

  split_60bp          300 contigs: 1, 5, 13, 14, 19, 59, 60, 61, 83, 84, 85 bases (seed spans 14 to 19, reads of 60, windows of 84) next to contigs of 300 to 2 000;
                      600 reads on a contig's first and last base, filling a 60-base contig, inside a contig shorter than the window, across one border with
                      1 / 13 / 20 / 30 bases on the far side, across a whole short contig.  Default, --local, -n 1, --local -U (the reference refuses -U without
                      --local), and default with --extra-sam-fields
  split_64, split_65  the same S in exactly 64 and 65 contigs: the two sides of the anchor kernel's lane-gather contig search
  split_cs_50col      the same construction in colour space (50 colours, windows of 70), default and --local
  split_pairs_2x60    opp-in pairs under -I 100,300: adj_* mates on two adjacent contigs, one_* on either side of a 1-base contig, in_* inside one contig of 130 to 250
                      bases, ctl_* inside a long one; default and --no-half-paired
  contigs_65536       65 536 contigs (fillers of 12 to 24 bases); 400 reads and 100 pairs from targets of 80 to 200 bases at indices 0, 63, 64, 65, 255, 256, 32 767,
                      32 768, 65 534, 65 535 and at 25 pairs (b, b + 32 768), every target its own sequence: a contig number cut to fewer bits shows in RNAME.
                      Only the SAM bodies are stored.

Without a GPU: the oracle gives every golden byte for byte, the windows driver carries the reference's records, the fixtures' conditions hold.  With one: the product
gives the same bytes on every path the contig number takes."""
import ctypes as C
import gzip, importlib.util, os, re, subprocess, sys
import numpy as np
import pytest
from tests import oracle_api as oa
from tests import test_read_windows as trw

GOLD = os.path.join(oa.ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(oa.ROOT, "tools", "make_golden.py"))
mg = importlib.util.module_from_spec(_spec); _spec.loader.exec_module(mg)           # the generator's own conditions (it reads the reference only in contigs_cases)

UNGAPPED = dict(local_alignment=1, ungapped=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255, hash_filter_calls=0)
# (fixture, tag) -> (colour space, oracle options, gm_params_t fields)
UNPAIRED = {
    ("split_60bp", None): (False, None, {}),
    ("split_60bp", "local"): (False, "local=1", dict(local_alignment=1)),
    ("split_60bp", "n1"): (False, "cmw-mode=1", dict(match_mode=1)),
    ("split_60bp", "ungapped"): (False, "local=1;ungapped=1", UNGAPPED),
    ("split_64", None): (False, None, {}),
    ("split_65", None): (False, None, {}),
    ("split_cs_50col", None): (True, "colour=1", {}),
    ("split_cs_50col", "local"): (True, "colour=1;local=1", dict(local_alignment=1)),
    ("contigs_65536", None): (False, None, {}),
}
# (fixture, tag) -> (oracle options, gm_pair_opts_t fields)
PAIRED = {("split_pairs_2x60", None): (None, {}), ("split_pairs_2x60", "nhp"): ("half-paired=0", dict(half_paired=0)), ("contigs_65536", "pairs"): (None, {})}
run_id = lambda r: r[0] + ("@" + r[1] if r[1] else "")
BODY_ONLY = "contigs_65536"
# mapped records of the reference per run, as counted when the fixtures were drawn
MAPPED = {"split_60bp": 437, "split_60bp@local": 500, "split_60bp@n1": 437, "split_60bp@ungapped": 553, "split_60bp@extra": 437, "split_64": 147, "split_65": 140,
          "split_cs_50col": 408, "split_cs_50col@local": 493}


_fx = {}
def fixture(name):
    """S, the contig table and the reads of a fixture; contigs: views of S"""
    if name not in _fx:
        z = np.load(os.path.join(GOLD, name + ".npz"))
        d = {k: z[k] for k in z.files}
        lens = d["contig_len"].astype(np.int64); off = np.concatenate([[0], np.cumsum(lens)])
        assert int(off[-1]) == len(d["S"])
        d.update(lens=lens, off=off, contigs=np.split(np.ascontiguousarray(d["S"], dtype=np.uint8), off[1:-1]))
        if "mates1" in d:
            d["names1"] = [bytes(n) + b"/1" for n in d["names"]]; d["names2"] = [bytes(n) + b"/2" for n in d["names"]]
        _fx[name] = d
    return _fx[name]


def golden(name, tag=None):
    with gzip.open(os.path.join(GOLD, name + ("@" + tag if tag else "") + ".sam.gz"), "rb") as f: return f.read()


def want_of(name, tag=None):
    """(header the product and the oracle print, the reference's records behind it): contigs_65536 stores the records only"""
    F = fixture(name); hdr = oa.sam_header(F["contigs"]); sam = golden(name, tag)
    if name == BODY_ONLY: assert not sam.startswith(b"@"); return hdr, sam
    assert sam.startswith(hdr); return hdr, sam[len(hdr):]


def _first_diff(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y: return i, x[:300], y[:300]
    return min(len(la), len(lb)), len(la), len(lb)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", sorted(UNPAIRED, key=run_id), ids=run_id)
def test_oracle_equals_the_reference_on_the_unpaired_goldens(oracle_lib, run):
    F = fixture(run[0]); _, want = want_of(*run)
    o = oa.Session(F["contigs"], opts=UNPAIRED[run][1])
    got = o.map_sam(F["reads"], nthreads=4); o.close()
    assert got == want, _first_diff(got, want)


@pytest.mark.parametrize("run", sorted(PAIRED, key=run_id), ids=run_id)
def test_oracle_equals_the_reference_on_the_paired_goldens(oracle_lib, run):
    F = fixture(run[0]); _, want = want_of(*run)
    o = oa.Session(F["contigs"], opts=PAIRED[run][0])
    o.set_pairing(str(F["mode"]), *(int(x) for x in F["ins"]))
    got = o.map_pairs_sam(F["mates1"], F["mates2"], F["names1"], F["names2"], nthreads=4); o.close()
    assert got == want, _first_diff(got, want)


def test_extra_fields_golden_is_the_default_golden_plus_its_tags():
    """the oracle does not print ZM / ZR / ZV / ZH / ZE: split_60bp@extra without them is split_60bp, which the oracle gives"""
    cut = re.sub(rb"\tZ[MRVHE]:[^\t\n]*", b"", golden("split_60bp", "extra"))
    assert cut == golden("split_60bp") and golden("split_60bp", "extra").count(b"\tZM:i:") == MAPPED["split_60bp@extra"]


def test_fixture_layouts_hold_every_class():
    for name, L in (("split_60bp", 60), ("split_cs_50col", 50)):
        F = fixture(name); lens = F["lens"]; W = mg.ct_window(L)
        assert W == {60: 84, 50: 70}[L] and len(lens) == 300 and 50_000 < len(F["S"]) < 70_000
        for c in mg.ct_classes(L): assert int((lens == c).sum()) >= 5, (name, c)
        assert int(((lens >= 300) & (lens <= 2000)).sum()) >= 80 and int(lens.max()) <= 2000
        assert sum(1 for i in range(len(lens) - 1) if (lens[i] >= 300) != (lens[i + 1] >= 300)) >= 100      # long contigs next to short ones
        kinds = [mg.CT_KINDS[k] for k in F["kind"]]
        assert len(kinds) == 600 == len(F["reads"])
        for k, n in (("first", 40), ("last", 40), ("fill", 10), ("inside", 10), ("border", 120), ("over", 60), ("random", 50)): assert kinds.count(k) >= n, (name, k, kinds.count(k))
        far = {k: 0 for k in mg.CT_FAR}
        for i, k in enumerate(kinds):
            a, b = mg.ct_spans(lens, int(F["pos"][i]), L)
            if k == "fill": assert a == b and lens[a] == L and F["pos"][i] == F["off"][a]
            if k == "inside": assert a == b and L < lens[a] < W
            if k == "first": assert F["pos"][i] == F["off"][a]
            if k == "last": assert F["pos"][i] + L == F["off"][b + 1]
            if k == "over": assert b - a >= 2
            if k == "border":
                assert b > a
                left = int(F["off"][a + 1] - F["pos"][i]); right = L - int(F["off"][b] - F["pos"][i])
                for x in (left, right):
                    if x in far: far[x] += 1
        assert min(far.values()) >= 20, far
    for n in (64, 65): assert len(fixture("split_%d" % n)["lens"]) == n and np.array_equal(fixture("split_%d" % n)["S"], fixture("split_60bp")["S"])
    assert np.array_equal(fixture("split_cs_50col")["S"], fixture("split_60bp")["S"][:len(fixture("split_cs_50col")["S"])])


@pytest.mark.parametrize("name,L", [("split_60bp", 60), ("split_cs_50col", 50)])
def test_fixture_conditions_of_the_split_reads(name, L):
    """from the reference's SAM alone: records on a contig shorter than the window (their windows are clipped to the contig), border-spanning reads mapped and left
    unmapped under default options, records on a contig shorter than the read under --local.  Counts of the committed draw in the comments of MAPPED's users."""
    F = fixture(name)
    c = mg.ct_split_conditions(F["lens"], L, F["kind"], F["pos"], golden(name), golden(name, "local"))
    print(name, c)
    assert c["clipped"] >= 40, c
    if name == "split_60bp":
        assert c == dict(clipped=81, spanning_mapped=90, spanning_unmapped=148, short_local=26), c
        assert c["spanning_mapped"] >= 20 and c["spanning_unmapped"] >= 10 and c["short_local"] >= 10
    else: assert c == dict(clipped=76, spanning_mapped=68, spanning_unmapped=167, short_local=21), c
    for key, n in MAPPED.items():
        if key.split("@")[0] == name: assert len(mg.ct_records(golden(*key.split("@")))) == n, key


@pytest.mark.parametrize("n", [64, 65])
def test_fixture_conditions_of_the_two_sides_of_the_lane_gather(n):
    """records on contigs 34 and up (the sixth step of the gather decides) and on the last contig"""
    recs = mg.ct_records(golden("split_%d" % n))
    hi = sum(1 for r in recs if r[2] >= 33); last = sum(1 for r in recs if r[2] == n - 1)
    assert (len(recs), hi, last) == {64: (147, 50, 6), 65: (140, 73, 7)}[n] and hi >= 40 and last >= 1


def test_fixture_conditions_of_the_split_pairs():
    F = fixture("split_pairs_2x60"); lens, off = F["lens"], F["off"]
    proper = mg._paired_names(golden("split_pairs_2x60"))
    kinds = {}
    for nm, p, f in zip(F["names"], F["pos"], F["frag"]):
        nm = bytes(nm); k = nm.split(b"_")[0].decode(); kinds.setdefault(k, []).append(nm in proper)
        a1, b1 = mg.ct_spans(lens, int(p), 60); a2, b2 = mg.ct_spans(lens, int(p + f) - 60, 60)
        assert a1 == b1 and a2 == b2 and F["ins"][0] + 25 <= f <= F["ins"][1] - 40        # each mate on one contig, the global distance well inside -I
        if k == "adj": assert a2 == a1 + 1
        if k == "one": assert a2 == a1 + 2 and lens[a1 + 1] == 1
        if k in ("in", "ctl"): assert a2 == a1 and ((lens[a1] <= 250) == (k == "in"))
    counts = {k: (len(v), sum(v)) for k, v in kinds.items()}
    assert counts == {"adj": (90, 0), "one": (46, 0), "in": (46, 46), "ctl": (60, 60)}, counts      # the reference pairs nothing across a border, everything else
    assert counts["adj"][0] - counts["adj"][1] >= 30
    assert not mg._paired_names(golden("split_pairs_2x60", "nhp")) - proper


def test_fixture_conditions_of_the_65536_contigs():
    F = fixture("contigs_65536"); lens = F["lens"]
    assert len(lens) == 65536 and 1_100_000 < len(F["S"]) < 1_300_000 and len(F["reads"]) == 400 and len(F["mates1"]) == 100
    targets = sorted(set(int(x) for x in F["target"]) | set(int(x) for x in F["pair_target"]))
    assert set(mg.CT_NAMED) <= set(targets) and len(targets) == 60
    fill = np.ones(65536, dtype=bool); fill[targets] = False
    assert lens[fill].min() >= 12 and lens[fill].max() <= 24 and lens[targets].min() >= 80 and lens[targets].max() <= 200
    seqs = {c: F["contigs"][c].tobytes() for c in targets}
    for c in targets:
        if c in mg.CT_NAMED: continue
        for other in (c & 0x7FFF, c ^ 0x8000):
            assert other in seqs and (other == c or seqs[other][:60] != seqs[c][:60])
    per, high = mg.ct_65536_conditions(golden("contigs_65536"), golden("contigs_65536", "pairs"))
    print(per, high)
    assert per == {0: 18, 63: 10, 64: 16, 65: 14, 255: 18, 256: 12, 32767: 20, 32768: 16, 65534: 14, 65535: 14} and high == 282
    assert min(per.values()) >= 5 and high >= 150
    # every record names the contig its read was cut from
    by_read = {int(n[1:]): cn for n, _, cn, _ in mg.ct_records(golden("contigs_65536"))}
    assert len(by_read) >= 390 and all(cn == int(F["target"][r]) for r, cn in by_read.items())


def test_every_new_fixture_is_no_larger_than_the_largest_before_it():
    for f in os.listdir(GOLD):
        if f.startswith(("split_", "contigs_65536")): assert os.path.getsize(os.path.join(GOLD, f)) <= 734_000, f


# ---- the windows driver ----------------------------------------------------------------------------------------------------------------------------------------
driver = trw.driver                                                      # (the fixture: tests/read_windows_oracle.cpp, compiled once for this module)
_drv = {}


def driver_rows(L, name, mode=2, colour=False):
    """(rows, off) of the driver on a fixture's reads, computed once"""
    if name not in _drv:
        F = fixture(name); cs = F["contigs"]; reads = np.ascontiguousarray(F["reads"], dtype=np.uint8)
        u8p = C.POINTER(C.c_uint8); S = F["S"]; base = S.ctypes.data
        ptrs = (u8p * len(cs))(*[C.cast(base + int(o), u8p) for o in F["off"][:-1]])
        h = L.rwo_create(len(cs), ptrs, (C.c_uint64 * len(cs))(*[int(x) for x in F["lens"]]), int(colour), mode)
        cap = 64 * len(reads); rows = np.zeros((cap, 12), dtype=np.int64)
        w = L.rwo_windows(h, reads.shape[0], reads.shape[1], reads.ctypes.data_as(u8p), trw.THREADS, rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
        L.rwo_destroy(h)
        assert 0 < w <= cap
        _drv[name] = (rows[:w].copy(), trw.offsets(rows[:w], len(reads)))
    return _drv[name]


def test_driver_windows_carry_the_records_of_the_extra_fields_golden(driver):
    """ZM and ZR of every mapped record of split_60bp@extra on a driver window of its read and strand that covers the alignment; the records on a contig shorter than
    the window have clipped windows only (w_len = the contig's length)"""
    F = fixture("split_60bp"); rows, off = driver_rows(driver, "split_60bp")
    assert trw.in_list_order(rows)
    recs = trw.records("split_60bp@extra")
    assert len(recs) == MAPPED["split_60bp@extra"]
    cands = trw.candidates(rows, off, recs)
    clipped = 0
    for r, c in zip(recs, cands):
        short = F["lens"][r[2]] < 84
        assert ((rows[c, 4] < 84) == short).all() and (not short or (rows[c, 4] == F["lens"][r[2]]).all())
        clipped += bool(short)
    assert clipped == 81 and clipped >= 40
    assert int((rows[:, 4] < 84).sum()) == 107                          # (clipped windows in all, mapped or not)


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


from tests.test_pair_edges import env_set                               # environment variables for the length of a block


def params_of(gm, colour, fields):
    p = gm.default_params_cs() if colour else gm.default_params()
    for k, v in fields.items(): setattr(p, k, v)
    return p


_open = {}
def opened(gm, name, colour=False, fields=None):
    """(index, session, params) of a fixture, kept open for the module"""
    key = (name, colour, tuple(sorted((fields or {}).items())))
    if key not in _open:
        p = params_of(gm, colour, fields or {})
        ix = gm.Index(fixture(name)["contigs"], params=p)
        _open[key] = (ix, gm.Session(ix, params=p, max_batch_reads=4096), p)
    return _open[key]


@pytest.fixture(scope="module", autouse=True)
def close_the_sessions_of_this_module():
    yield
    for ix, s, _ in _open.values(): s.close(); ix.close()
    _open.clear()


def map_unpaired(gm, run, index=None, fields=None):
    """header + records of one unpaired run on a fresh session (index: one made another way than Index(contigs))"""
    F = fixture(run[0]); colour, _, flds = UNPAIRED.get(run, (False, None, {}))
    p = params_of(gm, colour, dict(flds, **(fields or {})))
    ix = index if index is not None else gm.Index(F["contigs"], params=p)
    s = gm.Session(ix, params=p, max_batch_reads=4096)
    try:
        body = (s.map_reads_cs if colour else s.map_reads)(F["reads"]); hdr = ix.sam_header(); st = s.stats
    finally:
        s.close()
        if index is None: ix.close()
    return hdr, body, st


def map_paired(gm, run, index=None):
    F = fixture(run[0]); p = gm.default_params()
    opts = gm.PairOpts.default(str(F["mode"]), int(F["ins"][0]), int(F["ins"][1]))
    for k, v in PAIRED[run][1].items(): setattr(opts, k, v)
    ix = index if index is not None else gm.Index(F["contigs"], params=p)
    s = gm.Session(ix, params=p, max_batch_reads=4096)
    try:
        body = s.map_pairs(F["mates1"], F["mates2"], F["names1"], F["names2"], opts=opts); hdr = ix.sam_header(); st = s.stats
    finally:
        s.close()
        if index is None: ix.close()
    return hdr, body, st


@pytest.mark.gpu
@pytest.mark.parametrize("run", sorted(UNPAIRED, key=run_id) + [("split_60bp", "extra")], ids=run_id)
def test_unpaired_sam_matches_reference_golden(gm, run):
    """map_reads / map_reads_cs and the index's own header == the reference, byte for byte (contigs_65536: the header is oa.sam_header's 65 536 @SQ lines)"""
    hdr, want = want_of(*run)
    got_hdr, got, st = map_unpaired(gm, run, fields=dict(extra_sam_fields=1) if run[1] == "extra" else None)
    assert got_hdr == hdr, _first_diff(got_hdr, hdr)
    assert got == want, (_first_diff(got, want), st)


@pytest.mark.gpu
@pytest.mark.parametrize("run", sorted(PAIRED, key=run_id), ids=run_id)
def test_paired_sam_matches_reference_golden(gm, run):
    hdr, want = want_of(*run)
    got_hdr, got, st = map_paired(gm, run)
    assert got_hdr == hdr and got == want, (_first_diff(got, want), st)
    assert st["mp_unfiltered"] == 0, st


VARIANTS = [{"GM_SCAP": "256", "GM_SCAP2": "64"},                        # the heavy tier: the contig search in global memory, the exact path
            {"GM_NO_PRUNE": "1"}, {"GM_SLAB_BITS": "18", "GM_K1_V5": "1"}, {"GM_NO_BUCKETS": "1"},
            {"GM_NO_BUCKETS": "1", "GM_K1_V5": "1"}]                     # (split_60bp is one slab of 2^18 bases and keeps its buckets: only this entry runs k_lookup_v5 on it)
# what gm_last_lookup_kernel() names after the unpaired run of each entry, in their order (recorded before the choice moved into k1_plan, gm_lookup_plan.h)
VARIANT_KERNELS = {"split_60bp": ["k_lookup_bkt", "k_lookup_bkt", "k_lookup_bkt", "k_lookup_v3", "k_lookup_v5"],
                   "contigs_65536": ["k_lookup_bkt", "k_lookup_bkt", "k_lookup_v5", "k_lookup_v3", "k_lookup_v5"]}


@pytest.mark.gpu
@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
@pytest.mark.parametrize("name", ["split_60bp", "contigs_65536"])
def test_kernel_variants_match_reference_golden(gm, name, env):
    """five entries of tests/test_gpu_parity.py's KERNEL_VARIANTS (the tuning library reads them) on the two fixtures"""
    from tests.test_gpu_parity import KERNEL_VARIANTS
    assert env in KERNEL_VARIANTS
    hdr, want = want_of(name)
    with env_set(**env):
        got_hdr, got, st = map_unpaired(gm, (name, None))
        kern = gm.lib().gm_last_lookup_kernel().decode()
    print("lookup kernel: %s" % kern)
    assert got_hdr == hdr and got == want, (_first_diff(got, want), st)
    if "GM_SCAP" in env: assert st["exact_order_reads"] >= 300, st          # (most read-strands leave the small LDS tier and take the exact path: 441 and 378; none by default)
    assert kern == VARIANT_KERNELS[name][VARIANTS.index(env)], kern
    if name == "contigs_65536":
        with env_set(**env):
            _, got, st = map_paired(gm, (name, "pairs"))
        assert got == want_of(name, "pairs")[1], (_first_diff(got, want_of(name, "pairs")[1]), st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["split_60bp", "split_65", "contigs_65536"])
def test_read_windows_equal_the_driver(gm, driver, name):
    """row by row in list order, equal (read, st, cn, g_off) groups as multisets: cn, g_off, w_len and the anchor box of every window, the clipped ones included"""
    want, want_off = driver_rows(driver, name)
    ix, s, _ = opened(gm, name); reads = fixture(name)["reads"]
    wins, off = s.read_windows(reads)
    rows = trw.as_rows(wins)
    assert np.array_equal(off, trw.offsets(rows, len(reads))) and trw.in_list_order(rows) and (rows[:, 11] == 0).all()
    assert np.array_equal(off, want_off), np.nonzero(off != want_off)[0][:10]
    a, b = trw.canon(rows), trw.canon(want)
    assert np.array_equal(a, b), (a[(a != b).any(axis=1)][:5], b[(a != b).any(axis=1)][:5])
    if name == "split_60bp": assert int((rows[:, 4] < 84).sum()) == 107
    if name == "contigs_65536": assert int((rows[:, 2] >= 32768).sum()) >= 150 and int(rows[:, 2].max()) == 65535


_u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))


def oracle_scores(rows, contigs, reads, colour, gapless, p):
    """the oracle's sw_vector / sw_gapless on every window as pass 1 takes it (oracle/gm_oracle.hpp read_pass1): letter space, the forward contig against the read or its
    reverse complement; colour space, the turned window on the strand's colour contig against the read as given"""
    O = oa.load()
    O.gmo_sw_gapless.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_int, C.c_int]
    O.gmo_sw_gapless.restype = C.c_int
    used = sorted(set(int(c) for c in rows[:, 2]))
    fw = {c: np.ascontiguousarray(contigs[c]) for c in used}; rc = {c: trw.CMPL[fw[c][::-1]] for c in used}
    ls = {c: (trw.pack(fw[c]), trw.pack(rc[c])) for c in used}
    cs = {c: (trw.pack(trw.colours(fw[c])), trw.pack(trw.colours(rc[c]))) for c in used} if colour else None
    body = reads[:, 1:] if colour else reads; L = body.shape[1]
    rw = [trw.pack(r) for r in body]; rr = None if colour else [trw.pack(trw.CMPL[r[::-1]]) for r in body]
    out = np.zeros(len(rows), dtype=np.int32)
    for i, r in enumerate(rows):
        rd, st, cn, g_off, wl = (int(x) for x in r[:5]); clen = len(fw[cn])
        if colour: out[i] = O.gmo_sw_vector_cs(_u32(cs[cn][st]), g_off if st == 0 else clen - g_off - wl, wl, _u32(rw[rd]), L, _u32(ls[cn][st]), int(reads[rd, 0]))
        elif gapless: out[i] = O.gmo_sw_gapless(_u32(ls[cn][0]), clen, _u32(rr[rd] if st else rw[rd]), L, g_off + int(r[7]), int(r[8]), None, -1, 0, p.match_score, p.mismatch_score)
        else: out[i] = O.gmo_sw_vector(_u32(ls[cn][0]), g_off, wl, _u32(rr[rd] if st else rw[rd]), L)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,colour,gapless", [("split_60bp", False, False), ("split_60bp", False, True), ("split_cs_50col", True, False)],
                         ids=["split_60bp", "split_60bp-U", "split_cs_50col"])
def test_score_windows_equal_the_oracle_at_the_same_addresses(gm, oracle_lib, name, colour, gapless):
    """Session.score_windows on the session's own windows (default sessions: the ones held to the driver above) == the oracle's sw_vector / sw_gapless"""
    F = fixture(name); reads = np.ascontiguousarray(F["reads"], dtype=np.uint8)
    ix, s, p = opened(gm, name, colour, UNGAPPED if gapless else None)
    codes, ib = (np.ascontiguousarray(reads[:, 1:]), np.ascontiguousarray(reads[:, 0])) if colour else (reads, None)
    wins, off = s.read_windows(codes, initbp=ib)
    rows = trw.as_rows(wins)
    assert len(rows) >= 400 and int((rows[:, 1] == 1).sum()) >= 100 and int((rows[:, 4] < (70 if colour else 84)).sum()) >= 40
    scores, _ = s.score_windows(codes, wins, off, initbp=ib)
    want = oracle_scores(rows, F["contigs"], reads, colour, gapless, p)
    bad = np.nonzero(scores != want)[0]
    assert len(bad) == 0, (len(bad), rows[bad[:5]], scores[bad[:5]], want[bad[:5]])
    assert int(want.max()) == 10 * codes.shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [True, False], ids=["cache", "no-cache"])
def test_read_hits_equal_the_three_calls(gm, cache):
    """Session.read_hits on split_60bp == read_windows -> score_windows -> select_pass1(slots=), with the f1 call cache and without it"""
    from tests import test_pass1_seam as tps
    reads = np.ascontiguousarray(fixture("split_60bp")["reads"], dtype=np.uint8)
    ix, s, p = opened(gm, "split_60bp", False, None if cache else dict(hash_filter_calls=0))
    want = tps.chain_of(s, p, reads, cache=cache)
    hits, hit_off, wins, off, scores = s.read_hits(reads, want_windows=True)
    tps.same_up_to_equal_windows((wins, off, scores, hits, hit_off), want)
    assert len(set(hits["read"].tolist())) >= 300                       # (the reference maps 437 records)
    if not cache: assert s.stats["vec_bypassed"] == 0


def write_fasta(path, contigs, width=70):
    T = np.frombuffer(b"ACGTUMRWSYKVHDBN", dtype=np.uint8); out = bytearray()
    for i, c in enumerate(contigs):
        t = T[c].tobytes(); out += b">contig%d\n" % (i + 1)
        for k in range(0, len(t), width): out += t[k:k + width] + b"\n"
    with open(path, "wb") as f: f.write(bytes(out))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["split_60bp", "contigs_65536"])
def test_index_from_fasta_has_the_contig_table_and_maps_the_same_bytes(gm, name, tmp_path):
    """a FASTA of every contig (contigs_65536: 65 536 records, most shorter than a text line): gm_index_contig of every contig, the header and the mapping"""
    F = fixture(name); path = str(tmp_path / "g.fa")
    write_fasta(path, F["contigs"])
    ix = gm.Index.from_fasta(path)
    try:
        table = ix.contigs()
        assert table == [(b"contig%d" % (i + 1), int(n)) for i, n in enumerate(F["lens"])]
        hdr, want = want_of(name)
        got_hdr, got, st = map_unpaired(gm, (name, None), index=ix)
        assert got_hdr == hdr and got == want, (_first_diff(got, want), st)
        if name == "contigs_65536":
            _, got, st = map_paired(gm, (name, "pairs"), index=ix)
            assert got == want_of(name, "pairs")[1], st
    finally: ix.close()


@pytest.mark.gpu
def test_saved_and_loaded_index_of_65536_contigs_maps_the_same_bytes(gm, tmp_path):
    """save -> load (short seeds keep the files small: lists of 4^9 k-mers): the loaded index has the table and maps the built one's bytes, on every target"""
    F = fixture("contigs_65536"); seeds = ["11110111101", "1101101011011"]
    ix = gm.Index(F["contigs"], seeds=seeds); s = gm.Session(ix, max_batch_reads=4096)
    built = s.map_reads(F["reads"]); s.close()
    ix.save(str(tmp_path / "idx")); table = ix.contigs(); ix.close()
    ld = gm.Index.load(str(tmp_path / "idx")); s = gm.Session(ld, max_batch_reads=4096)
    try:
        loaded = s.map_reads(F["reads"])
        assert ld.contigs() == table and len(table) == 65536
    finally: s.close(); ld.close()
    assert loaded == built, _first_diff(loaded, built)
    by_read = {int(n[1:]): cn for n, _, cn, _ in mg.ct_records(built)}
    assert len(by_read) >= 300 and all(cn == int(F["target"][r]) for r, cn in by_read.items())


@pytest.mark.gpu
def test_65537_contigs_are_refused_by_every_index_entry_and_a_good_build_follows(gm, tmp_path):
    """GM_E_RANGE with the count and the limit from gm_index_build, gm_index_build_fasta and gm_index_load (a .genome file whose header says 65 537 contigs: the entry
    refuses on the count, before it reads a table); then split_64 builds and maps on the same device"""
    F = fixture("contigs_65536")
    contigs = F["contigs"] + [np.array([0, 1, 2, 3] * 4, dtype=np.uint8)]
    assert len(contigs) == 65537
    path = str(tmp_path / "g.fa"); write_fasta(path, contigs)
    with gzip.open(str(tmp_path / "idx.genome"), "wb") as f: f.write(np.array([1, 0, 65537], dtype=np.uint32).tobytes())
    for call in (lambda: gm.Index(contigs), lambda: gm.Index.from_fasta(path), lambda: gm.Index.load(str(tmp_path / "idx"))):
        with pytest.raises(gm.GmError) as e: call()
        assert "(%d)" % trw.GM_E_RANGE in str(e.value) and "65537 contigs" in str(e.value) and "65536" in str(e.value), str(e.value)
    hdr, want = want_of("split_64")
    got_hdr, got, st = map_unpaired(gm, ("split_64", None))
    assert got_hdr == hdr and got == want, (_first_diff(got, want), st)


@pytest.mark.gpu
def test_release_build_reproduces_the_many_contig_goldens():
    """`make release` (no tuning knobs compiled in; the build bench.py measures): the golden tests of this file in a child interpreter with GM_LIB_PATH on
    libgmapper_hip_release.so"""
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    env = dict(os.environ, GM_LIB_PATH=rel)
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "sam_matches_reference_golden", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, cwd=oa.ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) == len(UNPAIRED) + 1 + len(PAIRED), p.stdout[-500:]
