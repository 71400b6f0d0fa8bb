"""Window and anchor-band geometry off the defaults: -a (anchor width; -1: no anchor band at all, the threshold band in every full alignment), -w (window length, as a
percentage of the read and as an absolute count, shorter than the read included), -l (window overlap), -r, -h, -v, -z -- the option sets of tests/oracle_api.py
GEOMETRY_CASES through the reference on committed inputs (tools/make_golden.py --geometry-only), and the reference's own sw_full_ls / sw_full_cs at the anchor widths
-1, 0, 1, 9 and 99 (--anchor-kat-only: tests/golden/sw_kat_anchors.txt.gz, sw_kat_cs_anchors.txt.gz).

Without a GPU: the oracle gives every golden and every known answer byte for byte, the goldens' distances from the defaults hold, and the oracle with the anchor width
forced to 8 misses every -a golden that is not the default's.  With one: map_reads / map_reads_cs / map_pairs give the goldens' bytes, the batch entries the known
answers, and the seams agree with the drivers and the oracle under the same options."""
import ctypes as C
import gzip, os, re, subprocess, sys
import numpy as np
import pytest
from tests import oracle_api as oa
from tests.test_sw_full_batch import _item, run_ls, run_cs, check_ls, check_cs, LS_FIELDS, CS_FIELDS
from tests.test_sw_score_sets import _oracle_ls, _oracle_cs, _u32

GOLD = os.path.join(oa.ROOT, "tests", "golden")
TAGS = sorted(oa.GEOMETRY_CASES)
GM_E_ARG, GM_E_RANGE = -2, -4


def _first_diff(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y: return i, x[:300], y[:300]
    return min(len(la), len(lb)), len(la), len(lb)


_in = {}
def inputs(base):
    """the committed input of a geometry case"""
    if base not in _in:
        if oa.geometry_kind(base) == "pairs": _in[base] = oa.load_golden_pairs(base)
        else:
            contigs, reads, _ = oa.load_golden(base); _in[base] = dict(contigs=contigs, reads=reads)
    return _in[base]


def oracle_records(tag, more_opts=""):
    """the oracle's records of a case; more_opts: options behind the case's own (a later key overrides an earlier one)"""
    base, _, opts, _ = oa.GEOMETRY_CASES[tag]; n = oa.geometry_reads(tag); kind = oa.geometry_kind(base); g = inputs(base)
    opts = ";".join(x for x in ("colour=1" if kind == "cs" else "", opts, more_opts) if x)
    o = oa.Session(g["contigs"], g.get("contig_names"), opts=opts)
    try:
        if base in oa.GEOMETRY_UNAL: o.set(True, True)
        if kind == "pairs":
            o.set_pairing(g["mode"], *g["ins"])
            return o.map_pairs_sam(g["m1"][:n], g["m2"][:n], g["names1"][:n], g["names2"][:n], nthreads=4)
        return o.map_sam(g["reads"][:n], nthreads=4)
    finally: o.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_oracle_equals_the_reference_on_the_geometry_goldens(oracle_lib, tag):
    got, want = oracle_records(tag), oa.load_geometry_sam(tag)
    assert got == want, _first_diff(got, want)


# records of each golden that are not in its input's default golden, as the generator printed them
DISTANCE = {
    "stress_60bp:a-1": 9, "stress_60bp:a0": 207, "stress_60bp:a1": 96, "stress_60bp:a99": 9, "stress_60bp:w100": 778, "stress_60bp:w300": 11, "stress_60bp:w131abs": 10,
    "stress_60bp:w60abs": 778, "stress_60bp:w61abs": 568, "stress_60bp:w50abs": 1675, "stress_60bp:l20abs": 29, "stress_60bp:l100": 10, "stress_60bp:l10": 30,
    "stress_60bp:r250abs": 25, "stress_60bp:r90": 5, "stress_60bp:h437abs": 6, "stress_60bp:z5": 7, "stress_60bp:local_a-1": 1773, "stress_60bp:w100_a-1": 778,
    "stress_60bp:w100_n1": 791,
    "stress_100bp_unal:a-1": 10, "stress_100bp_unal:a0": 335, "stress_100bp_unal:a1": 167, "stress_100bp_unal:a99": 10, "stress_100bp_unal:w100": 1029,
    "stress_100bp_unal:w300": 10, "stress_100bp_unal:l20abs": 35, "stress_100bp_unal:r90": 154, "stress_100bp_unal:z5": 47, "stress_100bp_unal:local_a-1": 1879,
    "stress_cs_60col_unal:a-1": 0, "stress_cs_60col_unal:a0": 139, "stress_cs_60col_unal:w100": 591, "stress_cs_60col_unal:w300": 5, "stress_cs_60col_unal:v40_h80": 122,
    "stress_cs_60col_unal:local_a-1": 723,
    "stress_pairs_2x100:w100": 830, "stress_pairs_2x100:w250": 20, "stress_pairs_2x100:a-1": 34, "stress_pairs_2x100:a0": 48, "stress_pairs_2x100:w170abs_l30abs": 8,
    "stress_pairs_2x100:w100_nhp": 522, "stress_pairs_2x100:w250_n3": 64, "pair_edges_opp-in:w100": 635, "pair_edges_col-bw:w100": 639,
}
# records of the -a -1 and the -a 99 golden that are not in the -a 0 golden of the same input
DISTANCE_FROM_A0 = {"stress_60bp:a-1": 209, "stress_60bp:a99": 209, "stress_100bp_unal:a-1": 335, "stress_100bp_unal:a99": 335, "stress_cs_60col_unal:a-1": 139,
                    "stress_pairs_2x100:a-1": 50}


def test_every_case_has_its_golden_and_the_table_names_every_case():
    assert sorted(DISTANCE) == TAGS and len(TAGS) == 45
    for tag in TAGS:
        assert os.path.getsize(os.path.join(GOLD, oa.geometry_file(tag))) <= 130_000, tag
    for base, whats in (("stress_60bp", 20), ("stress_100bp_unal", 10), ("stress_cs_60col_unal", 6), ("stress_pairs_2x100", 7)):
        assert sum(t.startswith(base + ":") for t in TAGS) == whats


@pytest.mark.parametrize("tag", TAGS)
def test_golden_differs_from_the_default_golden_of_its_input(tag):
    base = tag.split(":")[0]
    d = oa.sam_distance(oa.load_geometry_sam(tag), oa.geometry_default_records(base, oa.geometry_reads(tag)))
    print(tag, d)
    assert d == DISTANCE[tag]
    assert d >= oa.GEOMETRY_MIN_DISTANCE or (tag in oa.GEOMETRY_SAME_AS_DEFAULT and d == 0)


@pytest.mark.parametrize("tag", sorted(DISTANCE_FROM_A0))
def test_no_anchor_band_and_the_widest_differ_from_width_zero(tag):
    """-a -1 and -a 99 against -a 0 on every input that has them; colour space -a -1, which equals the default there, among them"""
    d = oa.sam_distance(oa.load_geometry_sam(tag), oa.load_geometry_sam(tag.split(":")[0] + ":a0"))
    assert d == DISTANCE_FROM_A0[tag] and d >= oa.GEOMETRY_MIN_DISTANCE
    assert sorted(DISTANCE_FROM_A0) == sorted(t for t in TAGS if t.split(":")[1] in ("a-1", "a99"))


# (-w 100% -a -1 is not among them: a window of the read's length leaves the band nothing to decide, its golden is the bytes of -w 100%)
# ... nor the two colour-space -a -1 cases: on that input the threshold band and the band of width 8 give the same records, and width 0 is what the goldens rule out
WIDTH_8_ALIKE = ("stress_cs_60col_unal:a-1", "stress_cs_60col_unal:local_a-1")
A_TAGS = [t for t in TAGS if "anchor-width" in oa.GEOMETRY_CASES[t][2] and "match-window" not in oa.GEOMETRY_CASES[t][2] and t not in WIDTH_8_ALIKE]


@pytest.mark.parametrize("tag", A_TAGS)
def test_oracle_with_the_anchor_width_forced_to_8_misses_every_a_golden(oracle_lib, tag):
    """what a library that ignored anchor_width would print (colour space -a -1 apart: its golden is the default's, GEOMETRY_SAME_AS_DEFAULT)"""
    got, want = oracle_records(tag, "anchor-width=8"), oa.load_geometry_sam(tag)
    assert got != want and oa.sam_distance(want, got) >= oa.GEOMETRY_MIN_DISTANCE


@pytest.mark.parametrize("tag", WIDTH_8_ALIKE)
def test_oracle_colour_space_at_width_0_misses_the_a_minus_1_goldens(oracle_lib, tag):
    """the two colour-space -a -1 goldens are what width 8 gives too, and well away from width 0 -- which is about what a box narrowed by one (anchor_widen by -1, the
    library's answer before it knew the value) comes to: the goldens tell the threshold band from that"""
    want = oa.load_geometry_sam(tag)
    assert oracle_records(tag, "anchor-width=8") == want
    assert oa.sam_distance(want, oracle_records(tag, "anchor-width=0")) >= oa.GEOMETRY_MIN_DISTANCE


# ---- the known answers at other anchor widths -------------------------------------------------------------------------------------------------------------------
WIDTHS = [-1, 0, 1, 9, 99]
_kat = {}


def ls_width(w):
    """setup tuple, F / G / L items of one width (letter space)"""
    if "ls" not in _kat:
        d = {}
        for nm, setup, recs in oa.load_kat_anchors(False):
            F = [_item(r[9], r[1], r[2], r[10], r[3], tuple(r[4:8]), r[8], want=r[11], db=r[12], qr=r[13]) for r in recs if r[0] == "F"]
            lay = lambda rs: [_item(g, goff, glen, rd, rlen, None if no_anchor else (ax, ay, alen, aw), rv, thresh, sv, want=want, db=db, qr=qr)
                              for (goff, glen, rlen, ax, ay, alen, aw, rv, no_anchor, thresh, sv), g, rd, want, db, qr in rs]
            d[setup[-1]] = dict(name=nm, setup=setup, F=F, G=lay([r[1:] for r in recs if r[0] == "G"]), L=lay([r for r in recs if isinstance(r[0], tuple)]))
        _kat["ls"] = d
    return _kat["ls"][w]


def cs_width(w):
    if "cs" not in _kat:
        d = {}
        for nm, setup, recs in oa.load_kat_anchors(True):
            e = dict(name=nm, setup=setup, S=[], L=[])
            for r in recs:
                (goff, glen, rlen, initbp, ax, ay, alen, aw, rv, thresh), gls, rd, want, db, qr = r[1:7]
                e[r[0]].append(_item(gls, goff, glen, rd, rlen, (ax, ay, alen, aw), rv, thresh, initbp=initbp, want=want, db=db, qr=qr))
            d[setup[-1]] = e
        _kat["cs"] = d
    return _kat["cs"][w]


def box_classes(items):
    """how many items' boxes leave the matrix on each side, are wider than 4, or stand beside a window shorter than the read"""
    c = dict(left=0, right=0, below=0, wide=0, short=0)
    for it in items:
        if it["anchor"] is None: continue
        ax, ay, alen, aw = it["anchor"]
        c["left"] += ax < 0; c["right"] += ax + alen > it["glen"]; c["below"] += ay + alen > it["rlen"]; c["wide"] += aw > 4; c["short"] += it["glen"] < it["rlen"]
    return c


def test_anchor_fixtures_hold_every_width_and_box_shape():
    assert sorted(oa.load_kat_anchors(False)[k][1][-1] for k in range(5)) == sorted(WIDTHS) == sorted(s[1][-1] for s in oa.load_kat_anchors(True))
    for w in WIDTHS:
        s = ls_width(w); c = cs_width(w)
        assert s["setup"][:8] == (1400, 1000, -33, -7, -33, -3, 10, -15) and c["setup"][:10] == (1400, 1000, -33, -7, -33, -3, 10, -24, -20, 0)
        assert len(s["F"]) + len(s["G"]) + len(s["L"]) >= 300 and len(c["S"]) + len(c["L"]) >= 300, (w, len(s["F"]), len(s["G"]), len(s["L"]), len(c["S"]), len(c["L"]))
        assert any(it["anchor"] is None for it in s["L"]) and any(it["anchor"] is not None for it in s["L"])
        for name, items in (("F", s["F"]), ("G", s["G"]), ("L", s["L"]), ("S", c["S"]), ("cs L", c["L"])):
            bc = box_classes(items)
            assert min(bc.values()) >= 3, (w, name, bc)
            assert max(it["anchor"][3] for it in items if it["anchor"] is not None) == 12
        assert sum(it["want"][0] > 0 for it in c["S"]) >= 50 and sum(it["want"][0] > 0 for it in c["L"]) >= 50
    # the widths are told apart: the same cases under every width, and the records differ between -1, 0, 9 and 99 -- but in letter space not between -1 and 99: at a
    # threshold of half the read's score the threshold band and a box widened by 99 both hold every alignment these cases have, and the records are the same there
    # (colour space, whose thresholds go up to 0.6 of the read, does tell them apart)
    for kind in ("G", "L"):
        wants = {w: [(it["goff"], it["glen"], it["rlen"], it["anchor"], it["rv"], tuple(it["want"]), it["db"]) for it in ls_width(w)[kind]] for w in WIDTHS}
        assert set(wants[-1]) != set(wants[0]) and set(wants[0]) != set(wants[9]) and set(wants[-1]) != set(wants[9]) and set(wants[9]) != set(wants[99]), kind
    for kind in ("S", "L"):
        wants = {w: [(it["goff"], it["glen"], it["rlen"], it["anchor"], it["rv"], tuple(it["want"]), it["db"]) for it in cs_width(w)[kind]] for w in WIDTHS}
        assert set(wants[-1]) != set(wants[0]) and set(wants[0]) != set(wants[9]) and set(wants[-1]) != set(wants[9]), kind


@pytest.mark.parametrize("w", WIDTHS)
def test_oracle_letter_space_equals_the_reference_at_the_width(oracle_lib, w):
    s = ls_width(w); sc = oa.score_array(s["setup"][:-1], anchor_width=w)
    for kind, local in (("F", False), ("G", False), ("L", True)):
        for k, it in enumerate(s[kind]):
            got, db, qr = _oracle_ls(oracle_lib, sc, it, local)
            assert got == it["want"] and (db, qr) == (it["db"], it["qr"]), (w, kind, k, got, it["want"], db, it["db"], qr, it["qr"])


@pytest.mark.parametrize("w", WIDTHS)
def test_oracle_colour_space_equals_the_reference_at_the_width(oracle_lib, w):
    s = cs_width(w); sc = oa.score_array(s["setup"][:-1], anchor_width=w)
    for kind, local in (("S", False), ("L", True)):
        for k, it in enumerate(s[kind]):
            got, db, qr = _oracle_cs(oracle_lib, sc, it, local)
            if it["want"][0] == 0:                                   # below the threshold: score 0 and no strings
                assert got[0] == 0 and db == "" and qr == "", (w, kind, k, got)
                continue
            assert got == it["want"] and (db, qr) == (it["db"], it["qr"]), (w, kind, k, got, it["want"], db, it["db"], qr, it["qr"])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
from tests.test_pair_edges import env_set                               # environment variables for the length of a block
from tests import test_read_windows as trw

driver = trw.driver                                                      # (the fixture: tests/read_windows_oracle.cpp, compiled once for this module)


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
    yield gmapper
    for ix in _index.values(): ix.close()
    _index.clear()
    gmapper.sw_full_ls_setup(1400, 1000, -33, -7, -33, -3, 10, -15, True, 8)            # leave the thread's setups at the defaults
    gmapper.sw_full_cs_setup(1400, 1000, -33, -7, -33, -3, 10, -24, -20, True, 8, 0)


_index = {}
def index_of(gm, base, list_cutoff=0):
    """the index of an input, shared by its cases (-z is the index's own)"""
    key = (base, list_cutoff)
    if key not in _index:
        g = inputs(base); p = gm.default_params_cs() if oa.geometry_kind(base) == "cs" else gm.default_params()
        if list_cutoff: p.list_cutoff = list_cutoff
        _index[key] = gm.Index(g["contigs"], names=g.get("contig_names"), params=p)
    return _index[key]


def params_of(gm, tag, **more):
    """(gm_params_t, gm_pair_opts_t fields) of a case"""
    base, _, _, fields = oa.GEOMETRY_CASES[tag]
    p = gm.default_params_cs() if oa.geometry_kind(base) == "cs" else gm.default_params()
    for k, v in dict(fields, **more).items():
        if not k.startswith("pair_"): setattr(p, k, v)
    if base in oa.GEOMETRY_UNAL: p.sam_unaligned = 1
    return p, {k[5:]: v for k, v in fields.items() if k.startswith("pair_")}


def map_case(gm, tag, max_batch_reads=4096):
    """the records of one case through map_reads / map_reads_cs / map_pairs on a fresh session, and its stats"""
    base = tag.split(":")[0]; kind = oa.geometry_kind(base); n = oa.geometry_reads(tag); g = inputs(base)
    p, pair_fields = params_of(gm, tag)
    s = gm.Session(index_of(gm, base, int(p.list_cutoff)), params=p, max_batch_reads=max_batch_reads)
    try:
        if kind == "pairs":
            opts = gm.PairOpts.default(g["mode"], g["ins"][0], g["ins"][1])
            for k, v in pair_fields.items(): setattr(opts, k, v)
            body = s.map_pairs(g["m1"][:n], g["m2"][:n], g["names1"][:n], g["names2"][:n], opts=opts)
        else: body = (s.map_reads_cs if kind == "cs" else s.map_reads)(g["reads"][:n])
        return body, dict(s.stats)
    finally: s.close()


RELEASE_TAGS = ["stress_60bp:a-1", "stress_60bp:w50abs", "stress_100bp_unal:w300", "stress_cs_60col_unal:a-1", "stress_pairs_2x100:a-1", "pair_edges_col-bw:w100"]
MAP_TAGS = RELEASE_TAGS if os.environ.get("GM_GEOMETRY_RELEASE_CASES") else TAGS      # (the child interpreter of the release build runs six)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", MAP_TAGS)
def test_map_equals_the_reference_golden(gm, tag):
    """map_reads, map_reads_cs and map_pairs under the case's options == the reference's records, byte for byte"""
    got, st = map_case(gm, tag); want = oa.load_geometry_sam(tag)
    assert got == want, (_first_diff(got, want), st)


@pytest.mark.gpu
def test_release_build_reproduces_six_geometry_goldens():
    """`make release` (the build bench.py measures): six cases in a child interpreter with GM_LIB_PATH on libgmapper_hip_release.so"""
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    env = dict(os.environ, GM_LIB_PATH=rel, GM_GEOMETRY_RELEASE_CASES="1")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "test_map_equals_the_reference_golden", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, cwd=oa.ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) == len(RELEASE_TAGS), p.stdout[-500:]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["stress_60bp:a-1", "stress_cs_60col_unal:a-1", "stress_pairs_2x100:a-1"])
def test_no_anchor_band_under_the_heavy_tier_and_in_sub_batches_of_64(gm, tag):
    want = oa.load_geometry_sam(tag)
    with env_set(GM_SCAP="256", GM_SCAP2="64"):
        got, st = map_case(gm, tag)
    assert got == want, (_first_diff(got, want), st)
    got, st = map_case(gm, tag, max_batch_reads=64)
    assert got == want, (_first_diff(got, want), st)


# ---- the seams under the same options ----------------------------------------------------------------------------------------------------------------------------
WINDOW_SETS = ["w100", "w300", "w50abs", "l20abs"]
SEAM_READS = 600
_drv = {}


def driver_rows(L, what):
    """(rows, off) of the windows driver on the first SEAM_READS reads of stress_60bp under an option set, computed once"""
    if what not in _drv:
        g = inputs("stress_60bp"); cs = [np.ascontiguousarray(c, dtype=np.uint8) for c in g["contigs"]]; reads = np.ascontiguousarray(g["reads"][:SEAM_READS], dtype=np.uint8)
        f = oa._GEO_SETS[what][2]; u8p = C.POINTER(C.c_uint8)
        L.rwo_set_windows.argtypes = [C.c_void_p, C.c_double, C.c_double]; L.rwo_set_windows.restype = None
        h = L.rwo_create(len(cs), (u8p * len(cs))(*[c.ctypes.data_as(u8p) for c in cs]), (C.c_uint64 * len(cs))(*[len(c) for c in cs]), 0, 2)
        L.rwo_set_windows(h, f.get("window_len", 140.0), f.get("window_overlap", 90.0))
        cap = 64 * len(reads); rows = np.zeros((cap, 12), dtype=np.int64)
        w = L.rwo_windows(h, reads.shape[0], reads.shape[1], reads.ctypes.data_as(u8p), trw.THREADS, rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
        L.rwo_destroy(h)
        assert 0 < w <= cap
        _drv[what] = (rows[:w].copy(), trw.offsets(rows[:w], len(reads)))
    return _drv[what]


def test_driver_windows_have_the_length_the_option_asks_for(driver):
    """-w 100 %: 60, -w 300 %: 180, -w 50: 50 -- shorter than the read -- and 84 under -l 20; clipped windows apart (the contig of 70 bases, the contigs' ends)"""
    for what, W in (("w100", 60), ("w300", 180), ("w50abs", 50), ("l20abs", 84)):
        rows, _ = driver_rows(driver, what)
        assert int(rows[:, 4].max()) == W and int((rows[:, 4] == W).sum()) >= 0.9 * len(rows) and len(rows) >= 600, (what, W, len(rows))
    assert len(driver_rows(driver, "w300")[0]) != len(driver_rows(driver, "w100")[0])


@pytest.mark.gpu
@pytest.mark.parametrize("what", WINDOW_SETS)
def test_read_windows_equal_the_driver_and_score_windows_the_oracle(gm, driver, oracle_lib, what):
    """Session.read_windows row by row against the windows driver under the option set (w_len, the anchor boxes, the contig clips; groups of equal (read, st, cn, g_off)
    as multisets), then Session.score_windows on those windows against the oracle's sw_vector at the same addresses"""
    from tests.test_many_contigs import oracle_scores
    want, want_off = driver_rows(driver, what)
    tag = "stress_60bp:" + what; g = inputs("stress_60bp"); reads = np.ascontiguousarray(g["reads"][:SEAM_READS], dtype=np.uint8)
    p, _ = params_of(gm, tag)
    s = gm.Session(index_of(gm, "stress_60bp"), params=p, max_batch_reads=4096)
    try:
        wins, off = s.read_windows(reads)
        rows = trw.as_rows(wins)
        assert np.array_equal(off, want_off), np.nonzero(off != want_off)[0][:10]
        a, b = trw.canon(rows), trw.canon(want)
        assert np.array_equal(a, b), (a[(a != b).any(axis=1)][:5], b[(a != b).any(axis=1)][:5])
        scores, _ = s.score_windows(reads, wins, off)
    finally: s.close()
    ws = oracle_scores(rows, g["contigs"], reads, False, False, p)
    bad = np.nonzero(scores != ws)[0]
    assert len(bad) == 0, (len(bad), rows[bad[:5]], scores[bad[:5]], ws[bad[:5]])
    assert int(ws.max()) == 10 * min(60, int(rows[:, 4].max()))


@pytest.mark.gpu
def test_read_hits_equal_the_three_calls_under_an_absolute_overlap(gm):
    """-l 20 decides in pass 1's overlap rule: Session.read_hits == read_windows -> score_windows -> select_pass1 on the same session"""
    from tests import test_pass1_seam as tps
    reads = np.ascontiguousarray(inputs("stress_60bp")["reads"][:SEAM_READS], dtype=np.uint8)
    p, _ = params_of(gm, "stress_60bp:l20abs")
    s = gm.Session(index_of(gm, "stress_60bp"), params=p, max_batch_reads=4096)
    try:
        want = tps.chain_of(s, p, reads, cache=True)
        hits, hit_off, wins, off, scores = s.read_hits(reads, want_windows=True)
        tps.same_up_to_equal_windows((wins, off, scores, hits, hit_off), want)
        assert len(set(hits["read"].tolist())) >= 300
    finally: s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["a-1", "a99", "w300"])
def test_read_mappings_equal_the_chain_of_seams(gm, what):
    """Session.read_mappings under -a -1, -a 99 and -w 300 % == its own hits through sw_vector_batch -> sw_full_ls_batch (set up with the same width) -> select_pass2 ->
    the text entry; and through sam_records the reference's bytes"""
    from tests import test_read_mappings as trm
    tag = "stress_100bp_unal:" + what; g = inputs("stress_100bp_unal"); reads = np.ascontiguousarray(g["reads"][:SEAM_READS], dtype=np.uint8)
    p, _ = params_of(gm, tag)
    ix = index_of(gm, "stress_100bp_unal"); s = gm.Session(ix, params=p, max_batch_reads=8192)
    try:
        R = s.read_mappings(reads, want_ops=True)
        c = trm.chain_of(gm, ix, s, p, reads, R)
        n_run = trm.assert_equals_chain(gm, p, R, c)
        assert len(R.hits) > 200 and len(R.maps) > 100 and n_run > 100
        got, off = s.sam_records(reads, R)
    finally: s.close()
    skip = set()                                                        # (stress_100bp_unal has no groups of equal windows: every read is compared)
    want = trm.by_read(oa.load_geometry_sam(tag), len(g["reads"]))
    bad = [r for r in range(len(reads)) if r not in skip and got[int(off[r]):int(off[r + 1])] != want[r]]
    assert not bad, (len(bad), [(got[int(off[r]):int(off[r + 1])], want[r]) for r in bad[:3]])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["a-1", "a99", "w300", "local_a-1"])
def test_read_mappings_cs_equal_the_chain_of_seams(gm, oracle_lib, what):
    """colour space: Session.read_mappings_cs == its hits through sw_full_cs_batch (set up with the same width) -> post_sw_batch -> select_pass2 -> the text entry, and
    through sam_records the reference's bytes.  -a 99 (the widest widening: a band far outside the matrix in the kernels' int corner) has no golden in colour space:
    its records are held to the oracle's at that width, and map_reads_cs on the same session too"""
    from tests import test_read_mappings_cs as trc
    g = inputs("stress_cs_60col_unal")
    F = dict(contigs=g["contigs"], cnames=None, reads=np.ascontiguousarray(g["reads"][:SEAM_READS], dtype=np.uint8), names=None, quals=None, qual_delta=33)
    if what == "a99":
        tag = None; p, _ = params_of(gm, "stress_cs_60col_unal:a-1", anchor_width=99)
        want_text = oracle_records("stress_cs_60col_unal:a-1", "anchor-width=99")
        assert oa.geometry_reads("stress_cs_60col_unal:a-1") == SEAM_READS and oa.sam_distance(want_text, oa.load_geometry_sam("stress_cs_60col_unal:a0")) >= oa.GEOMETRY_MIN_DISTANCE
    else:
        tag = "stress_cs_60col_unal:" + what; p, _ = params_of(gm, tag); want_text = oa.load_geometry_sam(tag)
    ix = index_of(gm, "stress_cs_60col_unal"); s = gm.Session(ix, params=p, max_batch_reads=8192)
    try:
        R = s.read_mappings_cs(F["reads"], want_ops=True)
        c = trc.chain_of(gm, ix, s, p, F, R)
        trc.assert_equals_chain(gm, p, R, c)
        assert len(R.hits) > 200 and len(R.maps) > 100
        mine = trc.sam_of(s, F, R)
        skip = trc.tied(s, F)
        if tag is None: assert s.map_reads_cs(F["reads"]) == want_text
    finally: s.close()
    want = trc.by_read(want_text, None, len(g["reads"]))
    bad = [r for r in range(SEAM_READS) if r not in skip and mine[r] != want[r]]
    assert not bad, (len(bad), [(mine[r], want[r]) for r in bad[:3]])


# ---- the stripe gate of pass 1 (read_len > 128 && window_len > 256) from both sides ---------------------------------------------------------------------------------
# read length, -w: two stripes with the carry row in registers (W = 129, 182), one stripe on windows beyond 256 columns (W = 300), two stripes with the carry rows in LDS (W = 258)
GATE_SHAPES = [(129, 100.0), (182, 100.0), (100, 300.0), (129, 200.0)]
_gate = {}


def gate_inputs(L, colour):
    """a genome of 2 x 60 000 bases and 200 reads planted in it (2 % substitutions, indels in a few), once per shape"""
    from shrimp_amd import synth
    key = (L, colour)
    if key not in _gate:
        contigs = synth.make_genome([60_000, 60_000], 31)
        reads = synth.make_cs_reads(contigs, 200, L, 32 + L)[0] if colour else synth.make_reads(contigs, 200, L, 32 + L, p_sub=0.02, p_ins=0.002, p_del=0.002)[0]
        _gate[key] = (contigs, np.ascontiguousarray(reads, dtype=np.uint8))
    return _gate[key]


@pytest.mark.parametrize("colour", [False, True], ids=["letters", "colours"])
@pytest.mark.parametrize("L,w", GATE_SHAPES)
def test_oracle_maps_the_planted_reads_of_the_gate_shapes(oracle_lib, L, w, colour):
    """(the reference the GPU test below compares with is not empty: at least 150 of the 200 reads get a record, and the windows are as long as the shape says)"""
    contigs, reads = gate_inputs(L, colour)
    o = oa.Session(contigs, opts=("colour=1;" if colour else "") + "match-window=%d" % w)
    body = o.map_sam(reads, nthreads=4); o.close()
    assert len({l.split(b"\t")[0] for l in body.split(b"\n") if l}) >= 150
    _gate[(L, w, colour)] = body


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [False, True], ids=["letters", "colours"])
@pytest.mark.parametrize("L,w", GATE_SHAPES)
def test_stripe_gate_shapes_equal_the_oracle(gm, oracle_lib, L, w, colour):
    contigs, reads = gate_inputs(L, colour)
    if (L, w, colour) not in _gate:
        o = oa.Session(contigs, opts=("colour=1;" if colour else "") + "match-window=%d" % w); _gate[(L, w, colour)] = o.map_sam(reads, nthreads=4); o.close()
    want = _gate[(L, w, colour)]
    p = gm.default_params_cs() if colour else gm.default_params()
    p.window_len = w
    ix = gm.Index(contigs, params=gm.default_params_cs() if colour else gm.default_params()); s = gm.Session(ix, params=p, max_batch_reads=4096)
    try:
        got = (s.map_reads_cs if colour else s.map_reads)(reads); st = dict(s.stats)
    finally: s.close(); ix.close()
    assert got == want, (_first_diff(got, want), st)
    assert len({l.split(b"\t")[0] for l in want.split(b"\n") if l}) >= 150


# ---- refusals, each with a good call behind it ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_anchor_widths_outside_the_reference_range_are_refused(gm):
    """-a takes -1 .. 99 (gmapper.c:2014-2016): gm_session_create and both setups refuse -2 and 100 with GM_E_ARG and name the value; -1 and 99 are taken, and a default
    session on the same index maps its golden's first reads afterwards"""
    L = gm.lib(); ix = index_of(gm, "stress_60bp")
    for bad in (-2, 100):
        p = gm.default_params(); p.anchor_width = bad
        with pytest.raises(gm.GmError) as e: gm.Session(ix, params=p)
        assert "(%d)" % GM_E_ARG in str(e.value) and "anchor_width %d" % bad in str(e.value) and "[-1, 99]" in str(e.value), str(e.value)
        assert L.sw_full_ls_setup(1400, 1000, -33, -7, -33, -3, 10, -15, True, bad) == GM_E_ARG and b"anchor_width" in L.gm_last_error()
        assert L.sw_full_cs_setup(1400, 1000, -33, -7, -33, -3, 10, -24, -20, True, bad, 0) == GM_E_ARG and b"anchor_width" in L.gm_last_error()
    for good in (-1, 99):
        assert L.sw_full_ls_setup(1400, 1000, -33, -7, -33, -3, 10, -15, True, good) == 0 and L.sw_full_cs_setup(1400, 1000, -33, -7, -33, -3, 10, -24, -20, True, good, 0) == 0
    s = gm.Session(ix, max_batch_reads=4096)
    try: got = s.map_reads(inputs("stress_60bp")["reads"][:300])
    finally: s.close()
    assert got == oa.geometry_default_records("stress_60bp", 300)


@pytest.mark.gpu
def test_a_window_beyond_the_lds_of_pass_2_is_refused(gm):
    """pass 2 keeps a window's carry rows in LDS: four windows a wave in letter space, 4 x (112 + 16 ceil(W / 16) + 12 W) + 64 bytes beside reads of 100 -- 3 140 columns fit
    into the 160 KB of a CU, 3 141 do not.  map_reads refuses the longer window with GM_E_RANGE, the value and the limit named, and maps with the limit's neighbourhood
    left alone: -w 300 % on the same session's index afterwards gives its golden."""
    g = inputs("stress_100bp_unal"); ix = index_of(gm, "stress_100bp_unal")
    for w, limit in ((-3141.0, 3140), (3200.0, 3140)):
        p = gm.default_params(); p.window_len = w
        s = gm.Session(ix, params=p, max_batch_reads=4096)
        try:
            with pytest.raises(gm.GmError) as e: s.map_reads(g["reads"][:64])
            msg = str(e.value)
            assert "(%d)" % GM_E_RANGE in msg and "window length %d" % (3141 if w < 0 else 3200) in msg and "%d columns" % limit in msg, msg
        finally: s.close()
    got, st = map_case(gm, "stress_100bp_unal:w300")
    assert got == oa.load_geometry_sam("stress_100bp_unal:w300"), st


@pytest.mark.gpu
def test_a_window_beyond_the_lds_of_pass_2_is_refused_in_colour_space_and_per_mate(gm):
    """the other shapes gm_pass2_max_window answers for, by the launchers' own size functions: colour space, global alignment (the one-window kernel: 5 x 64 + 16 ceil(W / 16)
    + 48 W + 64 bytes beside 60 colours -- 3 335 columns), colour space, local alignment (the four-window kernel with int rows: 829), and map_pairs, which asks per mate:
    under -w 3145 the mate of 40 bases is within its limit (3 145) and the mate of 60 is not (3 144).  One column beyond each limit is refused with GM_E_RANGE, the limit
    named, and -w 300 % / -w 100 % on the same indexes map their goldens afterwards."""
    g = inputs("stress_cs_60col_unal"); ix = index_of(gm, "stress_cs_60col_unal")
    for local, limit in ((0, 3335), (1, 829)):
        p = gm.default_params_cs(); p.window_len = -(limit + 1.0); p.local_alignment = local
        s = gm.Session(ix, params=p, max_batch_reads=4096)
        try:
            with pytest.raises(gm.GmError) as e: s.map_reads_cs(g["reads"][:64])
            msg = str(e.value)
            assert "(%d)" % GM_E_RANGE in msg and "window length %d" % (limit + 1) in msg and "reads of 60" in msg and "%d columns" % limit in msg, msg
        finally: s.close()
    got, st = map_case(gm, "stress_cs_60col_unal:w300")
    assert got == oa.load_geometry_sam("stress_cs_60col_unal:w300"), st
    ge = inputs("pair_edges_opp-in"); ixp = index_of(gm, "pair_edges_opp-in")
    p = gm.default_params(); p.window_len = -3145.0
    s = gm.Session(ixp, params=p, max_batch_reads=4096)
    try:
        with pytest.raises(gm.GmError) as e:
            s.map_pairs(ge["m1"][:32], ge["m2"][:32], ge["names1"][:32], ge["names2"][:32], opts=gm.PairOpts.default(ge["mode"], ge["ins"][0], ge["ins"][1]))
        msg = str(e.value)
        assert "(%d)" % GM_E_RANGE in msg and "window length 3145" in msg and "reads of 60" in msg and "3144 columns" in msg, msg
    finally: s.close()
    got, st = map_case(gm, "pair_edges_opp-in:w100")
    assert got == oa.load_geometry_sam("pair_edges_opp-in:w100"), st


# ---- the batch entries at the known answers of other anchor widths --------------------------------------------------------------------------------------------------
def ls_setup_args(setup): return setup[:8] + (True, setup[8])
def cs_setup_args(setup): return setup[:9] + (True, setup[10], setup[9])


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_full_ls_batch_equals_the_F_G_and_L_records_at_the_width(gm, w):
    """one gm_sw_full_ls_batch call a record kind after sw_full_ls_setup with the width: global at threshold 0, global at half the read's score, local with the box and without"""
    s = ls_width(w)
    gm.sw_full_ls_setup(*ls_setup_args(s["setup"]))
    for kind, local in (("F", False), ("G", False), ("L", True)):
        recs, ops, strings, bases = run_ls(gm, s[kind], local=local)
        check_ls(s[kind], recs, strings, bases)
        assert int(recs["n_ops"].sum()) == ops.size
    it = s["G"][0]                                                                  # the single seam
    f, db, qr = gm.sw_full_ls(it["g"], it["goff"], it["glen"], it["r"], it["rlen"], it["anchor"], revcmpl=bool(it["rv"]), threshscore=it["thresh"], maxscore=it["maxscore"])
    assert [f[k] for k in LS_FIELDS] == it["want"] and (db, qr) == (it["db"], it["qr"])


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_full_cs_batch_equals_the_S_and_L_records_at_the_width(gm, w):
    s = cs_width(w)
    gm.sw_full_cs_setup(*cs_setup_args(s["setup"]))
    for kind, local in (("S", False), ("L", True)):
        recs, ops, strings, bases = run_cs(gm, s[kind], local=local)
        check_cs(s[kind], recs, strings, bases)
    it = next(i for i in s["S"] if i["want"][0] > 0)
    f, db, qr = gm.sw_full_cs(it["g"], it["goff"], it["glen"], it["r"], it["rlen"], it["initbp"], it["thresh"], it["anchor"], revcmpl=bool(it["rv"]))
    assert [f[k] for k in CS_FIELDS] == it["want"] and (db, qr) == (it["db"], it["qr"])
    if w == -1:                                                                     # no box at all: the reference's anchors == NULL, the same band -- at the seam and in the batch entry
        f, db, qr = gm.sw_full_cs(it["g"], it["goff"], it["glen"], it["r"], it["rlen"], it["initbp"], it["thresh"], None, revcmpl=bool(it["rv"]))
        assert [f[k] for k in CS_FIELDS] == it["want"] and (db, qr) == (it["db"], it["qr"])
        bare = [dict(i, anchor=None) for i in s["S"]]
        recs, ops, strings, bases = run_cs(gm, bare, local=False)
        check_cs(bare, recs, strings, bases)
    else:                                                                           # ... which any other width refuses, as before
        assert gm.sw_full_cs(it["g"], it["goff"], it["glen"], it["r"], it["rlen"], it["initbp"], it["thresh"], None)[0]["score"] == 0 and b"anchor box" in gm.lib().gm_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("w", [-1, 9])
def test_the_records_of_two_widths_laid_into_an_index(gm, w):
    """the same records through gm_sw_full_ls_batch_ix / gm_sw_full_cs_batch_ix on strand 0 (the layout of tests/test_seam_batch_ix.py)"""
    from tests import test_seam_batch_ix as tx
    s = ls_width(w)
    gm.sw_full_ls_setup(*ls_setup_args(s["setup"]))
    for kind, local in (("F", False), ("G", False), ("L", True)):
        its = s[kind]
        contigs, cn, base = tx.lay_out([it["g"] for it in its]); ix = gm.Index(contigs); a = tx.arrays(its)
        recs, ops, strings = ix.sw_full_ls_batch(cn, np.zeros(len(its), dtype=np.uint8), base + a["goff"], a["glen"], a["reads"], a["rlen"], a["anchors"], a["rv"], a["thresh"],
                                                 a["maxscore"], local_alignment=local)
        strings.prefetch()
        check_ls(its, recs, strings, base)
        ix.close()
    c = cs_width(w)
    gm.sw_full_cs_setup(*cs_setup_args(c["setup"]))
    for kind, local in (("S", False), ("L", True)):
        its = c[kind]
        contigs, cn, base = tx.lay_out([it["g"] for it in its]); ix = gm.Index(contigs, params=gm.default_params_cs()); a = tx.arrays(its)
        recs, ops, strings = ix.sw_full_cs_batch(cn, np.zeros(len(its), dtype=np.uint8), base + a["goff"], a["glen"], a["reads"], a["rlen"], a["initbp"], a["anchors"], a["rv"],
                                                 a["thresh"], xover=a["xs"], is_rna=0, local_alignment=local)
        strings.prefetch()
        check_cs(its, recs, strings, base)
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("w", [-1, 99])
def test_mangled_seams_replay_two_widths(gm, tmp_path, w):
    """tests/seam_driver.cpp (a C++ caller through the names the reference's objects ask for) with the width in its setups: the letter-space F records and the
    colour-space S and L records of the width.  The driver's F request is global at threshold 0 -- at width -1 that band is the whole matrix, so a thresholded band goes
    through sw_full_ls's mangled name only in colour space here (S, L); the letter-space G and L records are held through the batch and _ix entries above"""
    from tests.test_gpu_parity import _seam_driver, _hexw
    exe = _seam_driver(tmp_path)
    ls, cs = ls_width(w), cs_width(w)
    req = ["width %d" % w, "setup_v 0 -15", "setup_f_ls"]; want = []
    for it in ls["F"]:
        req.append("F %d %d %d %d %d %d %d %d %s %s" % ((it["goff"], it["glen"], it["rlen"]) + tuple(it["anchor"]) + (int(it["rv"]), _hexw(it["g"]), _hexw(it["r"]))))
        want.append("F " + " ".join(str(x) for x in it["want"]) + " %s %s" % (it["db"], it["qr"]))
    req += ["setup_f_cs"]
    for kind in "SL":
        for it in cs[kind]:
            req.append("%s %d %d %d %d %d %d %d %d %d %d %s %s" % ((kind, it["goff"], it["glen"], it["rlen"], it["initbp"]) + tuple(it["anchor"]) + (int(it["rv"]), it["thresh"], _hexw(it["g"]), _hexw(it["r"]))))
            want.append(kind + " " + " ".join(str(x) for x in it["want"]) + " %s %s" % (it["db"] or "-", it["qr"] or "-") if it["want"][0] != 0 else None)      # score 0: nothing else is defined
    assert len(want) >= 500
    p = subprocess.run([exe], input=("\n".join(req) + "\n").encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.decode().split("\n")
    assert len(got) == len(want) + 1 and got[-1] == ""
    for k, (g_, w_) in enumerate(zip(got, want)):
        if w_ is None: assert g_.split()[1] == "0", (k, g_)
        else: assert g_ == w_, (k, g_, w_)
