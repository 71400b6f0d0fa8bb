"""The Smith-Waterman kernels at other score sets than the defaults.

Every kernel takes its scores at run time, and every other kernel-level test hands it one set (10 / -15, gaps -33/-7 and -33/-3; colour space 10 / -24, crossover -20).
tests/golden/sw_kat_scores.txt.gz and sw_kat_cs_scores.txt.gz hold the reference's own answers (oracle/ref_kat.cpp, ref_kat_cs.cpp, mode "scores") at

    unit     1 / -1,   gaps  -1/-1   and  -1/-1      smallest values, maximal ties
    linear  10 / -15,  gaps   0/-12  and   0/-9      open 0: the affine recurrences degenerate
    swapped 10 / -15,  gaps -20/-2   and -45/-9      the genome-side gap much cheaper than the read-side one
    steep    7 / -40,  gaps -60/-1   and -25/-30     extend > open on one side, a mismatch dearer than a short gap
    large   32 / -60,  gaps -100/-20 and -90/-25     int16 headroom: 32 x 1000 = 32000

(colour space: crossovers -1, -14, -20, -40, -60, and "swapped" once more with indel_taboo_len 3).  Without a GPU the CPU restatement is held to them through its
score-taking entry points (gmo_*_p); on the GPU the batch seams are, one call per set and entry, and beyond the fixtures' shapes against the restatement."""
import ctypes as C
import numpy as np
import pytest
from tests import oracle_api as oa
from tests.test_sw_full_batch import _item, run_ls, run_cs, check_ls, check_cs, LS_FIELDS, CS_FIELDS

LS_SETS = ["unit", "linear", "swapped", "steep", "large"]
CS_SETS = LS_SETS + ["swapped_taboo"]
IX_SETS = ["swapped", "large"]                                   # the sets that also go through the resident index
GM_E_RANGE = -4
u32p = C.POINTER(C.c_uint32)
_u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32).ctypes.data_as(u32p)

_cache = {}


def ls_set(name):
    """setup tuple, V records, F / L items (the item dicts of tests/test_sw_full_batch.py) of one letter-space set"""
    if "ls" not in _cache:
        d = {}
        for nm, setup, recs in oa.load_kat_scores(False):
            V = [r for r in recs if r[0] == "V"]
            F = [_item(r[9], r[1], r[2], r[10], r[3], tuple(r[4:8]), r[8], want=r[11], db=r[12], qr=r[13]) for r in recs if r[0] == "F"]
            L = [_item(g, goff, glen, rd, rlen, None if no_anchor else (ax, ay, alen, aw), rv, thresh, sv, want=want, db=db, qr=qr)
                 for (goff, glen, rlen, ax, ay, alen, aw, rv, no_anchor, thresh, sv), g, rd, want, db, qr in (r for r in recs if isinstance(r[0], tuple))]
            d[nm] = dict(setup=setup, V=V, F=F, L=L)
        _cache["ls"] = d
    return _cache["ls"][name]


def cs_set(name):
    """setup tuple, C records, S / L / X / Y items of one colour-space set"""
    if "cs" not in _cache:
        d = {}
        for nm, setup, recs in oa.load_kat_scores(True):
            e = dict(setup=setup, C=[r for r in recs if r[0] == "C"], S=[], L=[], X=[], Y=[])
            for r in recs:
                if r[0] == "C": continue
                (goff, glen, rlen, initbp, ax, ay, alen, aw, rv, thresh), gls, rd, want, db, qr = r[1:7]
                e[r[0]].append(_item(gls, goff, glen, rd, rlen, (ax, ay, alen, aw), rv, thresh, initbp=initbp, xs=r[7] if len(r) > 7 else None, want=want, db=db, qr=qr))
            d[nm] = e
        _cache["cs"] = d
    return _cache["cs"][name]


def vector_args(setup, colour):
    """sw_vector_setup's arguments of a set (colour space: mismatch = match + crossover, ref: gmapper.c:2935)"""
    return setup[:6] + (setup[6], setup[6] + setup[8] if colour else setup[7], 1 if colour else 0, True)


def full_ls_args(setup): return setup[:8] + (True, 8)
def full_cs_args(setup): return setup[:9] + (True, 8, setup[9])


def test_fixtures_hold_every_set_and_record_kind():
    for name in LS_SETS:
        s = ls_set(name)
        assert len(s["V"]) >= 150 and len(s["F"]) >= 200 and len(s["L"]) >= 300, (name, len(s["V"]), len(s["F"]), len(s["L"]))
        assert any(it["anchor"] is None for it in s["L"]) and any(it["anchor"] is not None for it in s["L"])
        assert sum("-" in it["db"] or "-" in it["qr"] for it in s["F"]) >= 20, name                     # alignments with gaps
    assert [ls_set(n)["setup"][6] for n in LS_SETS] == [1, 10, 10, 7, 32]
    long_v = ls_set("large")["V"][-12:]                                                               # the set's last records: reads of more than one stripe
    assert sorted(r[3] for r in long_v) == [129] * 3 + [256] * 3 + [257] * 3 + [1000] * 3
    assert sum(r[2] <= 256 for r in long_v) == 6 and max(r[6] for r in long_v) >= 31000                 # half on windows of at most 256 columns; near the int16 ceiling
    for name in CS_SETS:
        s = cs_set(name)
        assert len(s["C"]) >= 150 and len(s["S"]) >= 300 and len(s["L"]) >= 150 and len(s["X"]) >= 150 and len(s["Y"]) >= 70, name
        gx = s["setup"][8]
        assert all(it["xs"].min() >= 2 * gx and it["xs"].max() <= -1 for it in s["X"] + s["Y"])
        assert sum(it["want"][9] > 0 for it in s["S"]) >= 20 and sum("-" in it["db"] or "-" in it["qr"] for it in s["S"]) >= 10, name
    assert cs_set("swapped_taboo")["setup"][9] == 3 and cs_set("swapped_taboo")["setup"][:9] == cs_set("swapped")["setup"][:9]


# ---- the CPU restatement against the reference's answers, set by set ------------------------------------------------------------------------------------
def _oracle_ls(L, sc, it, local):
    out = (C.c_int * 9)(); db = C.create_string_buffer(4096); qr = C.create_string_buffer(4096)
    a = it["anchor"] if it["anchor"] is not None else (0, 0, 1, 1)
    rc = L.gmo_sw_full_ls_p(sc, _u32(it["g"]), it["goff"], it["glen"], _u32(it["r"]), it["rlen"], it["thresh"], it["maxscore"], a[0], a[1], a[2], a[3],
                            0 if it["anchor"] is None else 1, int(it["rv"]), 1 if local else 0, out, db, qr, 4096)
    assert rc == 0
    return list(out), db.value.decode(), qr.value.decode()


def _oracle_cs(L, sc, it, local):
    out = (C.c_int * 10)(); db = C.create_string_buffer(4096); qr = C.create_string_buffer(4096)
    a = it["anchor"]
    xs = None if it["xs"] is None else np.ascontiguousarray(it["xs"], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    rc = L.gmo_sw_full_cs_p(sc, _u32(it["g"]), it["goff"], it["glen"], _u32(it["r"]), it["rlen"], it["initbp"], it["thresh"], a[0], a[1], a[2], a[3], int(it["rv"]),
                            1 if local else 0, xs, out, db, qr, 4096)
    assert rc == 0
    return list(out), db.value.decode(), qr.value.decode()


@pytest.mark.parametrize("name", LS_SETS)
def test_oracle_letter_space_equals_the_reference_at_the_set(oracle_lib, name):
    s = ls_set(name); sc = oa.score_array(s["setup"])
    for _, goff, glen, rlen, g, r, score in s["V"]:
        assert oracle_lib.gmo_sw_vector_p(sc, _u32(g), goff, glen, _u32(r), rlen) == score, (name, goff, glen, rlen)
    for kind, local in (("F", False), ("L", True)):
        for k, it in enumerate(s[kind]):
            got, db, qr = _oracle_ls(oracle_lib, sc, it, local)
            assert got == it["want"] and (db, qr) == (it["db"], it["qr"]), (name, kind, k, got, it["want"], db, it["db"], qr, it["qr"])


@pytest.mark.parametrize("name", CS_SETS)
def test_oracle_colour_space_equals_the_reference_at_the_set(oracle_lib, name):
    s = cs_set(name); sc = oa.score_array(s["setup"])
    for _, goff, glen, rlen, initbp, gcs, gls, rd, score in s["C"]:
        assert oracle_lib.gmo_sw_vector_cs_p(sc, _u32(gcs), goff, glen, _u32(rd), rlen, _u32(gls), initbp) == score, (name, goff, glen, rlen)
    for kind, local in (("S", False), ("L", True), ("X", False), ("Y", True)):
        for k, it in enumerate(s[kind]):
            got, db, qr = _oracle_cs(oracle_lib, sc, it, local)
            if it["want"][0] == 0:                                   # below the threshold: score 0 and no strings
                assert got[0] == 0 and db == "" and qr == "", (name, kind, k, got)
                continue
            assert got == it["want"] and (db, qr) == (it["db"], it["qr"]), (name, kind, k, got, it["want"], db, it["db"], qr, it["qr"])


def test_setup_refuses_match_times_qrlen_at_the_boundary():
    """sw_vector_setup refuses match * qrlen >= 32768 before it asks for a device (ref: sw-vector.c:393-398): 32 x 1024 is refused, 32 x 1023 is not"""
    from shrimp_amd import gmapper as gm
    L = gm.lib()
    assert L.sw_vector_setup(1400, 1024, -100, -20, -90, -25, 32, -60, 0, True) == GM_E_RANGE and b"32768" in L.gm_last_error()
    assert L.sw_vector_setup(1400, 1023, -100, -20, -90, -25, 32, -60, 0, True) != GM_E_RANGE
    assert L.sw_vector_setup(1400, 32768, -1, -1, -1, -1, 1, -1, 0, True) == GM_E_RANGE
    assert L.sw_vector_setup(1400, 32767, -1, -1, -1, -1, 1, -1, 0, True) != GM_E_RANGE


# ---- the early stop's inputs (made once; the oracle's full scores say on the CPU that both outcomes are there) ------------------------------------------
EARLY_SETS = ["unit", "swapped", "large"]
EARLY_N = 1500


def early_inputs(L):
    """1 500 windows of read length L: a third true hits (6 % substitutions), a third reads of which a part is random (scores around the middle threshold), a third
    chance windows with two seed-like runs -- the recipe of test_sw_vector_early_stop_is_exact_about_the_threshold"""
    key = ("early", L)
    if key not in _cache:
        from shrimp_amd import synth
        rng = np.random.default_rng(41 + L)
        n = EARLY_N
        G = rng.integers(0, 4, size=120_000, dtype=np.uint8)
        G[rng.integers(0, G.size, 120)] = 15
        starts = rng.integers(0, G.size - 600, size=n)
        reads = np.stack([G[s + 20:s + 20 + L].copy() for s in starts])
        reads = np.where(rng.random(reads.shape) < 0.06, rng.integers(0, 4, size=reads.shape), reads).astype(np.uint8)
        third = n // 3
        for i in range(third, 2 * third):
            cut = int(rng.integers(3 * L // 10, 7 * L // 10))
            if rng.integers(0, 2): reads[i, cut:] = rng.integers(0, 4, size=L - cut)
            else: reads[i, :cut] = rng.integers(0, 4, size=cut)
        for i in range(2 * third, n):
            keep = np.zeros(L, dtype=bool)
            for _ in range(2):
                a = int(rng.integers(0, L - 14)); keep[a:a + 14] = True
            reads[i] = np.where(keep, reads[i], rng.integers(0, 4, size=L))
        glen = np.full(n, int(1.4 * L), dtype=np.int32); glen[::7] = L - 10; glen[3::11] = 250
        _cache[key] = dict(gw=synth.pack_nibbles(G), rw=synth.pack_reads(reads), starts=starts, glen=glen, rlen=np.full(n, L, dtype=np.int32))
    return _cache[key]


def early_full(name, L):
    """the oracle's full scores of early_inputs(L) at the set"""
    key = ("early_full", name, L)
    if key not in _cache:
        e = early_inputs(L)
        _cache[key] = oa.sw_vector_batch_p(oa.score_array(ls_set(name)["setup"]), e["gw"], e["starts"], e["glen"], e["rw"], e["rlen"])
    return _cache[key]


def early_thresholds(name, L):
    m = ls_set(name)["setup"][6]
    return [int(0.3 * m * L), int(0.47 * m * L), int(0.7 * m * L)]


@pytest.mark.parametrize("L", [100, 150])
@pytest.mark.parametrize("name", EARLY_SETS)
def test_early_stop_inputs_hold_both_outcomes_at_the_middle_threshold(name, L):
    full = early_full(name, L); mid = early_thresholds(name, L)[1]
    assert (full >= mid).sum() > EARLY_N // 5 and (full < mid).sum() > EARLY_N // 5, (name, L, int((full >= mid).sum()))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------
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
    gmapper.sw_vector_setup(1400, 1000, -33, -7, -33, -3, 10, -15, 0, True)            # leave the thread's setups at the defaults
    gmapper.sw_full_ls_setup(1400, 1000, -33, -7, -33, -3, 10, -15, True, 8)
    gmapper.sw_full_cs_setup(1400, 1000, -33, -7, -33, -3, 10, -24, -20, True, 8, 0)


def lay_end_to_end(bitfields):
    """the records' bitfields laid end to end, each on a word boundary -> (words, first position of each)"""
    bases, at = [], 0
    for g in bitfields: bases.append(at * 8); at += len(g)
    return np.concatenate(bitfields), np.array(bases, dtype=np.int64)


def reads_matrix(reads, rlens):
    rw = max(max(len(r) for r in reads), max((int(n) + 7) // 8 for n in rlens))
    out = np.zeros((len(reads), rw), dtype=np.uint32)
    for i, r in enumerate(reads): out[i, :len(r)] = r
    return out


@pytest.mark.gpu
def test_setup_accepts_the_last_read_length_below_the_boundary(gm):
    L = gm.lib()
    assert L.sw_vector_setup(1400, 1023, -100, -20, -90, -25, 32, -60, 0, True) == 0
    assert L.sw_vector_setup(1400, 1024, -100, -20, -90, -25, 32, -60, 0, True) == GM_E_RANGE
    g = np.zeros(130, dtype=np.uint32); r = np.zeros(128, dtype=np.uint32)            # the accepted setup still stands: 1 023 A against 1 030 A
    assert gm.sw_vector(g, 3, 1030, r, 1023) == 32 * 1023


@pytest.mark.gpu
@pytest.mark.parametrize("name", LS_SETS)
def test_vector_batch_equals_the_V_records(gm, name):
    s = ls_set(name); V = s["V"]
    gm.sw_vector_setup(*vector_args(s["setup"], False))
    words, bases = lay_end_to_end([r[4] for r in V])
    goff, glen, rlen, want = (np.array([r[k] for r in V], dtype=np.int64) for k in (1, 2, 3, 6))
    got = gm.sw_vector_batch(words, bases + goff, glen, reads_matrix([r[5] for r in V], rlen), rlen)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]], glen[bad[:10]], rlen[bad[:10]])
    _, goff, glen, rlen, g, r, score = V[0]
    assert gm.sw_vector(g, goff, glen, r, rlen) == score


@pytest.mark.gpu
@pytest.mark.parametrize("name", CS_SETS)
def test_vector_batch_cs_equals_the_C_records(gm, name):
    s = cs_set(name); Cr = s["C"]
    gm.sw_vector_setup(*vector_args(s["setup"], True))
    gcs, bases = lay_end_to_end([r[5] for r in Cr]); gls, bases2 = lay_end_to_end([r[6] for r in Cr])
    assert np.array_equal(bases, bases2)
    goff, glen, rlen, initbp, want = (np.array([r[k] for r in Cr], dtype=np.int64) for k in (1, 2, 3, 4, 8))
    got = gm.sw_vector_batch_cs(gcs, gls, bases + goff, glen, reads_matrix([r[7] for r in Cr], rlen), rlen, initbp)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]])
    _, goff, glen, rlen, initbp, g_cs, g_ls, rd, score = Cr[0]
    assert gm.sw_vector(g_cs, goff, glen, rd, rlen, genome_ls=g_ls, initbp=initbp) == score


@pytest.mark.gpu
@pytest.mark.parametrize("name", LS_SETS)
def test_full_ls_batch_equals_the_F_and_L_records(gm, name):
    """global and local (anchor box and NULL in one call): every integer field, and the strings gm_sw_full_batch_strings rebuilds"""
    s = ls_set(name)
    gm.sw_full_ls_setup(*full_ls_args(s["setup"]))
    for kind, local in (("F", False), ("L", True)):
        recs, ops, strings, bases = run_ls(gm, s[kind], local=local)
        check_ls(s[kind], recs, strings, bases)
        assert int(recs["n_ops"].sum()) == ops.size
    it = s["F"][0]                                                                  # the single seam
    f, db, qr = gm.sw_full_ls(it["g"], it["goff"], it["glen"], it["r"], it["rlen"], it["anchor"], revcmpl=bool(it["rv"]))
    assert [f[k] for k in LS_FIELDS] == it["want"] and (db, qr) == (it["db"], it["qr"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CS_SETS)
def test_full_cs_batch_equals_the_S_L_X_and_Y_records(gm, name):
    """global, local, and both with a crossover_scores row; the set with indel_taboo_len 3 among them"""
    s = cs_set(name)
    gm.sw_full_cs_setup(*full_cs_args(s["setup"]))
    for kind, local in (("S", False), ("L", True), ("X", False), ("Y", True)):
        assert (kind in "XY") == all(it["xs"] is not None for it in s[kind])
        recs, ops, strings, bases = run_cs(gm, s[kind], local=local)
        check_cs(s[kind], recs, strings, bases)
        assert any(it["want"][0] > 0 for it in s[kind])
    it = next(i for i in s["S"] if i["want"][0] > 0)
    f, db, qr = gm.sw_full_cs(it["g"], it["goff"], it["glen"], it["r"], it["rlen"], it["initbp"], it["thresh"], it["anchor"], revcmpl=bool(it["rv"]))
    assert [f[k] for k in CS_FIELDS] == it["want"] and (db, qr) == (it["db"], it["qr"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", IX_SETS)
def test_the_records_laid_into_an_index(gm, name):
    """the same records through gm_sw_vector_batch_ix and gm_sw_full_ls / cs_batch_ix on strand 0 (the layout of tests/test_seam_batch_ix.py: five contigs, no contig
    start on a word boundary): every V, F and L record of the letter-space set and every S, L, X and Y record of the colour-space one.  Of the C records those whose
    window starts behind their bitfield's first colour (goff >= 1, as tests/test_seam_batch_ix.py::c_records takes them: the index derives a contig's first colour
    from T, the record's bitfield carries its own) -- at least half must remain; in these fixtures all 150 a set do."""
    from tests import test_seam_batch_ix as tx
    s = ls_set(name)
    V = s["V"]
    contigs, cn, base = tx.lay_out([r[4] for r in V]); ix = gm.Index(contigs)
    gm.sw_vector_setup(*vector_args(s["setup"], False))
    goff, glen, rlen, want = (np.array([r[k] for r in V], dtype=np.int64) for k in (1, 2, 3, 6))
    got = ix.sw_vector_batch(cn, np.zeros(len(V), dtype=np.uint8), base + goff, glen, reads_matrix([r[5] for r in V], rlen), rlen)
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:10])
    ix.close()
    gm.sw_full_ls_setup(*full_ls_args(s["setup"]))
    for kind, local in (("F", False), ("L", True)):
        its = s[kind]
        contigs, cn, base = tx.lay_out([it["g"] for it in its]); ix = gm.Index(contigs); a = tx.arrays(its)
        recs, ops, strings = ix.sw_full_ls_batch(cn, np.zeros(len(its), dtype=np.uint8), base + a["goff"], a["glen"], a["reads"], a["rlen"], a["anchors"], a["rv"], a["thresh"],
                                                 a["maxscore"], local_alignment=local)
        strings.prefetch()
        check_ls(its, recs, strings, base)
        ix.close()
    c = cs_set(name)
    Cr = [r for r in c["C"] if r[1] >= 1]                          # windows behind their bitfield's first colour (that colour is the record's own, not a contig's)
    assert 2 * len(Cr) >= len(c["C"])
    contigs, cn, base = tx.lay_out([r[6] for r in Cr]); ix = gm.Index(contigs, params=gm.default_params_cs())
    gm.sw_vector_setup(*vector_args(c["setup"], True))
    goff, glen, rlen, initbp, want = (np.array([r[k] for r in Cr], dtype=np.int64) for k in (1, 2, 3, 4, 8))
    got = ix.sw_vector_batch(cn, np.zeros(len(Cr), dtype=np.uint8), base + goff, glen, reads_matrix([r[7] for r in Cr], rlen), rlen, initbp=initbp)
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:10])
    ix.close()
    gm.sw_full_cs_setup(*full_cs_args(c["setup"]))
    for kind, local in (("S", False), ("L", True), ("X", False), ("Y", True)):
        its = c[kind]
        contigs, cn, base = tx.lay_out([it["g"] for it in its]); ix = gm.Index(contigs, params=gm.default_params_cs()); a = tx.arrays(its)
        recs, ops, strings = ix.sw_full_cs_batch(cn, np.zeros(len(its), dtype=np.uint8), base + a["goff"], a["glen"], a["reads"], a["rlen"], a["initbp"], a["anchors"], a["rv"],
                                                 a["thresh"], xover=a["xs"], is_rna=0, local_alignment=local)
        strings.prefetch()
        check_cs(its, recs, strings, base)
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["large", "swapped"])
def test_vector_multi_stripe_against_the_oracle(gm, name):
    """reads of more than 128 rows at the set: 64 windows each at read lengths 129, 256, 257, 300 and 1 000, on windows of 200 columns (the stripe carry in registers)
    and of 1.4 x the read (beyond 256 columns: the carry rows in LDS); 4 % substitutions, an insertion or a deletion in half of the reads.  One call."""
    from shrimp_amd import synth
    rng = np.random.default_rng(73)
    G = rng.integers(0, 4, size=200_000, dtype=np.uint8)
    starts, glens, rlens, reads = [], [], [], []
    for L in (129, 256, 257, 300, 1000):
        for W in (200, int(1.4 * L)):
            for i in range(64):
                s = int(rng.integers(0, G.size - 3000)); off = max(0, (W - L) // 2)
                rd = G[s + off:s + off + L].copy()
                if i % 8: rd = np.where(rng.random(L) < 0.04, rng.integers(0, 4, size=L), rd).astype(np.uint8)      # (every eighth read is an exact copy)
                if i % 2:
                    p = int(rng.integers(10, L - 10))
                    rd = np.concatenate([rd[:p], rd[p + 1:], rd[-1:]]) if i % 4 == 1 else np.concatenate([rd[:p], rd[p - 1:p], rd[p:-1]])
                starts.append(s); glens.append(W); rlens.append(L); reads.append(synth.pack_nibbles(rd))
    gw = synth.pack_nibbles(G); rw = reads_matrix(reads, rlens)
    setup = ls_set(name)["setup"]
    want = oa.sw_vector_batch_p(oa.score_array(setup), gw, starts, glens, rw, rlens)
    gm.sw_vector_setup(*vector_args(setup, False))
    got = gm.sw_vector_batch(gw, starts, glens, rw, rlens)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]], np.asarray(glens)[bad[:10]], np.asarray(rlens)[bad[:10]])
    if name == "large": assert want.max() == 32000                 # an exact copy of 1 000 bases: the largest score the setup allows


@pytest.mark.gpu
@pytest.mark.parametrize("L", [100, 150])
@pytest.mark.parametrize("name", EARLY_SETS)
def test_early_stop_is_exact_about_the_threshold_at_the_set(gm, name, L):
    """the property of test_sw_vector_early_stop_is_exact_about_the_threshold at the set: every stopped window's full score is below the threshold and its returned
    value a lower bound of it, every other window returns the full score; thresholds 0.3, 0.47 and 0.7 of match x L"""
    e = early_inputs(L); n = EARLY_N
    gm.sw_vector_setup(*vector_args(ls_set(name)["setup"], False))
    full = gm.sw_vector_batch(e["gw"], e["starts"], e["glen"], e["rw"], e["rlen"])
    assert np.array_equal(full, early_full(name, L))
    lo, mid, hi = early_thresholds(name, L)
    n_stopped = 0
    for thr in (mid, lo, hi):
        got, stopped = gm.sw_vector_batch_bounded(e["gw"], e["starts"], e["glen"], e["rw"], e["rlen"], thr)
        st = stopped.astype(bool)
        print("early stop %s L=%d thr=%d: %d stopped, %d at or above" % (name, L, thr, int(st.sum()), int((full >= thr).sum())))
        assert (got[~st] == full[~st]).all()
        assert (full[st] < thr).all(), np.nonzero(st & (full >= thr))[0][:10]
        assert (got[st] <= full[st]).all() and (got[st] >= 0).all()
        assert ((full >= thr) <= ~st).all()
        n_stopped += int(st.sum())
        if thr == mid: assert st.sum() > n // 5 and (full >= thr).sum() > n // 5      # both outcomes are well represented
    assert n_stopped > 0


@pytest.mark.gpu
def test_score_windows_on_hand_made_windows_at_a_set(gm):
    """gm_score_windows (pass 1's scoring kernel) under the set "swapped", on both strands, as tests/test_pass1_seam.py does at the defaults: windows at offset 0, ending
    at the contig's last base, shorter than the read, over every letter code; read lengths around the 64-lane step and beyond 128"""
    from tests import test_select as ts
    from tests.test_pass1_seam import hand_genome, hand_windows
    setup = ls_set("swapped")["setup"]; sc = oa.score_array(setup)
    contigs = hand_genome(); c0 = contigs[0]
    p = gm.default_params()
    p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score = setup[2:8]
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p, max_batch_reads=1024)
    O = oa.load(); packed = [ts.pack(c) for c in contigs]; rng = np.random.default_rng(6)
    for L in (63, 65, 129, 300):
        W = int(1.4 * L)
        r0 = c0[200:200 + L].copy(); r0[rng.integers(0, L, 3)] ^= 1
        r0 = np.concatenate([r0[:L // 2], r0[L // 2 + 2:], r0[-2:]])                 # two bases missing from the read: the cheap gap of this set
        r1 = ts.CMPL[c0[300:300 + L][::-1]].copy(); r1 = np.concatenate([r1[:L // 3], r1[L // 3 - 1:-1]])      # one base twice: the dear one
        reads = np.stack([r0, r1])
        wl = [(0, 0, W), (0, 95, W), (0, 190, W), (0, 290, W), (0, 205, max(1, L - 3)), (0, len(c0) - W, W), (0, len(c0) - 5, 5), (2, 0, W)]
        rows, off = hand_windows([wl] * 4)
        scores, slots = s.score_windows(reads, ts.as_wins(gm, rows), off)
        want = np.zeros(len(rows), dtype=np.int32)
        for i, r in enumerate(rows):
            rd, st, cn, g_off, w_len = (int(x) for x in r[:5])
            q = reads[rd] if st == 0 else ts.CMPL[reads[rd][::-1]]
            want[i] = O.gmo_sw_vector_p(sc, ts._u32(packed[cn]), g_off, w_len, ts._u32(ts.pack(q)), L)
        assert np.array_equal(scores, want), (L, rows[scores != want][:5], scores[scores != want][:5], want[scores != want][:5])
        assert want.max() >= 10 * L - 3 * 25 - 45 - 2 * 9
    s.close(); ix.close()


# ---- the production colour-space pass 2: both implementations at every colour-space score case ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"GM_P2_G": "16"}, {"GM_P2_G4": "0"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
@pytest.mark.parametrize("tag", ["cs_scores_swapped", "cs_gate_under", "cs_gate_over"])
def test_colour_space_score_cases_under_the_other_pass2_kernels(gm, tag, env):
    """gm_launch_pass2_cs takes k_pass2_cs_g4<8, int16_t> for cs_scores_swapped and cs_gate_under and k_pass2_cs_g4<16, int> for cs_gate_over (the cases' comments in
    tests/oracle_api.py; test_colour_space_local_and_ungapped_match_reference_golden runs them so).  Here the int kernel (GM_P2_G=16) and the one-window kernel
    (GM_P2_G4=0) take all three: every implementation meets every set whichever side of the gate it lies on."""
    import os
    base, _, fields, _ = oa.CS_OPTION_CASES[tag]
    contigs, reads, _ = oa.load_golden(base)
    want = oa.load_option_sam(base, tag)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        p = gm.default_params_cs()
        for k, v in fields.items(): setattr(p, k, v)
        ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p, max_batch_reads=1024)
        got = oa.sam_header(contigs) + s.map_reads_cs(reads)
        s.close(); ix.close()
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    assert got == want


# ---- the reference's own (mangled) names at a set --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mangled_seams_replay_the_steep_set(gm, tmp_path):
    """tests/seam_driver.cpp (a C++ caller through the names the reference's objects ask for) with the set's scores in its setup requests: every V, F, C, S, L, X and Y
    record of "steep" (the driver's L request is the colour-space one)"""
    import subprocess
    from tests.test_gpu_parity import _seam_driver, _hexw
    exe = _seam_driver(tmp_path)
    ls, cs = ls_set("steep"), cs_set("steep")
    a = ls["setup"]; c = cs["setup"]
    req = ["setup_v 0 %d %d %d %d %d %d" % (a[7], a[2], a[3], a[4], a[5], a[6]), "setup_f_ls %d %d %d %d %d %d" % a[2:8]]
    want = []
    for _, goff, glen, rlen, g, r, score in ls["V"]:
        req.append("V %d %d %d %s %s" % (goff, glen, rlen, _hexw(g), _hexw(r))); want.append("V %d" % score)
    for it in ls["F"]:
        req.append("F %d %d %d %d %d %d %d %d %s %s" % ((it["goff"], it["glen"], it["rlen"]) + tuple(it["anchor"]) + (int(it["rv"]), _hexw(it["g"]), _hexw(it["r"]))))
        want.append("F " + " ".join(str(x) for x in it["want"]) + " %s %s" % (it["db"], it["qr"]))
    req += ["setup_v 1 %d %d %d %d %d %d" % (c[6] + c[8], c[2], c[3], c[4], c[5], c[6]), "setup_f_cs %d %d %d %d %d %d %d %d" % c[2:10]]
    for _, goff, glen, rlen, initbp, gcs, gls, rd, score in cs["C"]:
        req.append("C %d %d %d %d %s %s %s" % (goff, glen, rlen, initbp, _hexw(gcs), _hexw(gls), _hexw(rd))); want.append("C %d" % score)
    for kind in "SLXY":
        for it in cs[kind]:
            t = "%s %d %d %d %d %d %d %d %d %d %d %s %s" % ((kind, it["goff"], it["glen"], it["rlen"], it["initbp"]) + tuple(it["anchor"]) + (int(it["rv"]), it["thresh"], _hexw(it["g"]), _hexw(it["r"])))
            if it["xs"] is not None: t += " " + ",".join(str(int(x)) for x in it["xs"])
            req.append(t)
            want.append(kind + " " + " ".join(str(x) for x in it["want"]) + " %s %s" % (it["db"] or "-", it["qr"] or "-") if it["want"][0] != 0 else None)      # score 0: nothing else is defined
    assert len(want) >= 1200
    p = subprocess.run([exe], input=("\n".join(req) + "\n").encode(), capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.decode().split("\n")
    assert len(got) == len(want) + 1 and got[-1] == ""
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None: assert g.split()[1] == "0", (k, g)
        else: assert g == w, (k, g, w)
