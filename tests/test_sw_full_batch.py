"""gm_sw_full_ls_batch / gm_sw_full_cs_batch: the batch forms of the full-alignment seams, against the reference's own known answers
(tests/golden/sw_kat*.txt.gz), the CPU oracle beyond the fixtures' shapes, and the single seams.  The host-only string rebuild is checked without a GPU."""
import ctypes as C
import os, subprocess, sys, threading
import numpy as np
import pytest
from tests import oracle_api as oa

LS_SETUP = (1400, 1000, -33, -7, -33, -3, 10, -15, True, 8)                 # the setups of the single-seam known-answer tests
CS_SETUP = (1400, 1000, -33, -7, -33, -3, 10, -24, -20, True, 8, 0)
LS_FIELDS = ("score", "read_start", "rmapped", "genome_start", "gmapped", "matches", "mismatches", "insertions", "deletions")
CS_FIELDS = LS_FIELDS + ("crossovers",)
LSTRANS = "ACGTUMRWSYKVHDBN"
CS_KINDS = {"sw_kat_cs.txt.gz": "S", "sw_kat_cs_local.txt.gz": "L", "sw_kat_cs_xover.txt.gz": "XY", "sw_kat_cs_rna.txt.gz": "SL"}      # the full-SW record kinds of each colour-space fixture
_s = lambda x: x.decode() if isinstance(x, bytes) else x


# ---- the fixtures as item lists: dict(g, goff, glen, r, rlen, anchor (x, y, length, width) or None, rv, thresh, maxscore, initbp, xs, want, db, qr) ----
def _item(g, goff, glen, r, rlen, anchor, rv, thresh=0, maxscore=0, initbp=0, xs=None, want=None, db="", qr=""):
    return dict(g=g, goff=goff, glen=glen, r=r, rlen=rlen, anchor=anchor, rv=rv, thresh=thresh, maxscore=maxscore, initbp=initbp, xs=xs, want=list(want), db=_s(db), qr=_s(qr))


_cache = {}


def items_F():
    if "F" not in _cache:
        _cache["F"] = [_item(rec[9], rec[1], rec[2], rec[10], rec[3], tuple(rec[4:8]), rec[8], want=rec[11], db=rec[12], qr=rec[13]) for rec in oa.load_kat() if rec[0] == "F"]
    return _cache["F"]


def items_local():
    return [_item(g, goff, glen, r, rlen, None if no_anchor else (ax, ay, alen, aw), rv, thresh, sv, want=want, db=db, qr=qr)
            for (goff, glen, rlen, ax, ay, alen, aw, rv, no_anchor, thresh, sv), g, r, want, db, qr in oa.load_kat_local()]


def items_cs(name, kinds):
    out = []
    for rec in oa.load_kat_cs(name):
        if rec[0] not in kinds: continue
        (goff, glen, rlen, initbp, ax, ay, alen, aw, rv, thresh), gls, rd, want, db, qr = rec[1:7]
        out.append(_item(gls, goff, glen, rd, rlen, (ax, ay, alen, aw), rv, thresh, initbp=initbp, xs=rec[7] if len(rec) > 7 else None, want=want, db=db, qr=qr))
    return out


def pack(items):
    """the items' genome bitfields laid end to end (each starts on a word boundary, as test_sw_vector_known_answers does), reads padded to one width"""
    base, bases, words = 0, [], []
    for it in items:
        bases.append(base * 8); words.append(it["g"]); base += len(it["g"])
    rw = max(max(len(it["r"]) for it in items), max((it["rlen"] + 7) // 8 for it in items))
    reads = np.zeros((len(items), rw), dtype=np.uint32)
    for i, it in enumerate(items): reads[i, :len(it["r"])] = it["r"]
    anchors = np.array([it["anchor"] if it["anchor"] is not None else (0, 0, 0, 0) for it in items], dtype=np.int64)
    d = dict(genome=np.concatenate(words), bases=np.array(bases, dtype=np.int64), reads=reads, anchors=anchors)
    d["g_off"] = d["bases"] + np.array([it["goff"] for it in items], dtype=np.int64)
    for k in ("glen", "rlen", "rv", "thresh", "maxscore", "initbp"): d[k] = np.array([it[k] for it in items], dtype=np.int64)
    if any(it["xs"] is not None for it in items):
        d["xs"] = np.zeros((len(items), max(it["rlen"] for it in items)), dtype=np.int32)
        for i, it in enumerate(items): d["xs"][i, :it["rlen"]] = it["xs"][:it["rlen"]]
    else: d["xs"] = None
    return d


def run_ls(gm, items, local=False, order=None):
    p = pack(items)
    o = np.arange(len(items)) if order is None else np.asarray(order)
    recs, ops, strings = gm.sw_full_ls_batch(p["genome"], p["g_off"][o], p["glen"][o], p["reads"][o], p["rlen"][o], p["anchors"][o], p["rv"][o], p["thresh"][o], p["maxscore"][o],
                                             local_alignment=local)
    return recs, ops, strings, p["bases"][o]


def run_cs(gm, items, local=False, is_rna=False):
    p = pack(items)
    recs, ops, strings = gm.sw_full_cs_batch(p["genome"], p["g_off"], p["glen"], p["reads"], p["rlen"], p["initbp"], p["anchors"], p["rv"], p["thresh"], xover=p["xs"],
                                             is_rna=is_rna, local_alignment=local)
    return recs, ops, strings, p["bases"]


def check_ls(items, recs, strings, bases, order=None):
    """all nine integer fields (genome_start less the item's base) and both strings, every item"""
    assert len(recs) == len(bases)
    for k in range(len(recs)):
        it = items[k if order is None else order[k]]; R = recs[k]
        assert R["status"] == 0, (k, R)
        got = [int(R[f]) for f in LS_FIELDS]; got[3] -= int(bases[k])
        assert got == it["want"], (k, got, it["want"])
        assert strings(k) == (it["db"], it["qr"]), (k, strings(k), it["db"], it["qr"])


def check_cs(items, recs, strings, bases):
    for k, it in enumerate(items):
        R = recs[k]
        assert R["status"] == 0, (k, R)
        if it["want"][0] == 0:                                   # below the threshold: the reference answers score 0 and no strings
            assert R["score"] == 0 and R["n_ops"] == 0 and strings(k) == (None, None), (k, R)
            continue
        got = [int(R[f]) for f in CS_FIELDS]; got[3] -= int(bases[k])
        assert got == it["want"], (k, got, it["want"])
        assert strings(k) == (it["db"], it["qr"]), (k, strings(k), it["db"], it["qr"])


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


# ---- 1 / 2: the reference's known answers, each whole set in one call ------------------------------------------------------------------
@pytest.mark.gpu
def test_ls_global_every_F_record_in_one_call(gm):
    items = items_F()
    assert len(items) >= 2990
    gm.sw_full_ls_setup(*LS_SETUP)
    recs, ops, strings, bases = run_ls(gm, items)
    check_ls(items, recs, strings, bases)
    assert int(recs["n_ops"].sum()) == ops.size and (recs["crossovers"] == 0).all()        # the ops buffer is compact
    inv, cells, secs = gm.seam_stats("sw_full_ls")
    assert inv == len(items) and cells > 0 and secs > 0


@pytest.mark.gpu
def test_ls_local_fixture_in_one_call(gm):
    items = items_local()
    assert len(items) >= 500 and any(it["anchor"] is None for it in items) and any(it["anchor"] is not None for it in items)
    gm.sw_full_ls_setup(*LS_SETUP)
    recs, ops, strings, bases = run_ls(gm, items, local=True)
    check_ls(items, recs, strings, bases)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kinds,local,rna,at_least", [
    ("sw_kat_cs.txt.gz", "S", False, False, 1400),
    ("sw_kat_cs_local.txt.gz", "L", True, False, 800),
    ("sw_kat_cs_xover.txt.gz", "X", False, False, 1000),          # per-position crossover rows, global
    ("sw_kat_cs_xover.txt.gz", "Y", True, False, 500),            # ... and local
    ("sw_kat_cs_rna.txt.gz", "S", False, True, 1),
    ("sw_kat_cs_rna.txt.gz", "L", True, True, 1),
])
def test_cs_fixture_in_one_call(gm, name, kinds, local, rna, at_least):
    items = items_cs(name, kinds)
    assert len(items) >= at_least
    # no full-SW record of the fixture is left out: the cases of this test take every kind the file holds (its "C" records are the vector filter's)
    assert {r[0] for r in oa.load_kat_cs(name)} - {"C"} == set(CS_KINDS[name]) and kinds in CS_KINDS[name]
    if kinds in "XY": assert all(it["xs"] is not None for it in items)
    gm.sw_full_cs_setup(*CS_SETUP)
    recs, ops, strings, bases = run_cs(gm, items, local=local, is_rna=rna)
    check_cs(items, recs, strings, bases)
    assert any(it["want"][0] > 0 for it in items)


# ---- 3: a wave's scratch is reused by items of every shape ------------------------------------------------------------------------------
def _is_tuning_build(gm):
    return "release" not in os.path.basename(gm.LIB_PATH)


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [0, 3])
def test_ls_slot_reuse_shuffled_triple(gm, slots, monkeypatch):
    """the F records three times over in a shuffled order: 8 970 items, more than the largest grid, so every wave takes items of several shapes through its one
    scratch.  slots = 3 (the tuning build's GM_SWF_SLOTS): three waves take them all, a 1-row item behind the largest.  The release build reads no knob: there the
    second case repeats the first."""
    items = items_F()
    order = np.random.default_rng(20261018).permutation(np.tile(np.arange(len(items)), 3))
    assert order.size > 2048 * 4
    if slots: monkeypatch.setenv("GM_SWF_SLOTS", str(slots))
    gm.sw_full_ls_setup(*LS_SETUP)
    recs, ops, strings, bases = run_ls(gm, items, order=order)
    check_ls(items, recs, strings, bases, order=order)


@pytest.mark.gpu
def test_cs_slot_reuse_few_slots(gm, monkeypatch):
    """colour space: the single call clears its scratch, the batch kernel must not need that -- global and local, the fixture's records three times over in reversed
    order: 4 200 and 2 400 items, more than the largest grid (2 048), so every wave reuses its scratch in any build; two slots for them all in the tuning build"""
    monkeypatch.setenv("GM_SWF_SLOTS", "2")
    gm.sw_full_cs_setup(*CS_SETUP)
    for name, kinds, local in (("sw_kat_cs.txt.gz", "S", False), ("sw_kat_cs_local.txt.gz", "L", True)):
        items = items_cs(name, kinds)[::-1] * 3
        assert len(items) > 2048
        recs, ops, strings, bases = run_cs(gm, items, local=local)
        check_cs(items, recs, strings, bases)


# ---- 4: beyond the fixtures' shapes, against the CPU oracle -----------------------------------------------------------------------------
def _nib_pack(codes):
    from shrimp_amd import synth
    return synth.pack_nibbles(np.asarray(codes, dtype=np.uint8))


def _oracle_items(rlen, glen, n, seed, colour):
    """n windows of glen with a read of rlen cut from them (substitutions, one insertion or deletion in half of them), an anchor box on the read's diagonal"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        goff = int(rng.integers(0, 8))
        G = rng.integers(0, 4, size=goff + glen + 8, dtype=np.uint8)
        off = max(0, (glen - rlen) // 2)
        src = G[goff + off:goff + glen]
        rd = np.resize(src, rlen).copy() if len(src) >= rlen else np.concatenate([src, rng.integers(0, 4, size=rlen - len(src), dtype=np.uint8)])
        if i % 4:                                                   # every fourth read is an exact copy
            m = rng.random(rlen) < 0.04; rd = np.where(m, rng.integers(0, 4, size=rlen), rd).astype(np.uint8)
        if i % 2 and rlen > 12:
            p = int(rng.integers(4, rlen - 4))
            rd = np.concatenate([rd[:p], rd[p + 1:], rd[-1:]]) if i % 4 == 1 else np.concatenate([rd[:p], rd[p - 1:p], rd[p:-1]])
        initbp = int(rng.integers(0, 4))
        if colour:                                                  # the read as colours behind the primer letter
            prev = np.concatenate([[initbp], rd[:-1]]); rd = (prev ^ rd).astype(np.uint8)
        p0 = int(rng.integers(0, max(1, min(rlen, glen - off) - 12)))
        anchor = (off + p0, p0, int(min(12, rlen)), 1 + i % 3)
        out.append(dict(g=_nib_pack(G), goff=goff, glen=glen, r=_nib_pack(rd), rlen=rlen, anchor=anchor, rv=i % 3 == 1, thresh=rlen * 10 * 3 // 10, maxscore=rlen * 10,
                        initbp=initbp, xs=None, want=None, db="", qr=""))
    return out


def _oracle_fill(L, items, mode):
    """the oracle's answer for every item (its seam functions keep no state between calls and ctypes drops the GIL: eight at a time)"""
    from concurrent.futures import ThreadPoolExecutor
    u32p = C.POINTER(C.c_uint32)
    def one(it):
        out = (C.c_int * 10)(); db = C.create_string_buffer(8192); qr = C.create_string_buffer(8192)
        g, r = np.ascontiguousarray(it["g"]), np.ascontiguousarray(it["r"])
        a = it["anchor"] if it["anchor"] is not None else (0, 0, 1, 1)
        if mode == "ls":
            rc = L.gmo_sw_full_ls(g.ctypes.data_as(u32p), it["goff"], it["glen"], r.ctypes.data_as(u32p), it["rlen"], a[0], a[1], a[2], a[3], int(it["rv"]), out, db, qr, 8192)
        elif mode == "ls_local":
            rc = L.gmo_sw_full_ls_local(g.ctypes.data_as(u32p), it["goff"], it["glen"], r.ctypes.data_as(u32p), it["rlen"], it["thresh"], it["maxscore"], a[0], a[1], a[2], a[3],
                                        0 if it["anchor"] is None else 1, int(it["rv"]), out, db, qr, 8192)
        else:
            rc = L.gmo_sw_full_cs(g.ctypes.data_as(u32p), it["goff"], it["glen"], r.ctypes.data_as(u32p), it["rlen"], it["initbp"], it["thresh"], a[0], a[1], a[2], a[3],
                                  int(it["rv"]), out, db, qr, 8192)
        assert rc == 0
        it["want"] = list(out)[:10 if mode == "cs" else 9]; it["db"] = db.value.decode(); it["qr"] = qr.value.decode()
    with ThreadPoolExecutor(8) as ex: list(ex.map(one, items))


SHAPES = [(300, 420), (1000, 1400), (20, 28), (40, 30)]              # read x window: mid, the setup's limits, tiny, window shorter than the read


@pytest.mark.gpu
@pytest.mark.parametrize("rlen,glen", SHAPES)
def test_against_the_cpu_oracle(gm, oracle_lib, rlen, glen):
    """64 items of one shape per entry and mode (revcmpl mixed 0/1; local letter space: anchored and unanchored mixed in the call) plus, in the same call, eight items of
    the tiny shape in front and behind, so that a wave's scratch and LDS serve two shapes"""
    small = (20, 28)
    def mixed(seed, colour):
        return _oracle_items(small[0], small[1], 8, seed + 1, colour) + _oracle_items(rlen, glen, 64, seed, colour) + _oracle_items(small[0], small[1], 8, seed + 2, colour)
    gm.sw_full_ls_setup(*LS_SETUP)
    items = mixed(rlen * 7, False); _oracle_fill(oracle_lib, items, "ls")
    recs, ops, strings, bases = run_ls(gm, items)
    check_ls(items, recs, strings, bases)
    assert any(it["want"][0] > 0 and ("-" in it["db"] or "-" in it["qr"]) for it in items)
    items = mixed(rlen * 7 + 3, False)
    u32p = C.POINTER(C.c_uint32)
    for i, it in enumerate(items):
        if i % 3 == 0: it["anchor"] = None                        # the threshold band for this item
        # maxscore is the vector filter's score of the window, as gmapper passes it (the second run is taken when the anchor band misses it, and must then reach it:
        # the reference asserts so), and a window below the threshold is never handed to sw_full_ls
        it["maxscore"] = int(oracle_lib.gmo_sw_vector(it["g"].ctypes.data_as(u32p), it["goff"], it["glen"], it["r"].ctypes.data_as(u32p), it["rlen"]))
        it["thresh"] = min(it["thresh"], it["maxscore"])
    _oracle_fill(oracle_lib, items, "ls_local")
    recs, ops, strings, bases = run_ls(gm, items, local=True)
    check_ls(items, recs, strings, bases)
    gm.sw_full_cs_setup(*CS_SETUP)
    items = mixed(rlen * 7 + 5, True); _oracle_fill(oracle_lib, items, "cs")
    recs, ops, strings, bases = run_cs(gm, items)
    check_cs(items, recs, strings, bases)
    assert sum(it["want"][0] > 0 for it in items) >= 40


# ---- 5: edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_edges_empty_one_and_not_set_up(gm, oracle_lib):
    gm.sw_full_ls_setup(*LS_SETUP); gm.sw_full_cs_setup(*CS_SETUP)
    L = gm.lib()
    z32 = np.zeros(1, dtype=np.uint32)
    recs, ops, _ = gm.sw_full_ls_batch(z32, [], [], np.zeros((0, 1), dtype=np.uint32), [])                    # n = 0
    assert len(recs) == 0 and ops.size == 0
    recs, ops, _ = gm.sw_full_cs_batch(z32, [], [], np.zeros((0, 1), dtype=np.uint32), [], [], np.zeros((0, 4)))
    assert len(recs) == 0 and ops.size == 0
    it = items_F()[7]                                                                                      # n = 1 == the single seam
    f, db, qr = gm.sw_full_ls(it["g"], it["goff"], it["glen"], it["r"], it["rlen"], it["anchor"], revcmpl=bool(it["rv"]))
    recs, ops, strings, bases = run_ls(gm, [it])
    got = {k: int(recs[0][k]) for k in LS_FIELDS}
    assert got == f and strings(0) == (db, qr) and f["score"] > 0
    io = dict(it); _oracle_fill(oracle_lib, [io], "ls")                                                    # both sides run one kernel: the CPU oracle is the independent one
    check_ls([io], recs, strings, bases)
    ic = next(i for i in items_cs("sw_kat_cs.txt.gz", "S") if i["want"][0] > 0)
    f, db, qr = gm.sw_full_cs(ic["g"], ic["goff"], ic["glen"], ic["r"], ic["rlen"], ic["initbp"], ic["thresh"], ic["anchor"], revcmpl=bool(ic["rv"]))
    recs, ops, strings, bases = run_cs(gm, [ic])
    assert {k: int(recs[0][k]) for k in CS_FIELDS} == f and strings(0) == (db, qr)
    io = dict(ic); _oracle_fill(oracle_lib, [io], "cs")
    assert io["want"][0] > 0
    check_cs([io], recs, strings, bases)
    res = {}                                                                                               # the setup state is per thread: a new thread has none
    def fresh():
        rec = np.zeros(1, dtype=gm.SW_FULL_REC_DTYPE); p = C.c_void_p(); ln = C.c_uint64(0)
        one = np.ones(1, dtype=np.int32); off = np.zeros(1, dtype=np.int64); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        u = z32.ctypes.data_as(C.POINTER(C.c_uint32))
        res["ls"] = L.gm_sw_full_ls_batch(1, u, 1, off.ctypes.data_as(C.POINTER(C.c_int64)), ip(one), u, 1, ip(one), None, None, ip(one), None, 0, rec.ctypes.data, C.byref(p), C.byref(ln))
        res["cs"] = L.gm_sw_full_cs_batch(1, u, 1, off.ctypes.data_as(C.POINTER(C.c_int64)), ip(one), u, 1, ip(one), None, None, None, ip(one), None, 0, 0, 0, rec.ctypes.data,
                                          C.byref(p), C.byref(ln))
        res["msg"] = L.gm_last_error()
    t = threading.Thread(target=fresh); t.start(); t.join()
    assert res["ls"] == -3 and res["cs"] == -3 and b"setup" in res["msg"]                                  # GM_E_NOTSETUP


@pytest.mark.gpu
def test_single_ls_seam_takes_a_window_beyond_64_kb_of_lds(gm, oracle_lib):
    """sw_full_ls is a batch call of one item, so it takes what the batch entry takes: a window of 5 400 needs 70 KB of LDS (12 bytes a column), more than a launch gets
    without asking.  Fields and strings against the CPU oracle, anchored, both strand rules."""
    gm.sw_full_ls_setup(6000, 1000, *LS_SETUP[2:])
    items = _oracle_items(100, 5400, 3, 77, False); _oracle_fill(oracle_lib, items, "ls")
    for it in items:
        f, db, qr = gm.sw_full_ls(it["g"], it["goff"], it["glen"], it["r"], it["rlen"], it["anchor"], revcmpl=bool(it["rv"]))
        assert [f[k] for k in LS_FIELDS] == it["want"] and (db, qr) == (it["db"], it["qr"]), (f, it["want"], db, it["db"])
    assert all(it["want"][0] > 0 for it in items)
    gm.sw_full_ls_setup(*LS_SETUP)


@pytest.mark.gpu
def test_cs_item_beyond_the_lds_limit_is_refused_alone(gm, oracle_lib):
    """48 bytes of LDS a window column: a window of 3 500 needs more than a work-group has.  In the middle of a call it comes back refused, its neighbours answered;
    so does a per-position crossover score outside 8 bits.  LDS is laid out for the longest window AND the longest read of a launch: a window of 3 300 with a
    10-colour read fits alone (161 856 bytes of 163 840) but not beside a 1 000-colour read of another item (166 816) -- it is refused, the long read is answered."""
    gm.sw_full_cs_setup(4000, 1000, *CS_SETUP[2:])
    items = [i for i in items_cs("sw_kat_cs_xover.txt.gz", "X")[:40]]
    big = _oracle_items(100, 3500, 1, 5, True)[0]; big["xs"] = np.full(100, -20, dtype=np.int32)
    bad = dict(items[3]); bad["xs"] = items[3]["xs"].copy(); bad["xs"][0] = -1000
    call = items[:20] + [big] + items[20:30] + [bad] + items[30:]
    recs, ops, strings, bases = run_cs(gm, call)
    msg = gm.lib().gm_last_error()
    assert recs[20]["status"] == -2 and recs[20]["score"] == 0 and recs[20]["n_ops"] == 0                  # GM_E_ARG
    assert recs[31]["status"] == -4 and recs[31]["score"] == 0 and b"crossover score outside" in msg       # GM_E_RANGE; the last refusal's reason
    keep = [k for k in range(len(call)) if k not in (20, 31)]
    check_cs([call[k] for k in keep], recs[keep], lambda j: strings(keep[j]), bases[keep])
    inv0 = gm.seam_stats("sw_full_cs")[0]
    wide = _oracle_items(10, 3300, 1, 6, True)[0]; long_read = _oracle_items(1000, 1400, 1, 7, True)     # (no crossover rows in this call)
    small = _oracle_items(20, 28, 4, 8, True); _oracle_fill(oracle_lib, long_read + small, "cs")
    call = small[:2] + [wide] + long_read + small[2:]
    recs, ops, strings, bases = run_cs(gm, call)
    assert recs[2]["status"] == -2 and recs[2]["score"] == 0 and b"LDS" in gm.lib().gm_last_error()
    keep = [0, 1, 3, 4, 5]
    check_cs([call[k] for k in keep], recs[keep], lambda j: strings(keep[j]), bases[keep])
    assert call[3]["want"][0] > 0
    assert gm.seam_stats("sw_full_cs")[0] == inv0 + 5                                                      # a refused item is no invocation
    recs, ops, strings, bases = run_cs(gm, [wide])                                                         # alone it fits, and is answered
    assert recs[0]["status"] == 0
    gm.sw_full_cs_setup(*CS_SETUP)


def test_record_mirror_has_the_library_size():
    from shrimp_amd import gmapper as gm
    L = gm.lib()
    assert L.gm_abi_sizeof(4) == C.sizeof(gm.SwFullRec) == gm.SW_FULL_REC_DTYPE.itemsize == 64
    assert gm.ANCHOR_DTYPE.itemsize == C.sizeof(gm.Anchor)


# ---- 6: the host-only string rebuild, no GPU --------------------------------------------------------------------------------------------
def _rec_of(gm, it, n_ops, colour):
    rec = np.zeros(1, dtype=gm.SW_FULL_REC_DTYPE)
    for k, v in zip(CS_FIELDS if colour else LS_FIELDS, it["want"]): rec[k] = v
    rec["ops_off"] = 5; rec["n_ops"] = n_ops                       # (behind five bytes of another item's)
    return rec


def _nib(words, i): return int((int(words[i // 8]) >> (4 * (i % 8))) & 15)


def test_strings_rebuilt_from_fixture_alignments_letter_space():
    from shrimp_amd import gmapper as gm
    n = 0
    for it in items_F():
        if it["want"][0] <= 0: continue
        ops = bytes(ord("D") if d == "-" else ord("I") if q == "-" else ord("M") for d, q in zip(it["db"], it["qr"]))
        rec = _rec_of(gm, it, len(ops), False)
        assert gm.sw_full_batch_strings(False, rec, np.frombuffer(b"MMMMM" + ops, dtype=np.uint8), it["g"], it["r"]) == (it["db"], it["qr"])
        n += 1
    assert n >= 2900
    rec = np.zeros(1, dtype=gm.SW_FULL_REC_DTYPE)                 # no alignment: two empty strings, as sw_full_ls
    assert gm.sw_full_batch_strings(False, rec, np.zeros(0, dtype=np.uint8), it["g"], it["r"]) == ("", "")


@pytest.mark.parametrize("name,kinds,rna", [("sw_kat_cs.txt.gz", "S", False), ("sw_kat_cs_local.txt.gz", "L", False), ("sw_kat_cs_rna.txt.gz", "SL", True)])
def test_strings_rebuilt_from_fixture_alignments_colour_space(name, kinds, rna):
    from shrimp_amd import gmapper as gm
    n = 0
    for it in items_cs(name, kinds):
        if it["want"][0] <= 0: continue
        # the four letter translations of the colour read (ref: sw-full-cs.c:1182-1197), to find the layer a printed read letter came from
        tr = []
        for k in range(4):
            letter = (k + it["initbp"]) % 4; row = []
            for j in range(it["rlen"]):
                base = _nib(it["r"], j)
                if base == 15: row.append(15); letter = (k + it["initbp"]) % 4; continue
                lt = 3 if (rna and letter == 4) else letter
                l2 = 15 if (letter == 15 or base > 3) else ((4 + lt + base) % 4 if lt % 2 == 0 else (4 + lt - base) % 4)
                if rna and l2 == 3: l2 = 4
                row.append(l2); letter = l2
            tr.append(row)
        ops, pi, pj = [], it["want"][1], it["want"][3]
        for d, q in zip(it["db"], it["qr"]):
            if q == "-": ops.append(1); pj += 1; continue
            x = 0x80 if q.islower() else 0
            shown = [LSTRANS[tr[k][pi]] for k in range(4)]
            if d != "-" and all(s == "N" for s in shown): lay = 0       # an N in the read prints the genome letter whatever the layer
            else: lay = shown.index(q.upper())
            ops.append((2 if d == "-" else 6) + lay | x); pi += 1; pj += d != "-"
        rec = _rec_of(gm, it, len(ops), True)
        got = gm.sw_full_batch_strings(True, rec, np.array([9] * 5 + ops, dtype=np.uint8), it["g"], it["r"], it["initbp"], rna)
        assert got == (it["db"], it["qr"]), (n, got, it["db"], it["qr"])
        n += 1
    assert n >= 500
    rec = np.zeros(1, dtype=gm.SW_FULL_REC_DTYPE)                 # no alignment: no strings, as sw_full_cs
    assert gm.sw_full_batch_strings(True, rec, np.zeros(0, dtype=np.uint8), it["g"], it["r"], 0, rna) == (None, None)


# ---- the release build (no tuning knobs compiled in) -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_release_build_passes_the_fixture_and_reuse_tests(gm):
    """the fixture, slot-reuse and edge tests of this file once more in a child interpreter on libgmapper_hip_release.so (what the existing goldens do for the read paths)"""
    if not _is_tuning_build(gm): return                           # (this IS the child)
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    sel = "in_one_call or slot_reuse or edges or lds_limit"
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=dict(os.environ, GM_LIB_PATH=rel), cwd=oa.ROOT, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    import re
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) >= 13, p.stdout[-500:]
