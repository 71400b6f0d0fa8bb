"""gm_post_sw_batch: the batch form of post_sw (S3) -- the colour-space posteriors of every record of one gm_sw_full_cs_batch call in one call -- against the reference's
own known answers (tests/golden/sw_kat_post.txt.gz, which indexes the "S" records of sw_kat_cs.txt.gz) and against the single seam post_sw beyond them.

Figures seen on an MI355X (profiles/r07a_post_sw_batch_error.json): see the docstrings of the two known-answer tests."""
import ctypes as C
import gzip, os, subprocess, sys, threading
import numpy as np
import pytest
from tests import oracle_api as oa
from tests.test_sw_full_batch import CS_SETUP, items_cs, pack, run_cs, _oracle_items

POST_MAX_LEN = 2400                       # tests/seam_driver.cpp: max_len 2400, sanger QVs, offset 0, delta 33
REL = 1e-9                                # the kernel's own tie margin: device and host must differ by far less for the letter-call guard to be sound
HOST_SHARE = 0.05                         # at most this share of the answered items may come from the host routine


def _fixture():
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", "sw_kat_post.txt.gz"), "rt") as f: rows = [l.split() for l in f if l.strip()]
    K = [float.fromhex(x) for x in [t for t in rows if t[0] == "K"][0][1:]]
    # P <S ordinal> <use_qvs> <qual in> <posterior %a> matches mismatches crossovers <qralign> <qual out>
    P = [dict(idx=int(t[1]), useq=int(t[2]), qin=t[3], posterior=float.fromhex(t[4]), counts=[int(x) for x in t[5:8]], qralign=t[8], qual=t[9]) for t in rows if t[0] == "P"]
    return K, P


_cache = {}


def fixture():
    if "f" not in _cache: _cache["f"] = _fixture()
    return _cache["f"]


def s_items():
    if "s" not in _cache: _cache["s"] = items_cs("sw_kat_cs.txt.gz", "S")
    return _cache["s"]


def setup(gm, use_qvs=False, reset=True):
    gm.sw_full_cs_setup(*CS_SETUP)
    gm.post_sw_setup(POST_MAX_LEN, *fixture()[0], use_read_qvs=use_qvs, use_sanger_qvs=True, qual_vector_offset=0, qual_delta=33, reset_stats=reset)


def chain(gm, items, quals=None, is_rna=False):
    """one gm_sw_full_cs_batch call, then one gm_post_sw_batch call on what it returned"""
    recs, ops, strings, bases = run_cs(gm, items, is_rna=is_rna)
    p = pack(items)
    post, qralign, qual = gm.post_sw_batch(recs, ops, p["genome"], p["reads"], p["rlen"], p["initbp"], quals=quals, is_rna=is_rna)
    return dict(recs=recs, ops=ops, p=p, post=post, qralign=qralign, qual=qual, strings=strings)


def rel(a, b): return abs(a - b) / abs(b) if b else abs(a)


def check_known(res, wanted, what, cap=True):
    """wanted: (item of the call, P record) pairs.  Counts, qralign and qual equal; posterior within REL of the fixture's, bit-equal where the host routine answered"""
    post, worst, by_host = res["post"], 0.0, 0
    for k, w in wanted:
        R = post[k]
        assert R["status"] == 0, (what, k, R)
        assert [int(R["matches"]), int(R["mismatches"]), int(R["crossovers"])] == w["counts"], (what, k, R, w)
        assert res["qralign"](k) == w["qralign"], (what, k, res["qralign"](k), w["qralign"])
        assert res["qual"](k) == w["qual"] and int(R["qual_len"]) == len(w["qual"]), (what, k, res["qual"](k), w["qual"])
        d = rel(float(R["posterior"]), w["posterior"]); by_host += int(R["by_host"])
        if R["by_host"]: assert float(R["posterior"]).hex() == w["posterior"].hex(), (what, k, float(R["posterior"]).hex(), w["posterior"].hex())
        else: worst = max(worst, d)
        assert d <= REL, (what, k, d)
    print("%s: %d items, %d by the host routine (%.3f %%), largest relative posterior difference of the device's %.3e" % (what, len(wanted), by_host, 100.0 * by_host / len(wanted), worst))
    if cap: assert by_host <= HOST_SHARE * len(wanted), (what, by_host, len(wanted))
    return worst, by_host


def check_vs_single(gm, res, quals=None, is_rna=False, what=""):
    """every item with an alignment against the Python single seam on the strings gm_sw_full_batch_strings gives: everything equal but the posterior (within REL; bits where by_host)"""
    n_al, by_host = 0, 0
    recs, p, post = res["recs"], res["p"], res["post"]
    for k in range(len(recs)):
        if recs[k]["status"] < 0: continue
        if recs[k]["score"] <= 0:
            assert post[k]["status"] == 0 and post[k]["qual_len"] == 0 and post[k]["posterior"] == 0, (what, k, post[k]); continue
        db, qr = gm.sw_full_batch_strings(True, recs[k], res["ops"], p["genome"], p["reads"][k], int(p["initbp"][k]), is_rna, rlen=int(p["rlen"][k]))
        w = gm.post_sw(p["reads"][k], int(p["initbp"][k]), db, qr, int(recs[k]["read_start"]), qual=None if quals is None else quals[k])
        R = post[k]
        assert R["status"] == 0, (what, k, R)
        got = dict(matches=int(R["matches"]), mismatches=int(R["mismatches"]), crossovers=int(R["crossovers"]), qralign=res["qralign"](k), qual=res["qual"](k))
        assert got == {f: w[f] for f in got}, (what, k, got, w)
        if R["by_host"]: assert float(R["posterior"]).hex() == w["posterior"].hex(), (what, k)
        assert rel(float(R["posterior"]), w["posterior"]) <= REL, (what, k, float(R["posterior"]), w["posterior"])
        n_al += 1; by_host += int(R["by_host"])
    return n_al, by_host


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


@pytest.fixture(scope="module")
def plain(gm):
    """every "S" record through the two calls, without QVs: computed once, shared by the tests below and left unchanged"""
    setup(gm)
    return chain(gm, s_items())


# ---- 1 / 2: the reference's known answers ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_known_answers_without_qvs(gm, plain):
    """1 222 records.  Seen on an MI355X: see profiles/r07a_post_sw_batch_error.json (largest relative posterior difference, share answered by the host routine)."""
    K, P = fixture()
    want = [(w["idx"], w) for w in P if w["useq"] == 0]
    assert len(want) == 1222 and len(plain["post"]) == len(s_items()) >= 1400
    check_known(plain, want, "no QVs")
    answered = {k for k, _ in want}
    for k, it in enumerate(s_items()):                                 # an "S" record that scored nothing: status 0, no base qualities
        if k in answered: continue
        assert it["want"][0] == 0 and plain["recs"][k]["score"] == 0
        assert plain["post"][k]["status"] == 0 and plain["post"][k]["qual_len"] == 0 and plain["post"][k]["posterior"] == 0 and plain["qralign"](k) is None
    assert len(answered) < len(s_items())


@pytest.mark.gpu
def test_known_answers_with_qvs(gm):
    """611 records, each with the QV string the fixture gave the reference (use_read_qvs, sanger, offset 0, delta 33)"""
    K, P = fixture()
    want = [w for w in P if w["useq"] == 1]
    assert len(want) == 611
    setup(gm, use_qvs=True)
    res = chain(gm, [s_items()[w["idx"]] for w in want], quals=[w["qin"].encode() for w in want])
    check_known(res, list(enumerate(want)), "QVs")


# ---- 3: against the single seam beyond the fixture -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,kinds,rna,at_least", [("sw_kat_cs_xover.txt.gz", "X", False, 1000), ("sw_kat_cs_rna.txt.gz", "S", True, 600)])
def test_against_the_single_seam(gm, name, kinds, rna, at_least):
    """alignments made with per-position crossover rows, and on an RNA genome with is_rna (U in dbalign and in the read's translations)"""
    items = items_cs(name, kinds)
    assert len(items) >= at_least
    if kinds == "X": assert all(it["xs"] is not None for it in items)
    setup(gm)
    res = chain(gm, items, is_rna=rna)
    n_al, by_host = check_vs_single(gm, res, is_rna=rna, what=name)
    print("%s: %d alignments, %d by the host routine" % (name, n_al, by_host))
    # How many records of a set align is the fixture's property (888 of the X records, 520 of the RNA S records): at least 80 % of the set must, so that a
    # regression that leaves the items unaligned fails here.  The host routine's share: the known-answer tests hold the 5 % cap the issue sets; it does not hold on
    # the RNA set, where a U in the genome matches no state and two letters often explain a column equally well (44 of 520 = 8.5 % on an MI355X, a property of the
    # tie guard's 1e-9 margin and the data, the same in the pipeline kernel).  A fifth is the floor below which the kernel, not cs_post_sw, is what the set checks.
    assert n_al >= max(1, int(0.8 * at_least)) and by_host <= 0.2 * n_al, (n_al, by_host)
    if rna: assert any("U" in gm.sw_full_batch_strings(True, res["recs"][k], res["ops"], res["p"]["genome"], res["p"]["reads"][k], int(res["p"]["initbp"][k]), True,
                                                        rlen=int(res["p"]["rlen"][k]))[0] for k in range(len(items)) if res["recs"][k]["score"] > 0)


# ---- 4: edge shapes, hand-made records in the public encoding ---------------------------------------------------------------------------------
def _nibbles(codes):
    from shrimp_amd import synth
    return synth.pack_nibbles(np.asarray(codes, dtype=np.uint8))


def _handmade(gm):
    """(genome words, reads (n, words), rlen, initbp, recs, ops, quals): one small call of hand-made alignments"""
    rng = np.random.default_rng(7)
    G = rng.integers(0, 4, size=256, dtype=np.uint8); G[40] = 15; G[41] = 4                     # an N and a U in the genome
    shapes = []                                                                               # (colours, read_start, genome_start, op types)
    m = lambda n: [6 + int(x) for x in rng.integers(0, 4, size=n)]
    col = lambda n: [int(x) for x in rng.integers(0, 4, size=n)]
    shapes.append((col(1), 0, 3, m(1)))                                                       # one read position
    c = col(20); c[1] = 15
    shapes.append((c, 4, 10, m(12)))                                                          # read_start > 0, a 15 among the skipped colours
    c = col(20); c[2] = 15; c[3] = 15
    shapes.append((c, 5, 30, m(15)))                                                          # ... two of them, and the alignment crosses the genome's N and U
    shapes.append((col(16), 2, 50, [1] + m(10)))                                              # begins with a genome letter against a gap
    shapes.append((col(16), 0, 60, [3] + m(10)))                                              # begins with a read letter against a gap
    shapes.append((col(16), 1, 70, m(10) + [1]))                                              # ends in either
    shapes.append((col(16), 0, 80, m(10) + [4, 2]))
    shapes.append(([15] * 9, 0, 100, m(9)))                                                   # every colour 15
    shapes.append(([15] * 9, 3, 110, m(3) + [1, 1] + m(3)))
    c = col(30); c[10] = 15
    shapes.append((c, 3, 120, m(8) + [2, 3] + m(4) + [1] + m(6)))                             # a 15 inside the alignment, gaps of both kinds
    n = len(shapes); rw = 4
    reads = np.zeros((n, rw), dtype=np.uint32); rlen = np.zeros(n, dtype=np.int32); initbp = rng.integers(0, 4, size=n).astype(np.uint8)
    recs = np.zeros(n, dtype=gm.SW_FULL_REC_DTYPE); ops = []; quals = []
    for i, (c, rs, gs, types) in enumerate(shapes):
        w = _nibbles(c); reads[i, :len(w)] = w; rlen[i] = len(c)
        assert rs + sum(t != 1 for t in types) <= len(c)
        recs[i]["score"] = 100; recs[i]["read_start"] = rs; recs[i]["genome_start"] = gs; recs[i]["ops_off"] = len(ops); recs[i]["n_ops"] = len(types)
        ops += [t | (0x80 if rng.random() < 0.2 else 0) for t in types]
        quals.append(bytes(int(x) for x in 33 + 2 + rng.integers(0, 39, size=len(c))))
    return _nibbles(G), reads, rlen, initbp, recs, np.array(ops, dtype=np.uint8), quals


def _run_handmade(gm, sel, use_qvs):
    g, reads, rlen, initbp, recs, ops, quals = _handmade(gm)
    sel = np.asarray(sel)
    q = [quals[k] for k in sel] if use_qvs else None
    post, qralign, qual = gm.post_sw_batch(recs[sel], ops, g, reads[sel], rlen[sel], initbp[sel], quals=q)
    res = dict(recs=recs[sel], ops=ops, p=dict(genome=g, reads=reads[sel], rlen=rlen[sel], initbp=initbp[sel]), post=post, qralign=qralign, qual=qual)
    return check_vs_single(gm, res, quals=q, what="hand-made")


@pytest.mark.gpu
@pytest.mark.parametrize("use_qvs", [False, True])
def test_edge_shapes_against_the_single_seam(gm, use_qvs):
    """one read position; read_start > 0 behind a skipped 15; alignments that begin and end in a gap column; a read of 15s only -- in one small call, alone (n = 1)
    and in a call of 65 (one past a wave)"""
    setup(gm, use_qvs=use_qvs)
    n = len(_handmade(gm)[4])
    assert _run_handmade(gm, range(n), use_qvs)[0] == n
    for k in (0, 1, 7): assert _run_handmade(gm, [k], use_qvs)[0] == 1                          # n = 1
    assert _run_handmade(gm, [k % n for k in range(65)], use_qvs)[0] == 65                     # (records may share an ops slice: they write the same bytes)


# ---- 5: a thread slot's scratch is reused by items of other lengths ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_scratch_slots_serve_items_of_several_lengths(gm, plain):
    """One 1 000-colour alignment, 8 000 alignments of 150 and 300 colours (80 distinct ones, shuffled) and 9 000 shuffled fixture items in one call.  1 000 columns x 140
    bytes leave 3 776 thread slots inside the 512 MiB budget for the launch of the long ones: the plan the library reports says so, and every slot takes two or three
    alignments of different lengths through the same scratch.  Every repeat equals its first occurrence to the last bit, every fixture item the answer of the plain call."""
    setup(gm)
    extra = _oracle_items(1000, 1400, 1, 11, True) + _oracle_items(300, 420, 40, 12, True) + _oracle_items(150, 210, 40, 13, True)
    items = extra + s_items()
    base = chain(gm, items)
    recs, ops, p = base["recs"], base["ops"], base["p"]
    assert all(recs[k]["score"] > 0 for k in range(len(extra)))
    n_al, _ = check_vs_single(gm, dict(base, recs=recs[:len(extra)]), what="long and mid")       # the distinct long and mid-length ones against the single seam
    assert n_al == len(extra)
    fx = [k for k in range(len(extra), len(items)) if recs[k]["score"] > 0]
    rng = np.random.default_rng(20261018)
    order = np.concatenate([[0], rng.permutation(np.concatenate([np.tile(np.arange(1, len(extra)), 100), rng.choice(fx, 9000)]))])
    r2 = recs[order].copy()
    r2["ops_off"] = np.concatenate([[0], np.cumsum(r2["n_ops"][:-1])])
    ops2 = np.concatenate([ops[int(recs[k]["ops_off"]):int(recs[k]["ops_off"]) + int(recs[k]["n_ops"])] for k in order])
    post, qralign, qual = gm.post_sw_batch(r2, ops2, p["genome"], p["reads"][order], p["rlen"][order], p["initbp"][order])
    plan = gm.post_sw_batch_last_plan()
    assert any(cols >= 1000 and n >= 2 * threads for n, threads, cols in plan), plan           # the long launch: at least two items a slot
    assert len(plan) >= 2 and sum(n for n, _, _ in plan) == len(order), plan                     # split by length: the fixture items have a launch of their own
    first = {}
    for j, k in enumerate(order):
        k = int(k)
        got = (float(post[j]["posterior"]).hex(), int(post[j]["matches"]), int(post[j]["mismatches"]), int(post[j]["crossovers"]), int(post[j]["by_host"]), qralign(j), qual(j))
        assert post[j]["status"] == 0
        if k not in first:
            first[k] = got
            B = base["post"][k]                                                                 # ... which is the answer of the call that held every item once
            assert got == (float(B["posterior"]).hex(), int(B["matches"]), int(B["mismatches"]), int(B["crossovers"]), int(B["by_host"]), base["qralign"](k), base["qual"](k)), (j, k)
            if k >= len(extra):                                                                 # a fixture item: the plain call's answer (test 1's)
                q = k - len(extra); A = plain["post"][q]
                assert got == (float(A["posterior"]).hex(), int(A["matches"]), int(A["mismatches"]), int(A["crossovers"]), int(A["by_host"]), plain["qralign"](q), plain["qual"](q)), (j, k)
        else: assert got == first[k], (j, k, got, first[k])


# ---- 6: refusals beside answers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_items_beside_answered_ones(gm):
    K, P = fixture()
    want = [w for w in P if w["useq"] == 1][:40]
    setup(gm, use_qvs=True)
    items = [s_items()[w["idx"]] for w in want]
    recs, ops, strings, bases = run_cs(gm, items)
    p = pack(items)
    recs = recs.copy(); ops = ops.copy(); rlen = p["rlen"].copy(); quals = [w["qin"].encode() for w in want]
    bad = {3: "ops", 9: "read", 17: "byte", 22: "status", 31: "qv"}
    recs[3]["ops_off"] = ops.size - int(recs[3]["n_ops"]) + 1                                   # its operations pass ops_len by one byte
    rlen[9] = int(recs[9]["read_start"]) + sum(1 for b in ops[int(recs[9]["ops_off"]):int(recs[9]["ops_off"]) + int(recs[9]["n_ops"])] if (b & 15) != 1) - 1   # runs past the read
    ops[int(recs[17]["ops_off"]) + 2] = 0x0b                                                    # no operation of the encoding (none of the good items shares the byte)
    recs[22]["status"] = -4; recs[22]["score"] = 0
    quals[31] = quals[31][:int(rlen[31]) - 1]
    post, qralign, qual = gm.post_sw_batch(recs, ops, p["genome"], p["reads"], rlen, p["initbp"], quals=quals)
    msg = gm.lib().gm_last_error()
    for k in (3, 9, 17, 31): assert post[k]["status"] == -2 and post[k]["qual_len"] == 0 and post[k]["posterior"] == 0, (k, post[k])
    assert post[22]["status"] == -4
    assert b"item 31" in msg and b"QV string" in msg, msg                                        # the last refused item's reason
    good = [(k, w) for k, w in enumerate(want) if k not in bad]
    check_known(dict(post=post, qralign=qralign, qual=qual), good, "beside refusals", cap=False)       # (35 items: the share is test 2's business)


# ---- 7: stats ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stats_count_a_batch_item_like_a_single_call(gm, plain):
    setup(gm)                                                                                     # (resets the counters)
    recs, ops, p = plain["recs"], plain["ops"], plain["p"]
    gm.post_sw_batch(recs, ops, p["genome"], p["reads"], p["rlen"], p["initbp"])
    inv_b, cells_b, secs_b = gm.seam_stats("post_sw")
    setup(gm)
    for k in range(len(recs)):
        if recs[k]["score"] <= 0: continue
        db, qr = plain["strings"](k)
        gm.post_sw(p["reads"][k], int(p["initbp"][k]), db, qr, int(recs[k]["read_start"]))
    inv_s, cells_s, _ = gm.seam_stats("post_sw")
    assert (inv_b, cells_b) == (inv_s, cells_s) and inv_b == 1222 and cells_b > 0 and secs_b > 0, (inv_b, cells_b, inv_s, cells_s)


@pytest.mark.gpu
def test_release_build_passes_these_tests(gm):
    """the GPU tests of this file once more in a child interpreter on libgmapper_hip_release.so"""
    if "release" in os.path.basename(gm.LIB_PATH): return                                       # (this IS the child)
    rel_lib = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel_lib), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=dict(os.environ, GM_LIB_PATH=rel_lib), cwd=oa.ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    import re
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 10, r.stdout[-500:]


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------------------
def test_post_record_mirror_has_the_library_size():
    from shrimp_amd import gmapper as g
    L = g.lib()
    assert L.gm_abi_sizeof(5) == C.sizeof(g.PostRec) == g.POST_REC_DTYPE.itemsize == 40
    assert L.gm_abi_sizeof(6) == -1


def _raw_call(g, n, recs=True, post=True, outs=True):
    """gm_post_sw_batch on one empty record with chosen pointers left out; returns (rc, the three output words)"""
    L = g.lib()
    rec = np.zeros(1, dtype=g.SW_FULL_REC_DTYPE); rec["score"] = 1; po = np.zeros(1, dtype=g.POST_REC_DTYPE); po["status"] = 77
    z = np.zeros(2, dtype=np.uint32); one = np.ones(1, dtype=np.int32); ib = np.zeros(1, dtype=np.uint8)
    qa, qo, ql = C.c_void_p(0x1234), C.c_void_p(0x5678), C.c_uint64(99)
    rc = L.gm_post_sw_batch(n, rec.ctypes.data if recs else None, None, 0, z.ctypes.data_as(C.POINTER(C.c_uint32)), 2, z.ctypes.data_as(C.POINTER(C.c_uint32)), 1,
                            one.ctypes.data_as(C.POINTER(C.c_int)), ib.ctypes.data, None, 0, po.ctypes.data if post else None,
                            C.byref(qa) if outs else None, C.byref(qo) if outs else None, C.byref(ql) if outs else None)
    return rc, (qa.value, qo.value, ql.value, int(po[0]["status"]))


def test_not_set_up_empty_and_missing_arguments():
    from shrimp_amd import gmapper as g
    res = {}
    def fresh():                                                                                 # the setup state is per thread: a new thread has none
        res["rc"] = _raw_call(g, 1)[0]; res["msg"] = g.lib().gm_last_error()
    t = threading.Thread(target=fresh); t.start(); t.join()
    assert res["rc"] == -3 and b"post_sw_setup" in res["msg"]                                   # GM_E_NOTSETUP
    g.post_sw_setup(POST_MAX_LEN, *fixture()[0])
    assert _raw_call(g, 0) == (0, (0x1234, 0x5678, 99, 77))                                     # n = 0: GM_OK, nothing is touched
    assert _raw_call(g, 0, recs=False, post=False, outs=False)[0] == 0
    for kw in (dict(recs=False), dict(post=False), dict(outs=False)):
        assert _raw_call(g, 1, **kw)[0] == -2, kw                                               # GM_E_ARG


def test_python_single_seam_reproduces_fixture_records():
    """post_sw is host code: ten records of each QV mode to the last bit, no device"""
    from shrimp_amd import gmapper as g
    K, P = fixture()
    for useq in (0, 1):
        g.post_sw_setup(POST_MAX_LEN, *K, use_read_qvs=bool(useq), use_sanger_qvs=True, qual_vector_offset=0, qual_delta=33)
        for w in [w for w in P if w["useq"] == useq][:10]:
            it = s_items()[w["idx"]]
            got = g.post_sw(it["r"], it["initbp"], it["db"], it["qr"], it["want"][1], qual=w["qin"] if useq else None)
            assert got["posterior"].hex() == w["posterior"].hex() and [got["matches"], got["mismatches"], got["crossovers"]] == w["counts"], (w, got)
            assert got["qralign"] == w["qralign"] and got["qual"] == w["qual"], (w, got)
        assert g.seam_stats("post_sw")[0] == 10
