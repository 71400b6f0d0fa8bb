"""Pass 1 as a seam: gm_score_windows (Session.score_windows), gm_select_pass1_f1 (Session.select_pass1 with slots) and gm_read_hits (Session.read_hits).

What is held to what.  Without a GPU: hash_genome_window and the f1 call cache rule (f1_run, f1-wrapper.h:97-134) are restated here in Python on top of
tests/test_select.py's restate_pass1, and pinned to the oracle's top hits with hash_filter_calls on and off on tests/golden/f1_twins_60bp -- a segment and an
earlier copy of it with runs of IUPAC twins (S Y K N for A C G T), whose windows ALWAYS share a cache slot with the clean ones and score differently; the two
committed reference outputs (default, and -Z) differ in 49 reads.  On the GPU the library is held to the CPU oracle's scores, to the restatement, to its own
three-call chain and, chained to text, to the two reference outputs."""
import ctypes as C
import gzip, os, re
import numpy as np
import pytest
from tests import oracle_api as oa
from tests import test_select as ts
from tests import test_read_windows as trw

GM_E_ARG, GM_E_RANGE = -2, -4
TWINS = "f1_twins_60bp"
TWIN_OF = np.array([8, 9, 10, 15], dtype=np.uint8)                        # S Y K N: base & 3 folds them onto A C G T
LETTER_FIXTURES = ["cfg2s_100bp_2Mbp", "stress_60bp", "n1_noisy_70bp"]
CMPL_RNA = ts.CMPL.copy(); CMPL_RNA[0] = 4                              # complement_base of an RNA sequence: A <-> U (util.h:125-151)
M32 = 0xFFFFFFFF


# ---- restatements -------------------------------------------------------------------------------------------------------------------------------------------------
def hash_slot(codes):
    """hash_genome_window(array, goff, glen) % f1_window_cache_size on the glen codes themselves (ref: common/util.h:221-241, common/hash.h:69-92, f1-wrapper.h:27)"""
    key = 0
    for i in range(0, len(codes), 16):
        buf = 0
        for c in codes[i:i + 16]: buf = ((buf << 2) | (int(c) & 3)) & M32
        key = (key + (buf >> 16)) & M32                                  # hash_accumulate
        tmp = (((buf & 0xFFFF) << 11) ^ key) & M32
        key = ((key << 16) ^ tmp) & M32
        key = (key + (key >> 11)) & M32
    key ^= (key << 3) & M32; key = (key + (key >> 5)) & M32              # hash_finalize
    key ^= (key << 4) & M32; key = (key + (key >> 17)) & M32
    key ^= (key << 25) & M32; key = (key + (key >> 6)) & M32
    return key % 1048576


def slots_of(rows, contigs, colour=False):
    """the slot of every window: letter space the forward letters, colour space the colour translation of the strand the window is turned onto"""
    if not colour: return np.array([hash_slot(contigs[int(r[2])][int(r[3]):int(r[3]) + int(r[4])]) for r in rows], dtype=np.uint32)
    cols = [[ts.colours(c), ts.colours(ts.CMPL[c[::-1]])] for c in contigs]
    out = []
    for r in rows:
        st, cn, g_off, wl = (int(x) for x in r[1:5])
        go = g_off if st == 0 else len(contigs[cn]) - g_off - wl
        out.append(hash_slot(cols[cn][st][go:go + wl]))
    return np.array(out, dtype=np.uint32)


def f1_taken(rows, off, scores, slots, read_len, R):
    """the cache rule per read-strand: -> (the score every window TAKES, bypassed calls).  A window past the matches check and the overlap check takes the score of
    the first earlier COMPUTED window of its read-strand with its slot, else keeps its own and is computed; last_good advances on the taken score."""
    W = int(ts.abs_or_pct(R["window_len"], read_len)) & 0xFFFF
    ov = int(ts.abs_or_pct(R["window_overlap"], W)) & 0xFFFFFFFF
    taken = np.array(scores, dtype=np.int32).copy(); bypassed = 0
    for rs in range(len(off) - 1):
        cache, last = {}, None                                           # a new tag per read-strand (mapping.c:1268)
        for i in range(int(off[rs]), int(off[rs + 1])):
            cn, g_off, w_len, _, matches = (int(x) for x in rows[i, 2:7])
            if matches < R["match_mode"]: continue
            if last is not None and cn == last[0] and g_off + ov <= last[1] + W: continue
            s = int(slots[i])
            if s in cache: taken[i] = cache[s]; bypassed += 1
            else: cache[s] = int(scores[i])
            thr = int(ts.abs_or_pct(R["sw_vect_threshold"], min(read_len, w_len) * R["match"]))
            if taken[i] >= thr: last = (cn, g_off)
    return taken, bypassed


def restate_pass1_f1(rows, off, scores, slots, read_len, R, clen):
    """restate_pass1 with the cache (slots None: without): -> (top, hits, hit_off, bypassed)"""
    if slots is None: return ts.restate_pass1(rows, off, scores, read_len, R, clen) + (0,)
    taken, byp = f1_taken(rows, off, scores, slots, read_len, R)
    return ts.restate_pass1(rows, off, taken, read_len, R, clen) + (byp,)


# ---- the twins fixture ----------------------------------------------------------------------------------------------------------------------------------------------
_twins = {}


def twins(L):
    """what the CPU side knows of f1_twins_60bp, as test_select.reference keeps it for its fixtures, with the oracle's top hits under both settings of the cache"""
    if _twins: return _twins
    contigs, reads, _ = oa.load_golden(TWINS)
    cs = [np.ascontiguousarray(c, dtype=np.uint8) for c in contigs]; reads = np.ascontiguousarray(reads, dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    h = L.rwo_create(len(cs), (u8p * len(cs))(*[c.ctypes.data_as(u8p) for c in cs]), (C.c_uint64 * len(cs))(*[len(c) for c in cs]), 0, 2)
    cap = 64 * len(reads); rows = np.zeros((cap, 12), dtype=np.int64)
    w = L.rwo_windows(h, reads.shape[0], reads.shape[1], reads.ctypes.data_as(u8p), ts.THREADS, rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
    L.rwo_destroy(h)
    assert 0 < w <= cap
    rows = rows[:w].copy()
    off = np.searchsorted(rows[:, 0] * 2 + rows[:, 1], np.arange(2 * len(reads) + 1)).astype(np.uint64)
    g = ts.pack(cs[0]); O = oa.load()
    scores = np.zeros(w, dtype=np.int32)
    for i in range(w):
        rd, st, _, g_off, wl = (int(x) for x in rows[i, :5])
        scores[i] = O.gmo_sw_vector(ts._u32(g), g_off, wl, ts._u32(ts.pack(ts.CMPL[reads[rd][::-1]] if st else reads[rd])), reads.shape[1])
    top = {}
    for on in (False, True):
        S = oa.Session(contigs); S.set(hash_filter_calls=on)
        top[on] = S.tophits(reads, nthreads=ts.THREADS).copy(); S.close()
    _twins.update(contigs=cs, reads=reads, rows=rows, off=off, scores=scores, top=top, clen=np.array([len(c) for c in cs], dtype=np.int64), rlen=reads.shape[1])
    return _twins


def by_read(sam):
    out = {}
    for l in sam.splitlines(keepends=True):
        if not l.startswith(b"@"): out.setdefault(int(l.split(b"\t", 1)[0][1:]), []).append(l)
    return out


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_three_entries():
    """fails without the feature"""
    try: import torch
    except Exception: pass
    from shrimp_amd import gmapper as gm
    L = gm.lib()
    header = open(os.path.join(oa.ROOT, "include", "gmapper_hip.h")).read()
    for name in ("gm_score_windows", "gm_select_pass1_f1", "gm_read_hits"):
        assert hasattr(L, name) and name in gm.EXPORTS and re.search(r"\b%s\(" % name, header), name
    for meth in ("score_windows", "read_hits"): assert callable(getattr(gm.Session, meth))


def test_the_two_reference_outputs_differ_by_the_cache():
    _, reads, sam = oa.load_golden(TWINS)
    on, off = by_read(sam), by_read(oa.load_option_sam(TWINS, "no_cache"))
    differ = [r for r in range(len(reads)) if on.get(r) != off.get(r)]
    assert len(differ) >= 20 and len(differ) == 49 and len(off) == 300 and len(on) == 251
    for r in differ:
        assert r not in on                                               # unmapped by default (no record without --sam-unaligned) ...
        assert len(off[r]) == 1 and off[r][0].split(b"\t")[5] == b"60M"  # ... a perfect mapping under -Z


def test_the_committed_fixture_is_the_recipe():
    contigs, reads, _ = oa.load_golden(TWINS)
    assert len(contigs) == 1 and contigs[0].shape == (40000,) and reads.shape == (300, 60)
    g = contigs[0]; seg = g[25000:25400]; copy = g[5000:5400]
    assert np.array_equal(np.delete(g, np.arange(5000, 5400)), np.delete(np.random.default_rng(11).integers(0, 4, 40000).astype(np.uint8), np.arange(5000, 5400)))
    assert (seg < 4).all()
    twin = np.zeros(400, dtype=bool)
    for lo in range(40, 321, 40): twin[lo:lo + 22] = True
    assert np.array_equal(copy[~twin], seg[~twin]) and np.array_equal(copy[twin], TWIN_OF[seg[twin]]) and int(twin.sum()) == 8 * 22
    assert all(np.array_equal(reads[k], seg[20 + k:80 + k]) for k in range(300))
    assert hash_slot(seg[:84]) == hash_slot(copy[:84])                   # twins fold onto their letters: one slot


def test_restated_cache_rule_gives_the_top_hits_of_the_oracle(driver):
    F = twins(driver); R = ts.fixture_rules("cfg2s_100bp_2Mbp")          # (the defaults: match mode 2, letter space)
    slots = slots_of(F["rows"], F["contigs"])
    top_on, _, _, byp = restate_pass1_f1(F["rows"], F["off"], F["scores"], slots, F["rlen"], R, F["clen"])
    top_off, _, _, _ = restate_pass1_f1(F["rows"], F["off"], F["scores"], None, F["rlen"], R, F["clen"])
    assert (len(F["top"][True]), len(F["top"][False])) == (256, 305)
    assert np.array_equal(top_on, F["top"][True]) and np.array_equal(top_off, F["top"][False])
    assert byp == 49                                                     # the reference reports 49 bypassed calls on this input


@pytest.mark.parametrize("name", LETTER_FIXTURES)
def test_slots_change_nothing_on_the_selection_fixtures(driver, name):
    """the slot function pinned the other way: no spurious sharing.  The restatement with slots gives the top hits it gives without, and the oracle agrees"""
    F = ts.reference(driver, name); R = ts.fixture_rules(name)
    slots = slots_of(F["rows"], F["contigs"])
    top, _, _, _ = restate_pass1_f1(F["rows"], F["off"], F["scores"], slots, F["rlen"], R, F["clen"])
    assert np.array_equal(top, F["top"])
    S = oa.Session(F["contigs"], opts=ts.FIXTURES[name][2]); S.set(hash_filter_calls=True)
    on = S.tophits(F["reads"], nthreads=ts.THREADS).copy(); S.close()
    assert np.array_equal(on, F["top"])


driver = ts.driver                                                       # (the fixture: tests/read_windows_oracle.cpp, compiled once for this module)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------------------
gm = ts.gm
_open = {}


def opened(gm, name, fields=None):
    """(index, session, params, reads) of a fixture under its match mode and the given gm_params_t fields.  This module's own, with sub-batches of 8 192 reads (every
    fixture fits one), and closed when the module is done: the device memory of the sessions is not held while the modules after this one run"""
    key = (name, tuple(sorted((fields or {}).items())))
    if key not in _open:
        contigs, reads, _ = oa.load_golden(name)
        p = ts.params_of(gm, name, **(fields or {})) if name in ts.FIXTURES else gm.default_params()
        if name not in ts.FIXTURES:
            for k, v in (fields or {}).items(): setattr(p, k, v)
        ix = gm.Index(contigs, params=p)
        _open[key] = (ix, gm.Session(ix, params=p, max_batch_reads=8192), p, np.ascontiguousarray(reads, dtype=np.uint8))
    return _open[key]


def open_twins(gm, **fields): return opened(gm, TWINS, fields)


@pytest.fixture(scope="module", autouse=True)
def close_the_sessions_of_this_module():
    yield
    for ix, s, _, _ in _open.values(): s.close(); ix.close()
    _open.clear()


def body_of(p, reads):
    """(codes, initbp) as the read entries take a fixture's reads"""
    return (np.ascontiguousarray(reads[:, 1:]), np.ascontiguousarray(reads[:, 0])) if p.colour_space else (reads, None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ts.FIXTURES))
def test_scores_and_slots_on_the_driver_windows_equal_the_oracle(gm, driver, name):
    F = ts.reference(driver, name)
    assert len(F["rows"]) == trw.FIXTURES[name][2]
    ix, s, p, reads = opened(gm, name)
    codes, ib = body_of(p, reads)
    scores, slots = s.score_windows(codes, ts.as_wins(gm, F["rows"]), F["off"], initbp=ib)
    bad = np.nonzero(scores != F["scores"])[0]
    assert len(bad) == 0, (len(bad), F["rows"][bad[:5]], scores[bad[:5]], F["scores"][bad[:5]])
    assert np.array_equal(slots, slots_of(F["rows"], F["contigs"], F["colour"]))
    if name == "stress_60bp":                                            # the mirrored call (the reverse-complement contig, the read as given) is not pass 1's
        rows = F["rows"]; rev = np.nonzero(rows[:, 1] == 1)[0]
        from shrimp_amd import synth
        rw = np.ascontiguousarray(synth.pack_reads(reads)); clen = ix.contig_lengths()
        ts.vector_setup(gm, p)
        mirrored = ix.sw_vector_batch(rows[rev, 2], np.ones(len(rev), dtype=np.uint8), clen[rows[rev, 2]] - rows[rev, 3] - rows[rev, 4], rows[rev, 4], rw[rows[rev, 0]],
                                      np.full(len(rev), reads.shape[1]))
        wrong = rev[mirrored != F["scores"][rev]]
        assert len(wrong) == 2 and (np.abs(mirrored[mirrored != F["scores"][rev]] - F["scores"][wrong]) == 25).all()
        assert np.array_equal(scores[wrong], F["scores"][wrong])


def hand_genome():
    rng = np.random.default_rng(1701)
    c0 = rng.integers(0, 4, 4000).astype(np.uint8); c0[100:116] = np.arange(16, dtype=np.uint8)        # every letter code
    c1 = np.array([0, 1, 2, 4], dtype=np.uint8)[rng.integers(0, 4, 2500)]                                # an RNA contig: U, no T
    c2 = rng.integers(0, 4, 1500).astype(np.uint8)
    return [c0, c1, c2]


def hand_windows(lists):
    """per read-strand a list of (cn, g_off, w_len) -> rows, off"""
    rows, off = [], [0]
    for rs, lst in enumerate(lists):
        for k, (cn, g_off, w_len) in enumerate(lst): rows.append((rs // 2, rs & 1, cn, g_off, w_len, 100 + k, 2, 1, 1, 5, 1, 0))
        off.append(len(rows))
    return np.array(rows, dtype=np.int64).reshape(-1, 12), np.array(off, dtype=np.uint64)


@pytest.mark.gpu
def test_hand_made_windows_in_letter_space(gm):
    """read lengths around the word boundaries of the device reverse complement, the 64-lane step and the over-128 path, on both strands; windows at offset 0, ending
    at the contig's last base, shorter than the read, holding every letter code; a U read (no T) on an RNA contig on strand 1"""
    contigs = hand_genome(); c0, c1, _ = contigs
    p = gm.default_params(); ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p, max_batch_reads=1024)
    O = oa.load(); packed = [ts.pack(c) for c in contigs]; rng = np.random.default_rng(5)
    for L in (7, 8, 9, 63, 64, 65, 127, 128, 129, 1000):
        W = min(1400, int(1.4 * L))
        r0 = c0[200:200 + L].copy(); r0[rng.integers(0, L, 2)] ^= 1
        r1 = ts.CMPL[c0[300:300 + L][::-1]].copy()
        seg = c1[50:50 + L]; r2 = CMPL_RNA[seg[::-1]].copy()                # strand 1 of an RNA molecule: its reverse complement through the RNA table is seg again
        if L >= 63: assert (r2 == 4).any() and not (r2 == 3).any()
        reads = np.stack([r0, r1, r2])
        wl = [(0, 0, W), (0, 95, W), (0, 190, W), (0, 205, max(1, L - 3)), (0, len(c0) - W, W), (0, len(c0) - 5, 5), (1, 40, W), (1, len(c1) - W, W), (2, 0, min(W, len(contigs[2])))]
        rows, off = hand_windows([wl] * 6)
        scores, slots = s.score_windows(reads, ts.as_wins(gm, rows), off)
        want = np.zeros(len(rows), dtype=np.int32)
        for i, r in enumerate(rows):
            rd, st, cn, g_off, w_len = (int(x) for x in r[:5])
            q = reads[rd]
            if st: q = (CMPL_RNA if (q == 4).any() and not (q == 3).any() else ts.CMPL)[q[::-1]]
            want[i] = O.gmo_sw_vector(ts._u32(packed[cn]), g_off, w_len, ts._u32(ts.pack(q)), L)
        assert np.array_equal(scores, want), (L, rows[scores != want][:5], scores[scores != want][:5], want[scores != want][:5])
        assert np.array_equal(slots, slots_of(rows, contigs))
        if L >= 63: assert want[rows[:, 0] == 2].max() == 10 * L            # the U read scores in full on its RNA contig, strand 1
    s.close(); ix.close()


@pytest.mark.gpu
def test_hand_made_windows_in_colour_space(gm):
    """colour reads with each primer letter, both strands, windows at both ends of a contig and over every letter code"""
    contigs = [hand_genome()[0], hand_genome()[2]]
    p = gm.default_params_cs(); ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p, max_batch_reads=1024)
    O = oa.load()
    letters = [[c, ts.CMPL[c[::-1]]] for c in contigs]
    ls = [[ts.pack(x) for x in pair] for pair in letters]; cs = [[ts.pack(ts.colours(x)) for x in pair] for pair in letters]
    for L in (25, 65, 130):
        W = int(1.4 * L)
        src = [contigs[0][200:201 + L], ts.CMPL[contigs[0][300:301 + L][::-1]], contigs[1][0:1 + L], ts.CMPL[contigs[1][-1 - L:][::-1]]]
        cols = np.stack([ts.colours(x)[1:] for x in src]); cols[0, 3] ^= 1
        ib = np.array([0, 1, 2, 3], dtype=np.uint8)
        wl = [(0, 0, W), (0, 95, W), (0, 195, W), (0, len(contigs[0]) - W, W), (0, 290, L - 4), (1, 0, W), (1, len(contigs[1]) - W, W)]
        rows, off = hand_windows([wl] * 8)
        scores, slots = s.score_windows(cols, ts.as_wins(gm, rows), off, initbp=ib)
        want = np.zeros(len(rows), dtype=np.int32)
        for i, r in enumerate(rows):
            rd, st, cn, g_off, w_len = (int(x) for x in r[:5])
            go = g_off if st == 0 else len(contigs[cn]) - g_off - w_len
            want[i] = O.gmo_sw_vector_cs(ts._u32(cs[cn][st]), go, w_len, ts._u32(ts.pack(cols[rd])), L, ts._u32(ls[cn][st]), int(ib[rd]))
        assert np.array_equal(scores, want), (L, rows[scores != want][:5], scores[scores != want][:5], want[scores != want][:5])
        assert np.array_equal(slots, slots_of(rows, contigs, True))
        assert int(want.max()) >= 10 * (L - 2)
    s.close(); ix.close()


def ungapped_case(gm, which):
    """(index, session, params, reads [n, L(+1)]) of an ungapped session"""
    if which in ("rna_ls", "rna_cs"):
        case = oa.load_rna_case(which); colour = case["colour"]; contigs = case["contigs"]; reads = case["reads"][0][1]
        fields = dict(oa.CS_OPTION_CASES["cs_ungapped"][2]) if colour else {k: v for k, v in oa.OPTION_CASES["ungapped60_n1"][2].items() if k != "match_mode"}
    elif which == "stress_60bp": contigs, reads, _ = oa.load_golden(which); colour = False; fields = dict(oa.OPTION_CASES["ungapped60_n1"][2])
    else: contigs, reads, _ = oa.load_golden(which); colour = True; fields = dict(oa.CS_OPTION_CASES["cs_ungapped_unal"][2])
    p = gm.default_params_cs() if colour else gm.default_params()
    for k, v in fields.items(): setattr(p, k, v)
    ix = gm.Index(contigs, params=p)
    return ix, gm.Session(ix, params=p, max_batch_reads=8192), p, np.ascontiguousarray(reads, dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["stress_60bp", "stress_cs_60col_unal", "rna_ls", "rna_cs"])
def test_ungapped_sessions_score_the_diagonal_through_the_box(gm, which):
    """-U: score_windows == gm_sw_gapless_batch_ix fed by hand (letter space: the forward contig, the box as the record holds it, the read turned on the host; colour
    space: the hit and its box turned, the read as given), and == the pipeline's score on every window that is a top hit"""
    from shrimp_amd import synth
    ix, s, p, reads = ungapped_case(gm, which)
    colour = bool(p.colour_space); codes, ib = body_of(p, reads); L = codes.shape[1]
    wins, off = s.read_windows(codes, initbp=ib)
    rows = ts.win_rows(wins); assert len(rows) > len(codes) // 2 and (rows[:, 1] == 1).sum() > len(codes) // 8      # (a window for most reads, both strands in use)
    scores, _ = s.score_windows(codes, wins, off, initbp=ib)
    clen = ix.contig_lengths(); rd, st, cn = rows[:, 0], rows[:, 1], rows[:, 2]
    gm.sw_gapless_setup(p.match_score, p.match_score + p.crossover_score if colour else p.mismatch_score, True)
    if colour:
        t = st == 1
        go = np.where(t, clen[cn] - rows[:, 3] - rows[:, 4], rows[:, 3])
        ax = np.where(t, -rows[:, 7] + (rows[:, 4] - 1) - (rows[:, 9] - 1) - (rows[:, 10] - 1), rows[:, 7])
        ay = np.where(t, -rows[:, 8] + (L - 1) - (rows[:, 9] - 1) + (rows[:, 10] - 1), rows[:, 8])
        rw = np.ascontiguousarray(synth.pack_reads(codes))
        by_hand = ix.sw_gapless_batch(cn, st.astype(np.uint8), rw[rd], np.full(len(rows), L), go + ax, ay, initbp=ib[rd], colour_space=True)
    else:
        rna = np.array([(r == 4).any() and not (r == 3).any() for r in codes])
        rc = np.stack([(CMPL_RNA if rna[k] else ts.CMPL)[codes[k][::-1]] for k in range(len(codes))])
        rw = np.ascontiguousarray(synth.pack_reads(codes)); rcw = np.ascontiguousarray(synth.pack_reads(np.ascontiguousarray(rc)))
        both = np.where((st == 1)[:, None], rcw[rd], rw[rd])
        by_hand = ix.sw_gapless_batch(cn, np.zeros(len(rows), dtype=np.uint8), both, np.full(len(rows), L), rows[:, 3] + rows[:, 7], rows[:, 8])
        if which == "rna_ls": assert rna.any()
    bad = np.nonzero(scores != by_hand)[0]
    assert len(bad) == 0, (len(bad), rows[bad[:5]], scores[bad[:5]], by_hand[bad[:5]])
    top = s.tophits(codes, initbp=ib)                                    # read st cn g_off w_len score_vector pct matches ax ay alen awidth
    mine = {}
    for r, sc in zip(rows, scores): mine.setdefault(tuple(int(x) for x in r[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10]]), set()).add(int(sc))
    assert len(top) > len(codes) // 4
    for t in top:
        k = tuple(int(x) for x in t[[0, 1, 2, 3, 4, 7, 8, 9, 10, 11]])
        assert k in mine and (int(t[5]) in mine[k] or int(t[5]) == 0), (t, mine.get(k))     # (0: a window the overlap rule skipped)
    s.close(); ix.close()


@pytest.mark.gpu
def test_twin_windows_share_their_slots_read_by_read(gm, driver):
    F = twins(driver)
    ix, s, p, reads = open_twins(gm)
    scores, slots = s.score_windows(reads, ts.as_wins(gm, F["rows"]), F["off"])
    assert np.array_equal(scores, F["scores"]) and np.array_equal(slots, slots_of(F["rows"], F["contigs"]))
    rows = F["rows"]; shared = 0
    for r in range(len(reads)):
        a, b = int(F["off"][2 * r]), int(F["off"][2 * r + 1])
        dmg = [i for i in range(a, b) if rows[i, 3] < 20000]; clean = [i for i in range(a, b) if rows[i, 3] >= 20000]
        if not dmg or not clean: continue
        for i in dmg:
            mates = [j for j in clean if rows[j, 3] - 20000 == rows[i, 3] and rows[j, 4] == rows[i, 4]]
            if mates: shared += 1; assert all(slots[j] == slots[i] for j in mates) and all(scores[j] > scores[i] for j in mates)
    assert shared >= 49


@pytest.mark.gpu
def test_selection_with_the_cache_on_the_twins(gm, driver):
    F = twins(driver)
    ix, s, p, reads = open_twins(gm)
    wins = ts.as_wins(gm, F["rows"])
    scores, slots = s.score_windows(reads, wins, F["off"])
    hits, hit_off, byp = s.select_pass1(wins, F["off"], scores, F["rlen"], slots=slots, want_bypassed=True)
    top, want, want_off, want_byp = restate_pass1_f1(F["rows"], F["off"], scores, slots, F["rlen"], ts.rules_of(p), F["clen"])
    got = ts.hit_rows(hits)
    assert np.array_equal(hit_off, want_off) and np.array_equal(got, want) and byp == want_byp and byp >= 49
    assert np.array_equal(ts.unturned(got, F["rlen"], F["clen"]), F["top"][True])
    plain, plain_off = s.select_pass1(wins, F["off"], scores, F["rlen"])
    none, none_off, zero = s.select_pass1(wins, F["off"], scores, F["rlen"], slots=None, want_bypassed=True)
    assert plain.tobytes() == none.tobytes() and np.array_equal(plain_off, none_off) and zero == 0
    assert np.array_equal(ts.unturned(ts.hit_rows(plain), F["rlen"], F["clen"]), F["top"][False])


@pytest.mark.gpu
def test_selection_with_hand_made_slots(gm, driver):
    """stress_60bp's windows and scores under slot arrays that put the rule's cases side by side, each against the restatement"""
    F = ts.reference(driver, "stress_60bp")
    ix, s, p, reads = opened(gm, "stress_60bp")
    rows, off, scores = F["rows"], F["off"], F["scores"]; wins = ts.as_wins(gm, rows); R = ts.rules_of(p); n = len(rows)
    per = np.diff(off.astype(np.int64)); assert per.max() > 128             # lists across the 64-window step
    W = int(ts.abs_or_pct(R["window_len"], F["rlen"])); ov = int(ts.abs_or_pct(R["window_overlap"], W))

    def check(slots, sc=scores, rws=rows):
        hits, hit_off, byp = s.select_pass1(ts.as_wins(gm, rws), off, sc, F["rlen"], slots=slots, want_bypassed=True)
        _, want, want_off, want_byp = restate_pass1_f1(rws, off, sc, slots, F["rlen"], R, F["clen"])
        got = ts.hit_rows(hits)
        assert np.array_equal(hit_off, want_off) and byp == want_byp, (byp, want_byp)
        assert np.array_equal(got, want), (got[(got != want).any(axis=1)][:5], want[(got != want).any(axis=1)][:5])
        return got, byp
    _, byp = check(np.zeros(n, dtype=np.uint32))                         # all slots equal: every read-strand scores its first computed window only
    assert byp > 1000
    got, byp = check(np.arange(n, dtype=np.uint32))                      # all distinct: nothing is bypassed, the plain selection
    assert byp == 0 and np.array_equal(got, ts.hit_rows(s.select_pass1(wins, off, scores, F["rlen"])[0]))
    key = rows[:, 0] * 2 + rows[:, 1]
    check((key % 2).astype(np.uint32))                                   # one slot a strand: the two strands of a read must not share
    big = int(np.argmax(per)); a = int(off[big])                         # the longest list: a slot shared across the 64-window step
    sl = np.arange(n, dtype=np.uint32); sl[a + 100] = sl[a + 3]; sl[a + 130] = sl[a + 3]
    check(sl)
    # a shared slot whose first holder is passed over by `matches`, skipped by the overlap rule, or itself bypassed: three windows at chosen places of one list
    assert (W, ov) == (84, 75)                                           # (60-base reads: the threshold is 300 of 600)
    lst = [(0, 1000, 84, 600, 2), (0, 1000 + W - ov, 84, 100, 2), (0, 3000, 84, 290, 2), (0, 5000, 84, 590, 2), (0, 7000, 84, 100, 2), (0, 9000, 84, 580, 2)]
    def shaped(matches1, slots6):
        l2 = [w if k != 1 else w[:4] + (matches1,) for k, w in enumerate(lst)]
        r, o, sc = ts.shape_windows([l2, []])
        hits, hit_off, byp = s.select_pass1(ts.as_wins(gm, r), o, sc, F["rlen"], slots=np.array(slots6, dtype=np.uint32), want_bypassed=True)
        _, want, want_off, want_byp = restate_pass1_f1(r, o, sc, np.array(slots6), F["rlen"], R, F["clen"])
        assert np.array_equal(ts.hit_rows(hits), want) and np.array_equal(hit_off, want_off) and byp == want_byp
        return ts.hit_rows(hits)[:, 7].tolist(), byp
    sv, byp = shaped(2, [1, 7, 3, 4, 7, 6])                               # window 1 is skipped by window 0 (overlap): not computed, window 4 keeps its own 100
    assert byp == 0 and sorted(sv) == [580, 590, 600]
    sv, byp = shaped(1, [1, 7, 3, 4, 7, 6])                               # window 1 is passed over by matches: the same
    assert byp == 0 and sorted(sv) == [580, 590, 600]
    sv, byp = shaped(2, [1, 2, 3, 3, 3, 6])                               # window 3 takes 290 from window 2 and is NOT computed: window 4 takes 290 too, not 590
    assert byp == 2 and sorted(sv) == [580, 600]
    sv, byp = shaped(2, [1, 2, 9, 4, 5, 1])                               # window 5 takes window 0's 600
    assert byp == 1 and sorted(sv) == [590, 600, 600]


@pytest.mark.gpu
def test_the_cache_in_colour_space_gives_the_top_hits_of_the_pipeline(gm, driver):
    name = "cfg4s_50col_2Mbp"
    F = ts.reference(driver, name)
    ix, s, p, reads = opened(gm, name)
    assert p.hash_filter_calls == 1
    codes, ib = body_of(p, reads); wins = ts.as_wins(gm, F["rows"])
    scores, slots = s.score_windows(codes, wins, F["off"], initbp=ib)
    hits, hit_off = s.select_pass1(wins, F["off"], scores, F["rlen"], slots=slots)
    top_ref = s.tophits(codes, initbp=ib)
    assert len(top_ref) > 3000 and np.array_equal(ts.unturned(ts.hit_rows(hits), F["rlen"], F["clen"]), top_ref)


def chain_of(s, p, reads, cache):
    codes, ib = body_of(p, reads)
    wins, off = s.read_windows(codes, initbp=ib)
    scores, slots = s.score_windows(codes, wins, off, initbp=ib)
    hits, hit_off = s.select_pass1(wins, off, scores, slots=slots if cache else None)
    return wins, off, scores, hits, hit_off


def same_up_to_equal_windows(got, want):
    """hits, offsets, windows and own scores of two runs: byte-equal, where groups of equal (read, st, cn, g_off) windows (in no promised order) are compared as
    multisets and the hits that name a window of such a group without their window index and box"""
    wins, off, scores, hits, hit_off = got; wins2, off2, scores2, hits2, hit_off2 = want
    assert np.array_equal(off, off2) and np.array_equal(hit_off, hit_off2)
    a = np.concatenate([ts.win_rows(wins), scores[:, None].astype(np.int64)], axis=1); b = np.concatenate([ts.win_rows(wins2), scores2[:, None].astype(np.int64)], axis=1)
    tied = ts.tie_mask(a[:, :12])
    assert np.array_equal(tied, ts.tie_mask(b[:, :12]))
    assert wins[~tied].tobytes() == wins2[~tied].tobytes() and np.array_equal(scores[~tied], scores2[~tied])
    assert np.array_equal(trw.canon(a), trw.canon(b))
    h, h2 = ts.hit_rows(hits), ts.hit_rows(hits2)
    assert h.shape == h2.shape
    if not tied.any(): assert hits.tobytes() == hits2.tobytes(); return 0
    in_group = tied[h[:, 2]]; cols = np.ones(16, dtype=bool); cols[[2, 12, 13, 14, 15]] = False
    assert np.array_equal(h[~in_group], h2[~in_group]) and np.array_equal(h[in_group][:, cols], h2[in_group][:, cols])
    return int(tied.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ts.FIXTURES) + [TWINS])
def test_read_hits_equal_the_three_calls(gm, name):
    ix, s, p, reads = open_twins(gm) if name == TWINS else opened(gm, name)
    codes, ib = body_of(p, reads)
    want = chain_of(s, p, reads, cache=True)
    hits, hit_off, wins, off, scores = s.read_hits(codes, initbp=ib, want_windows=True)
    st = dict(s.stats)
    tied = same_up_to_equal_windows((wins, off, scores, hits, hit_off), want)
    assert (tied > 0) == (name == "stress_60bp")
    assert st["windows"] == len(wins) == st["vec_calls"] and st["reads"] == len(reads)
    assert st["vec_cells"] == int((wins["w_len"].astype(np.int64) * codes.shape[1]).sum())
    _, _, byp = s.select_pass1(wins, off, scores, slots=s.score_windows(codes, wins, off, initbp=ib)[1], want_bypassed=True)
    assert st["vec_bypassed"] == byp and (byp >= 49 if name == TWINS else True)
    h2, o2 = s.read_hits(codes, initbp=ib)                               # the short form: the same hits
    assert np.array_equal(o2, hit_off) and (tied or h2.tobytes() == hits.tobytes())


@pytest.mark.gpu
def test_read_hits_over_three_sub_batches_with_a_capacity_growth(gm):
    """stress_60bp through sub-batches of 1 024 reads (three), rows of 64 windows that two read-strands overflow: window indices and offsets are the call's"""
    _, s0, p, reads = opened(gm, "stress_60bp")
    want = chain_of(s0, p, reads, cache=True)
    ix, s, _, _ = trw.open_session(gm, "stress_60bp", max_batch_reads=1024)
    hits, hit_off, wins, off, scores = s.read_hits(reads, want_windows=True)
    st = dict(s.stats); s.close(); ix.close()
    assert st["retries"] >= 1 and st["windows"] == len(wins) and st["reads"] == len(reads) == 3000
    same_up_to_equal_windows((wins, off, scores, hits, hit_off), want)
    assert (hits["win"] >= 0).all() and (hits["win"] < len(wins)).all() and (np.diff(hits["read"]) >= 0).all() and int(hits["read"].max()) > 2048
    assert np.array_equal(wins["read"][hits["win"]], hits["read"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cfg2s_100bp_2Mbp", TWINS])
def test_read_hits_without_the_cache_equal_the_chain_without_slots(gm, name):
    ix, s, p, reads = open_twins(gm, hash_filter_calls=0) if name == TWINS else opened(gm, name, dict(hash_filter_calls=0))
    want = chain_of(s, p, reads, cache=False)
    hits, hit_off, wins, off, scores = s.read_hits(reads, want_windows=True)
    same_up_to_equal_windows((wins, off, scores, hits, hit_off), want)
    assert s.stats["vec_bypassed"] == 0
    if name == TWINS: assert len(hits) == 305


def chain_to_sam(gm, ix, s, p, reads, hits, hit_off):
    """letter space: hits -> vector again -> full -> select_pass2 -> text -> sam_records: the records of every read"""
    from shrimp_amd import synth
    n = len(hits); L = reads.shape[1]
    rw = np.ascontiguousarray(synth.pack_reads(reads))[hits["read"]]; lens = np.full(n, L)
    ts.full_setup(gm, p); ts.vector_setup(gm, p)
    thresh = np.array([int(ts.abs_or_pct(p.sw_full_threshold, sm)) for sm in hits["score_max"]], dtype=np.int32)
    anchors = [(int(h["ax"]), int(h["ay"]), int(h["alen"]), int(h["awidth"])) for h in hits]
    cn, gst, goff, wl = hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"]
    sv = ix.sw_vector_batch(cn, gst, goff, wl, rw, lens)
    recs, ops, _ = ix.sw_full_ls_batch(cn, gst, goff, wl, rw, lens, anchors=anchors, revcmpl=(hits["gen_st"] == 1).astype(np.uint8), threshscore=thresh, maxscore=sv)
    recs = recs.copy(); recs["score"][sv < thresh] = 0
    maps, map_off = s.select_pass2(hits, hit_off, recs, None)
    status, _, _, cigar, edit = ix.sw_full_batch_text(cn, gst, recs, ops, rw, lens, reverse=(hits["gen_st"] == 1).astype(np.uint8), clip="S", what=("cigar", "edit"),
                                                      colour_space=False)
    assert (status == 0).all()
    got, off = s.sam_records(reads, hits, recs, maps, map_off, cigar, score_vector=sv)
    return [got[int(off[r]):int(off[r + 1])] for r in range(len(reads))]


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [True, False])
def test_the_chain_from_read_hits_ends_in_the_bytes_of_the_reference(gm, cache):
    """f1_twins_60bp: the session default gives the reference's default output read by read, hash_filter_calls = 0 its output under -Z; gm_map_reads agrees"""
    ix, s, p, reads = open_twins(gm) if cache else open_twins(gm, hash_filter_calls=0)
    contigs, _, sam = oa.load_golden(TWINS)
    if not cache: sam = oa.load_option_sam(TWINS, "no_cache")
    want = by_read(sam)
    hits, hit_off = s.read_hits(reads)
    mine = chain_to_sam(gm, ix, s, p, reads, hits, hit_off)
    bad = [r for r in range(len(reads)) if mine[r] != b"".join(want.get(r, []))]
    assert not bad, (len(bad), [(mine[r], want.get(r)) for r in bad[:3]])
    assert sum(1 for m in mine if m) == (251 if cache else 300)
    assert oa.sam_header(contigs) + s.map_reads(reads) == sam


@pytest.mark.gpu
def test_every_refusal_is_followed_by_a_good_call(gm, driver):
    F = ts.reference(driver, "cfg2s_100bp_2Mbp")
    ix, s, p, reads = opened(gm, "cfg2s_100bp_2Mbp")
    cix, cs_, cp, creads = opened(gm, "cfg4s_50col_2Mbp")
    wins = ts.as_wins(gm, F["rows"]); off = F["off"]; n = len(reads)
    good_scores, good_slots = s.score_windows(reads, wins, off)
    good_hits, good_off = s.select_pass1(wins, off, good_scores, slots=good_slots)

    def refused(call, code, word):
        with pytest.raises(gm.GmError) as e: call()
        assert "(%d)" % code in str(e.value) and word in str(e.value), str(e.value)
        a, b = s.score_windows(reads, wins, off)                         # the session serves the next call
        assert np.array_equal(a, good_scores) and np.array_equal(b, good_slots)
    L = gm.lib(); u32p, u64p, ipt = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    from shrimp_amd import synth
    packed = np.ascontiguousarray(synth.pack_reads(reads), dtype=np.uint32)
    rd = packed.ctypes.data_as(u32p); wp = wins.ctypes.data_as(C.c_void_p); op = off.ctypes.data_as(u64p)
    hit_off = np.zeros(n + 1, dtype=np.uint64); out = C.c_void_p(); nh = C.c_uint64(); wout = C.c_void_p(); nw = C.c_uint64()

    raw = lambda rc, what: (lambda: gm._check(rc(), what))              # the C entries themselves, where the Python methods cannot make the call
    # NULL outputs
    refused(raw(lambda: L.gm_score_windows(s.h, n, 100, rd, None, wp, len(wins), op, None, None), "gm_score_windows"), GM_E_ARG, "bad arguments")
    refused(raw(lambda: L.gm_select_pass1_f1(s.h, n, 100, wp, len(wins), op, good_scores.ctypes.data_as(ipt), good_slots.ctypes.data_as(u32p), None, C.byref(nh),
                                             hit_off.ctypes.data_as(u64p), None), "gm_select_pass1_f1"), GM_E_ARG, "bad arguments")
    refused(raw(lambda: L.gm_read_hits(s.h, n, 100, rd, None, None, C.byref(nh), hit_off.ctypes.data_as(u64p), None, None, None, None, None), "gm_read_hits"), GM_E_ARG, "bad arguments")
    # the four optional outputs of read_hits given only in part
    refused(raw(lambda: L.gm_read_hits(s.h, n, 100, rd, None, C.byref(out), C.byref(nh), hit_off.ctypes.data_as(u64p), C.byref(wout), C.byref(nw), None, None, None),
                "gm_read_hits"), GM_E_ARG, "together")
    # offsets, windows
    bad_off = off.copy(); bad_off[5], bad_off[6] = off[6] + 1, off[5]
    short = off.copy(); short[-1] -= 1
    for call_of in (lambda w, o: s.score_windows(reads, w, o), lambda w, o: s.select_pass1(w, o, good_scores, slots=good_slots)):
        refused(lambda: call_of(wins, bad_off), GM_E_ARG, "ascending")
        refused(lambda: call_of(wins, short), GM_E_ARG, "offsets run")
        for field, value, word in (("read", 7, "says read"), ("st", 1 - int(wins["st"][0]), "says read"), ("cn", len(F["contigs"]), "contig"), ("cn", -1, "contig"),
                                   ("w_len", 0, "w_len"), ("g_off", 2 ** 31, "beyond contig"), ("g_off", int(F["clen"][wins["cn"][0]]) - int(wins["w_len"][0]) + 1, "beyond contig")):
            w = wins.copy(); w[field][0] = value
            refused(lambda: call_of(w, off), GM_E_ARG, word)
    # initbp missing or spurious; a read length out of range
    refused(lambda: s.score_windows(reads, wins, off, initbp=np.zeros(n, dtype=np.uint8)), GM_E_ARG, "colour-space")
    refused(lambda: s.read_hits(reads, initbp=np.zeros(n, dtype=np.uint8)), GM_E_ARG, "colour-space")
    refused(lambda: cs_.read_hits(np.ascontiguousarray(creads[:, 1:])), GM_E_ARG, "initbp")
    refused(lambda: cs_.score_windows(np.ascontiguousarray(creads[:, 1:]), wins[:0], np.zeros(2 * len(creads) + 1, dtype=np.uint64)), GM_E_ARG, "initbp")
    refused(lambda: s.read_hits(np.zeros((4, s.params.longest_read_len + 1), dtype=np.uint8)), GM_E_RANGE, "out of range")
    # num_tmp_outputs = 65
    s65 = gm.Session(ix, params=ts.params_of(gm, "cfg2s_100bp_2Mbp", num_tmp_outputs=65), max_batch_reads=1024)
    for call in (lambda: s65.read_hits(reads), lambda: s65.select_pass1(wins, off, good_scores, 100, slots=good_slots)):
        with pytest.raises(gm.GmError) as e: call()
        assert "(%d)" % GM_E_RANGE in str(e.value) and "num_tmp_outputs" in str(e.value)
    a, _ = s65.score_windows(reads, wins, off)                           # (scoring does not select)
    assert np.array_equal(a, good_scores)
    s65.close()
    # empty calls, then the good ones again
    e, eo = s.read_hits(np.zeros((0, 100), dtype=np.uint8))
    assert len(e) == 0 and e.dtype == gm.PASS1_HIT_DTYPE and eo.tolist() == [0]
    h, ho = s.select_pass1(wins, off, good_scores, slots=good_slots)
    assert np.array_equal(h, good_hits) and np.array_equal(ho, good_off)
    h, ho = s.read_hits(reads)
    assert np.array_equal(ho, good_off) and len(h) == len(good_hits)
