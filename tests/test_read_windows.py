"""gm_read_windows (Session.read_windows): the candidate windows of a read batch -- every window read_get_hit_list_per_strand yields for each read on each strand,
before pass 1 -- as a tight array with 2 n + 1 offsets.

What the windows are compared with: tests/read_windows_oracle.cpp, a driver over the CPU restatement (oracle/gm_oracle.hpp) that runs the read loop up to
read_get_hit_list and dumps both lists.  It is compiled here, with the flags of oracle/Makefile, into pytest's temporary directory.  The driver itself is pinned to
the REFERENCE without a GPU: the three goldens written with --extra-sam-fields carry, per mapped record, the window's match count (ZM), its window-generation score
(ZR) and its vector score (ZV); every such record must have a window of its read and strand on its contig that covers the alignment and carries ZM and ZR, and
scoring that window at the address the header gives (strand 1: the reverse-complement contig, the read as given) must give ZV.  The GPU tests then hold the library to
the driver row by row, and to the goldens directly with the library's own vector kernel on the resident index.

Equal (read, st, cn, g_off) windows exist (33 groups on stress_60bp): the reference keeps them in anchor order, pass 1 cannot tell them apart, and the header promises
(cn, g_off) order only -- so rows are compared after ordering such groups by the whole record."""
import ctypes as C
import gzip, os, re, subprocess
import numpy as np
import pytest
from tests import oracle_api as oa

# fixture -> (match mode, colour space, windows, most on one read-strand, groups of equal (read, st, cn, g_off)): the driver's counts
FIXTURES = {
    "cfg2s_100bp_2Mbp": (2, False, 5575, 3, 0),
    "stress_60bp": (2, False, 5586, 283, 33),
    "n1_noisy_70bp": (1, False, 53830, 17, 0),
    "cfg4s_50col_2Mbp": (2, True, 3302, 3, 0),
}
# golden with --extra-sam-fields -> (fixture, mapped records)
GOLDENS = {"cfg2s_100bp_2Mbp@extra_fields": ("cfg2s_100bp_2Mbp", 5000), "n1_noisy_70bp@extra_fields_rg_unal": ("n1_noisy_70bp", 3887),
           "cfg4s_50col_2Mbp@cs_extra_rg": ("cfg4s_50col_2Mbp", 2942)}
COLS = ("read", "st", "cn", "g_off", "w_len", "score_window_gen", "matches", "ax", "ay", "alen", "awidth", "reserved")
GM_E_ARG, GM_E_RANGE = -2, -4
CMPL = np.array([3, 2, 1, 0, 0, 10, 9, 7, 8, 6, 5, 14, 13, 12, 11, 15], dtype=np.uint8)      # complement_base (A C G T U M R W S Y K V H D B N)
THREADS = max(1, min(8, os.cpu_count() or 1))


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------------------
def offsets(rows, n):
    """rows come read by read, strand 0 then 1: -> off[2 n + 1]"""
    key = rows[:, 0] * 2 + rows[:, 1]
    assert (np.diff(key) >= 0).all()
    return np.searchsorted(key, np.arange(2 * n + 1)).astype(np.uint64)


def in_list_order(rows):
    """every read-strand ascending in (cn, g_off)"""
    same = (rows[1:, 0] == rows[:-1, 0]) & (rows[1:, 1] == rows[:-1, 1])
    up = (rows[1:, 2] > rows[:-1, 2]) | ((rows[1:, 2] == rows[:-1, 2]) & (rows[1:, 3] >= rows[:-1, 3]))
    return bool((up | ~same).all())


def canon(rows):
    """groups of equal (read, st, cn, g_off) ordered by the rest of the record; a list in (cn, g_off) order keeps every other row where it is"""
    return rows[np.lexsort(rows.T[::-1])]


def tie_groups(rows):
    c = canon(rows); eq = (c[1:, :4] == c[:-1, :4]).all(axis=1)
    return int((eq & ~np.concatenate([[False], eq[:-1]])).sum())


def as_rows(wins):
    return np.stack([wins[c].astype(np.int64) for c in COLS], axis=1) if len(wins) else np.zeros((0, 12), dtype=np.int64)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rwo") / "librwo.so")
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", open(os.path.join(oa.ROOT, "oracle", "Makefile")).read(), re.M).group(1).split()
    r = subprocess.run(["g++", *flags, "-shared", "-fPIC", "-I", os.path.join(oa.ROOT, "oracle"), "-o", so, os.path.join(oa.ROOT, "tests", "read_windows_oracle.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(so)
    u8p = C.POINTER(C.c_uint8)
    L.rwo_create.argtypes = [C.c_int, C.POINTER(u8p), C.POINTER(C.c_uint64), C.c_int, C.c_int]; L.rwo_create.restype = C.c_void_p
    L.rwo_destroy.argtypes = [C.c_void_p]
    L.rwo_windows.argtypes = [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int, C.POINTER(C.c_longlong), C.c_long]; L.rwo_windows.restype = C.c_long
    return L


_drv = {}


def driver_rows(L, name):
    """(contigs, reads, rows, off) of a fixture: the driver's windows, computed once"""
    if name not in _drv:
        mode, colour = FIXTURES[name][:2]
        contigs, reads, _ = oa.load_golden(name)
        cs = [np.ascontiguousarray(c, dtype=np.uint8) for c in contigs]; reads = np.ascontiguousarray(reads, dtype=np.uint8)
        u8p = C.POINTER(C.c_uint8)
        h = L.rwo_create(len(cs), (u8p * len(cs))(*[c.ctypes.data_as(u8p) for c in cs]), (C.c_uint64 * len(cs))(*[len(c) for c in cs]), int(colour), mode)
        cap = 64 * len(reads); rows = np.zeros((cap, 12), dtype=np.int64)
        w = L.rwo_windows(h, reads.shape[0], reads.shape[1], reads.ctypes.data_as(u8p), THREADS, rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
        L.rwo_destroy(h)
        assert 0 < w <= cap
        _drv[name] = (cs, reads, rows[:w].copy(), offsets(rows[:w], len(reads)))
    return _drv[name]


# ---- the reference's records ------------------------------------------------------------------------------------------------------------------------------------
def records(golden):
    """mapped records of a golden: (read, st, cn, pos, reference span, ZM, ZR, ZV)"""
    out = []
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", golden + ".sam.gz"), "rt") as f:
        for line in f:
            if line.startswith("@"): continue
            t = line.rstrip("\n").split("\t")
            if int(t[1]) & 4: continue
            tags = {x[:2]: x[5:] for x in t[11:]}
            span = sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", t[5]) if op in "MD")
            out.append((int(t[0][1:]), 1 if int(t[1]) & 16 else 0, int(t[2][len("contig"):]) - 1, int(t[3]) - 1, span, int(tags["ZM"]), int(tags["ZR"]), int(tags["ZV"])))
    return out


def candidates(rows, off, recs):
    """per record: the windows of its read and strand on its contig that cover the alignment and carry its ZM and ZR -- at least one each"""
    cands, missing = [], []
    for k, (rd, st, cn, pos, span, zm, zr, _) in enumerate(recs):
        a, b = int(off[2 * rd + st]), int(off[2 * rd + st + 1]); w = rows[a:b]
        ok = (w[:, 2] == cn) & (w[:, 3] <= pos) & (pos + span <= w[:, 3] + w[:, 4]) & (w[:, 6] == zm) & (w[:, 5] == zr)
        cands.append(a + np.nonzero(ok)[0])
        if not ok.any(): missing.append(k)
    assert not missing, (len(missing), [recs[k] for k in missing[:5]])
    return cands


def pack(codes):
    from shrimp_amd import synth
    return synth.pack_nibbles(np.asarray(codes, dtype=np.uint8))


def colours(letters):
    """colour i between letters i - 1 and i, the first against T; 15 where either letter is above 3"""
    a = np.concatenate([[3], letters[:-1]]).astype(np.int64); b = letters.astype(np.int64)
    return np.where((a > 3) | (b > 3), 15, a ^ b).astype(np.uint8)


def header_address(rows, clen):
    """a window as the header says it feeds the _ix seams: (gen_st, offset on that strand's contig); strand 1 is what reverse_hit makes of it"""
    st = rows[:, 1]
    return st, np.where(st == 0, rows[:, 3], clen[rows[:, 2]] - rows[:, 3] - rows[:, 4])


def some_candidate_gives_zv(recs, cands, scores_of):
    """scores_of(window indices, read of each) -> vector scores; every record needs one candidate with its ZV"""
    idx = np.concatenate(cands); who = np.concatenate([np.full(len(c), k) for k, c in enumerate(cands)])
    got = scores_of(idx, np.array([recs[k][0] for k in who]))
    hit = np.zeros(len(recs), dtype=bool); hit[who[got == np.array([recs[k][7] for k in who])]] = True
    assert hit.all(), (int((~hit).sum()), [recs[k] for k in np.nonzero(~hit)[0][:5]])


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_and_its_record_size():
    """fails without the feature"""
    from shrimp_amd import gmapper as gm
    L = gm.lib()
    assert hasattr(L, "gm_read_windows") and hasattr(L, "gm_read_window_size")
    assert "gm_read_windows" in gm.EXPORTS and "gm_read_window_size" in gm.EXPORTS
    assert L.gm_read_window_size() == 48 == C.sizeof(gm.ReadWindow) == gm.READ_WINDOW_DTYPE.itemsize
    assert gm.READ_WINDOW_DTYPE.names == COLS
    assert [gm.READ_WINDOW_DTYPE.fields[c][1] for c in COLS] == list(range(0, 48, 4))
    assert L.gm_abi_sizeof(6) == -1                      # the list of gm_abi_sizeof stays 0..5: the record has its own size function


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_driver_lists_are_ordered_and_counted(driver, name):
    """every list ascending in (cn, g_off); windows, the longest list and the groups of equal (read, st, cn, g_off) as counted when the driver was written"""
    _, reads, rows, off = driver_rows(driver, name)
    assert in_list_order(rows) and (rows[:, 11] == 0).all()
    per = np.diff(off.astype(np.int64))
    assert (len(rows), int(per.max()), tie_groups(rows)) == FIXTURES[name][2:]
    if name == "stress_60bp": assert int((per > 64).sum()) == 2


@pytest.mark.parametrize("golden", sorted(GOLDENS))
def test_driver_windows_carry_the_reference_records(driver, golden):
    """ZM and ZR of every mapped record of the reference's own output, on a window that covers the alignment"""
    name, n_mapped = GOLDENS[golden]
    _, _, rows, off = driver_rows(driver, name)
    recs = records(golden)
    assert len(recs) == n_mapped
    candidates(rows, off, recs)


@pytest.mark.parametrize("golden", sorted(GOLDENS))
def test_driver_windows_at_the_header_address_give_zv(driver, oracle_lib, golden):
    """the oracle's vector filter on (cn, gen_st, offset on that strand, w_len) with the read as given == ZV, for some candidate window of every record (one letter-space
    record has two).  Colour space: the colour contig and the letter contig of the strand, the read's colours and primer."""
    name, _ = GOLDENS[golden]
    colour = FIXTURES[name][1]
    contigs, reads, rows, off = driver_rows(driver, name)
    recs = records(golden); cands = candidates(rows, off, recs)
    clen = np.array([len(c) for c in contigs], dtype=np.int64)
    letters = [[c, CMPL[c[::-1]]] for c in contigs]
    ls = [[pack(x) for x in pair] for pair in letters]
    cs = [[pack(colours(x)) for x in pair] for pair in letters] if colour else None
    rw = [pack(r[1:] if colour else r) for r in reads]; rlen = reads.shape[1] - (1 if colour else 0)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def scores_of(idx, rd):
        st, goff = header_address(rows[idx], clen)
        out = np.zeros(len(idx), dtype=np.int64)
        for k, (i, r) in enumerate(zip(idx, rd)):
            cn, wl = int(rows[i, 2]), int(rows[i, 4])
            if colour: out[k] = oracle_lib.gmo_sw_vector_cs(u32(cs[cn][st[k]]), int(goff[k]), wl, u32(rw[r]), rlen, u32(ls[cn][st[k]]), int(reads[r, 0]))
            else: out[k] = oracle_lib.gmo_sw_vector(u32(ls[cn][st[k]]), int(goff[k]), wl, u32(rw[r]), rlen)
        return out
    some_candidate_gives_zv(recs, cands, scores_of)


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------------
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


def params_of(gm, name):
    mode, colour = FIXTURES[name][:2]
    p = gm.default_params_cs() if colour else gm.default_params()
    p.match_mode = mode
    return p


def open_session(gm, name, max_batch_reads=None):
    contigs, reads, _ = oa.load_golden(name)
    p = params_of(gm, name)
    if max_batch_reads is None: max_batch_reads = {"n1_noisy_70bp": 4096, "stress_60bp": 8192}.get(name, 131072)
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p, max_batch_reads=max_batch_reads)
    return ix, s, p, np.ascontiguousarray(reads, dtype=np.uint8)


def read_windows(s, name, reads):
    return s.read_windows(reads[:, 1:], initbp=reads[:, 0]) if FIXTURES[name][1] else s.read_windows(reads)


_lib = {}


def library_rows(gm, name):
    """(ix, session, params, reads, rows, off, stats) of a fixture: one Session.read_windows call, made once (the index and the session stay open for the module)"""
    if name not in _lib:
        ix, s, p, reads = open_session(gm, name)
        wins, off = read_windows(s, name, reads)
        assert wins.dtype == gm.READ_WINDOW_DTYPE and off.dtype == np.uint64 and off.shape == (2 * len(reads) + 1,)
        _lib[name] = (ix, s, p, reads, as_rows(wins), off, dict(s.stats))
    return _lib[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_read_windows_equal_the_driver(gm, driver, name):
    _, _, want, want_off = driver_rows(driver, name)
    _, _, _, reads, rows, off, stats = library_rows(gm, name)
    assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all() and int(off[-1]) == len(rows)
    assert np.array_equal(off, offsets(rows, len(reads)))            # the records' own (read, st) say what the offsets say
    assert in_list_order(rows) and (rows[:, 11] == 0).all()
    assert stats["windows"] == len(rows) and stats["reads"] == len(reads)
    assert np.array_equal(off, want_off), np.nonzero(off != want_off)[0][:10]
    a, b = canon(rows), canon(want)
    assert np.array_equal(a, b), (a[(a != b).any(axis=1)][:5], b[(a != b).any(axis=1)][:5])


@pytest.mark.gpu
def test_sub_batches_and_a_capacity_growth(gm):
    """stress_60bp, 3 000 reads through sub-batches of 1 024: three of them, and rows of 64 windows that two read-strands overflow (283 on one)"""
    _, _, _, reads, want, want_off, _ = library_rows(gm, "stress_60bp")
    ix, s, _, _ = open_session(gm, "stress_60bp", max_batch_reads=1024)
    wins, off = s.read_windows(reads)
    stats = dict(s.stats)
    s.close(); ix.close()
    assert stats["retries"] >= 1 and stats["windows"] == len(wins) == len(want) and stats["reads"] == len(reads)
    assert np.array_equal(off, want_off)
    assert np.array_equal(canon(as_rows(wins)), canon(want))


@pytest.mark.gpu
@pytest.mark.parametrize("golden", sorted(GOLDENS))
def test_library_windows_carry_the_reference_records_and_give_zv(gm, golden):
    """the driver's two CPU checks with the library in its place: windows from read_windows, ZV from gm_sw_vector_batch_ix on the resident index at the address the
    header gives, under the session's scores (colour space: mismatch = match + crossover, the reads' primers)"""
    name, n_mapped = GOLDENS[golden]
    colour = FIXTURES[name][1]
    ix, _, p, reads, rows, off, _ = library_rows(gm, name)
    recs = records(golden)
    assert len(recs) == n_mapped
    cands = candidates(rows, off, recs)
    from shrimp_amd import synth
    body = np.ascontiguousarray(reads[:, 1:]) if colour else reads
    rw = np.ascontiguousarray(synth.pack_reads(body)); clen = ix.contig_lengths()
    gm.sw_vector_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score,
                       p.match_score + p.crossover_score if colour else p.mismatch_score, 1 if colour else 0, True)

    def scores_of(idx, rd):
        st, goff = header_address(rows[idx], clen)
        return ix.sw_vector_batch(rows[idx, 2], st.astype(np.uint8), goff, rows[idx, 4], rw[rd], np.full(len(idx), body.shape[1]), initbp=reads[rd, 0] if colour else None)
    some_candidate_gives_zv(recs, cands, scores_of)


@pytest.mark.gpu
def test_every_row_of_tophits_is_a_window(gm):
    _, s, _, reads, rows, _, _ = library_rows(gm, "stress_60bp")
    top = s.tophits(reads)                                           # read st cn g_off w_len score_vector pct_score_vector matches ax ay alen awidth
    assert len(top) >= len(reads) // 2
    have = set(map(tuple, rows[:, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]].tolist()))
    lost = [t for t in map(tuple, top[:, [0, 1, 2, 3, 4, 7, 8, 9, 10, 11]].tolist()) if t not in have]
    assert not lost, (len(lost), lost[:5])


@pytest.mark.gpu
def test_state_and_reuse(gm):
    """read_windows between mapping calls on one session: the SAM is the golden's, a second read_windows answer is the first, a call at another read length in
    between changes neither"""
    contigs, reads, sam = oa.load_golden("cfg2s_100bp_2Mbp")
    ix, s, _, reads = open_session(gm, "cfg2s_100bp_2Mbp")
    w1, o1 = s.read_windows(reads); st1 = dict(s.stats)
    assert oa.sam_header(contigs) + s.map_reads(reads) == sam
    assert s.stats["windows"] == st1["windows"] == len(w1) and s.stats["anchors"] == st1["anchors"] and s.stats["survivors"] == st1["survivors"]
    w80, o80 = s.read_windows(np.ascontiguousarray(reads[:700, 10:90]))
    assert len(w80) > 0 and int(o80[-1]) == len(w80) and (w80["read"] < 700).all()
    w2, o2 = s.read_windows(reads)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2)
    assert oa.sam_header(contigs) + s.map_reads(reads) == sam
    s.close(); ix.close()


@pytest.mark.gpu
def test_refusals_leave_the_session_usable(gm):
    ix, s, _, reads, want, want_off, _ = library_rows(gm, "cfg2s_100bp_2Mbp")
    cix, cs_, _, creads, cwant, cwant_off, _ = library_rows(gm, "cfg4s_50col_2Mbp")
    cols, primers = np.ascontiguousarray(creads[:, 1:]), np.ascontiguousarray(creads[:, 0])
    bad = primers.copy(); bad[17] = 4
    for call, code, word in ((lambda: s.read_windows(reads, initbp=np.zeros(len(reads), dtype=np.uint8)), GM_E_ARG, "colour-space"),
                             (lambda: cs_.read_windows(cols), GM_E_ARG, "initbp"),
                             (lambda: cs_.read_windows(cols, initbp=bad), GM_E_ARG, "read 17"),
                             (lambda: s.read_windows(np.zeros((4, s.params.longest_read_len + 1), dtype=np.uint8)), GM_E_RANGE, "out of range")):
        with pytest.raises(gm.GmError) as e: call()
        assert "(%d)" % code in str(e.value) and word in str(e.value), str(e.value)
    wins, off = s.read_windows(np.zeros((0, 100), dtype=np.uint8))
    assert len(wins) == 0 and wins.dtype == gm.READ_WINDOW_DTYPE and off.tolist() == [0] and s.stats["windows"] == 0
    wins, off = s.read_windows(reads)
    assert np.array_equal(off, want_off) and np.array_equal(canon(as_rows(wins)), canon(want))
    wins, off = cs_.read_windows(cols, initbp=primers)
    assert np.array_equal(off, cwant_off) and np.array_equal(canon(as_rows(wins)), canon(cwant))
