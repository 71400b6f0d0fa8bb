"""The batch seams on the resident index (gm_index_get_windows, gm_sw_vector_batch[_bounded]_ix, gm_sw_gapless_batch_ix, gm_sw_full_ls/cs_batch_ix,
gm_post_sw_batch_ix): windows addressed as the reference addresses them -- contig, strand, offset -- and read from the index's own genome.

How the fixtures become an index: the known-answer records carry a little bitfield each.  lay_out() unpacks them, lays the items of a set end to end into five
contigs (a random lead of 1-7 bases and a tail each, so that no contig length and no global contig start is a multiple of 8) and an Index is built from those; item k
is then (cn_k, 0, base_k + goff_k, glen_k).  For strand 1 a second index holds the reverse complements of the five contigs (numpy, the 16-entry complement table):
its strand 1 is the first index's strand 0, so item k is (cn_k, 1, base_k + goff_k, glen_k) there.  The table is an involution on every code but U, so items that
hold a U stay out of that leg.  The expected answers are the fixture's own on both strands (genome_start less base_k): nothing in them comes from the code under
test.  sw_gapless scores against the whole contig, so its records get a contig each."""
import ctypes as C
import gzip, os, struct, subprocess, sys, threading
import numpy as np
import pytest
from tests import oracle_api as oa
from tests.test_sw_full_batch import LS_SETUP, CS_SETUP, items_F, items_local, items_cs, check_ls, check_cs
from tests import test_post_sw_batch as tp

CMPL = np.array([3, 2, 1, 0, 0, 10, 9, 7, 8, 6, 5, 14, 13, 12, 11, 15], dtype=np.uint8)      # complement_base (A C G T U M R W S Y K V H D B N)
IX_SYMBOLS = ["gm_index_genome_is_rna", "gm_index_get_windows", "gm_sw_vector_batch_ix", "gm_sw_vector_batch_bounded_ix", "gm_sw_gapless_batch_ix", "gm_sw_full_ls_batch_ix",
              "gm_sw_full_cs_batch_ix", "gm_post_sw_batch_ix"]
GM_E_ARG, GM_E_NOTSETUP = -2, -3


# ---- numpy statements of the two strands and of the colour translation ---------------------------------------------------------------------------------
def unpack(words, n=None):
    w = np.asarray(words, dtype=np.uint32)
    c = ((w[:, None] >> (4 * np.arange(8, dtype=np.uint32))) & 0xf).astype(np.uint8).ravel()
    return c if n is None else c[:n]


def pack(codes):
    from shrimp_amd import synth
    return synth.pack_nibbles(np.asarray(codes, dtype=np.uint8))


def is_rna(contig):
    """uracil and no thymine"""
    return bool((contig == 4).any() and not (contig == 3).any())


def revcomp(contig, rna=None):
    rna = is_rna(contig) if rna is None else rna
    out = CMPL[contig[::-1]]
    if rna: out = np.where(out == 3, 4, out).astype(np.uint8)
    return out


def colours(letters, rna):
    """colour i between letters i - 1 and i, the first against T; 15 where either letter is above 3; U as T on an RNA contig"""
    a = np.concatenate([[3], letters[:-1]]).astype(np.int64); b = letters.astype(np.int64)
    if rna: a = np.where(a == 4, 3, a); b = np.where(b == 4, 3, b)
    return np.where((a > 3) | (b > 3), 15, a ^ b).astype(np.uint8)


def strand_contig(contig, st):
    """letters and colours of strand st of a contig, as genome_contigs[_rc] / genome_cs_contigs[_rc] hold them (the contig's own RNA flag decides both)"""
    rna = is_rna(contig)
    let = contig if st == 0 else revcomp(contig, rna)
    return let, colours(let, rna)


def mirror(clen, off, glen):
    """the Python statement of Index.strand_offset"""
    return clen - off - glen


# ---- fixtures -> contigs ---------------------------------------------------------------------------------------------------------------------------------
def lay_out(bitfields, n_contigs=5, seed=20261018):
    """-> (contigs, cn[k], base[k]): item k's codes start at position base[k] of contig cn[k]"""
    rng = np.random.default_rng(seed)
    codes = [unpack(g) for g in bitfields]
    per = (len(codes) + n_contigs - 1) // n_contigs
    contigs, cn, base, start = [], [], [], 0
    for c in range(n_contigs):
        part = codes[c * per:(c + 1) * per]
        lead = rng.integers(0, 4, size=int(rng.integers(1, 8)), dtype=np.uint8)
        pos = len(lead)
        for x in part: cn.append(c); base.append(pos); pos += len(x)
        tail = 1
        while (pos + tail) % 8 == 0 or (start + pos + tail) % 8 == 0: tail += 1
        contigs.append(np.concatenate([lead] + part + [rng.integers(0, 4, size=tail, dtype=np.uint8)]))
        assert len(contigs[-1]) % 8 != 0 and (c == 0 or start % 8 != 0)
        start += len(contigs[-1])
    return contigs, np.array(cn, dtype=np.int32), np.array(base, dtype=np.int64)


def no_u(bitfield):
    return not (unpack(bitfield) == 4).any()


class IndexPair:
    """[0]: the index of the contigs, [1]: the index of their reverse complements (each built at its first use), [2]: the contigs, [3]: cn[k], [4]: base[k]"""
    def __init__(self, gm, contigs, cn, base, colour):
        self.gm, self.colour, self.built, self.rest = gm, colour, {}, (contigs, cn, base)

    def __getitem__(self, k):
        if k >= 2: return self.rest[k - 2]
        if k not in self.built:
            contigs = self.rest[0] if k == 0 else [revcomp(c) for c in self.rest[0]]
            self.built[k] = self.gm.Index(contigs, params=self.gm.default_params_cs() if self.colour else None)
        return self.built[k]

    def close(self):
        for ix in self.built.values(): ix.close()


_idx = {}


def indexes(gm, key, bitfields, colour=False, per_item=False):
    """the IndexPair of a fixture set, built once per module.  per_item: a contig per (bitfield, length)"""
    if key not in _idx:
        if per_item: contigs = [unpack(g, n) for g, n in bitfields]; cn = np.arange(len(contigs), dtype=np.int32); base = np.zeros(len(contigs), dtype=np.int64)
        else: contigs, cn, base = lay_out(bitfields)
        _idx[key] = IndexPair(gm, contigs, cn, base, colour)
    return _idx[key]


def reads_matrix(reads, rlens):
    rw = max(max(len(r) for r in reads), max((int(n) + 7) // 8 for n in rlens))
    out = np.zeros((len(reads), rw), dtype=np.uint32)
    for i, r in enumerate(reads): out[i, :len(r)] = r
    return out


def arrays(items):
    d = {k: np.array([it[k] for it in items], dtype=np.int64) for k in ("goff", "glen", "rlen", "rv", "thresh", "maxscore", "initbp")}
    d["reads"] = reads_matrix([it["r"] for it in items], d["rlen"])
    d["anchors"] = np.array([it["anchor"] if it["anchor"] is not None else (0, 0, 0, 0) for it in items], dtype=np.int64)
    d["xs"] = None
    if any(it["xs"] is not None for it in items):
        d["xs"] = np.zeros((len(items), int(d["rlen"].max())), dtype=np.int32)
        for i, it in enumerate(items): d["xs"][i, :it["rlen"]] = it["xs"][:it["rlen"]]
    return d


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
    for v in _idx.values(): v.close()
    _idx.clear()


# ---- 1: get_windows against numpy ------------------------------------------------------------------------------------------------------------------------
def genome7(seed=7):
    """seven contigs with all 16 codes: of 1, 5, 8 and 9 bases among them, one DNA contig with a U, one RNA contig (U, no T) that is not the last"""
    rng = np.random.default_rng(seed)
    def rnd(n):
        c = rng.integers(0, 4, size=n, dtype=np.uint8)
        amb = rng.random(n) < 0.05
        return np.where(amb, rng.integers(5, 16, size=n), c).astype(np.uint8)
    c0 = rnd(1203); c0[:16] = np.arange(16); c0[100] = 4                                  # DNA with a U (and T)
    c1 = np.array([2], dtype=np.uint8)
    c2 = rnd(5)
    r = rnd(997); r = np.where(r == 3, 4, r).astype(np.uint8); r[5] = 4                   # RNA: U, no T
    c4 = rnd(8); c5 = rnd(9)
    c6 = rnd(2011)
    cs = [c0, c1, c2, r, c4, c5, c6]
    assert is_rna(cs[3]) and not is_rna(cs[0]) and (cs[0] == 4).any() and not is_rna(cs[-1])
    assert set(np.concatenate(cs).tolist()) == set(range(16))
    return cs


def window_cases(contigs, n_random, seed):
    rng = np.random.default_rng(seed)
    lens = np.array([len(c) for c in contigs]); starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rows = []
    for _ in range(n_random):
        c = int(rng.integers(0, len(contigs))); st = int(rng.integers(0, 2))
        gl = int(rng.integers(1, min(300, lens[c]) + 1)); off = int(rng.integers(0, lens[c] - gl + 1))
        rows.append((c, st, off, gl))
    for st in (0, 1):
        for c in range(len(contigs)): rows.append((c, st, 0, int(lens[c])) if lens[c] <= 9 else (c, st, 0, 17))      # small contigs whole; offset 0 everywhere
        for c in (0, len(contigs) - 1):                                                                               # the first and the last contig
            rows.append((c, st, int(lens[c]) - 31, 31))                                                               # ... ending at the contig's last base
            for gl in (63, 64, 65): rows.append((c, st, 11, gl)); rows.append((c, st, int(lens[c]) - gl, gl))
        for c in (0, 3, 6):                                                                                           # 2 positions whose forward start is 7 mod 8
            f = next(f for f in range(40, 60) if (starts[c] + f) % 8 == 7)
            rows.append((c, st, f if st == 0 else mirror(int(lens[c]), f, 2), 2))
    a = np.array(rows, dtype=np.int64)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.uint8), a[:, 2], a[:, 3].astype(np.int32)


def expected_windows(contigs, cn, st, off, glen, colour):
    strands = {(c, s): strand_contig(contigs[c], s) for c in range(len(contigs)) for s in (0, 1)}
    return [strands[(int(c), int(s))][1 if colour else 0][int(o):int(o) + int(g)] for c, s, o, g in zip(cn, st, off, glen)]


@pytest.mark.gpu
def test_get_windows_against_numpy(gm):
    contigs = genome7()
    cn, st, off, glen = window_cases(contigs, 2000, 1)
    for colour in (False, True):
        ix = gm.Index(contigs, params=gm.default_params_cs() if colour else None)
        assert list(ix.contig_lengths()) == [len(c) for c in contigs] and ix.genome_is_rna() is False      # (the flag of the LAST contig)
        for col in ((False, True) if colour else (False,)):
            got = ix.get_windows(cn, st, off, glen, colours=col)
            want = expected_windows(contigs, cn, st, off, glen, col)
            for k in range(len(cn)):
                g = unpack(got[k])
                assert np.array_equal(g[:glen[k]], want[k]) and not g[glen[k]:].any(), (colour, col, k, cn[k], st[k], off[k], glen[k], g[:glen[k]], want[k])
        ix.close()
    ix = gm.Index([contigs[0], contigs[3]])                                   # the RNA contig last
    assert ix.genome_is_rna() is True
    ix.close()


# ---- 2 / 10: sw_full_ls ----------------------------------------------------------------------------------------------------------------------------------
def run_full_ls(gm, key, items, local, order=None, strands=(0, 1)):
    gm.sw_full_ls_setup(*LS_SETUP)
    for st in strands:
        its = items if st == 0 else [it for it in items if no_u(it["g"])]
        assert len(its) >= 0.9 * len(items)
        ix = indexes(gm, (key, st > 0), [it["g"] for it in its])
        a = arrays(its); o = np.arange(len(its)) if order is None else order(len(its))
        recs, ops, strings = ix[st].sw_full_ls_batch(ix[3][o], np.full(len(o), st, dtype=np.uint8), (ix[4] + a["goff"])[o], a["glen"][o], a["reads"][o], a["rlen"][o],
                                                     a["anchors"][o], a["rv"][o], a["thresh"][o], a["maxscore"][o], local_alignment=local)
        strings.prefetch()
        check_ls(its, recs, strings, ix[4][o], order=None if order is None else o)
        assert int(recs["n_ops"].sum()) == ops.size


@pytest.mark.gpu
def test_full_ls_F_records_both_strands(gm):
    items = items_F()
    assert len(items) >= 2990
    run_full_ls(gm, "F", items, False)


@pytest.mark.gpu
def test_full_ls_local_records_both_strands(gm):
    items = items_local()
    assert len(items) >= 2260
    run_full_ls(gm, "local", items, True)


@pytest.mark.gpu
def test_full_ls_scratch_reuse_shuffled_triple_on_strand_1(gm):
    """the F set three times over in a shuffled order in one call (8 970 items, more than the largest grid) through the strand-1 addressing"""
    order = lambda n: np.random.default_rng(20261018).permutation(np.tile(np.arange(n), 3))
    assert order(len(items_F())).size > 2048 * 4
    run_full_ls(gm, "F", items_F(), False, order=order, strands=(1,))


# ---- 3: sw_full_cs ---------------------------------------------------------------------------------------------------------------------------------------
def run_full_cs(gm, key, items, local, st, rna=-1):
    its = items if st == 0 else [it for it in items if no_u(it["g"])]
    ix = indexes(gm, (key, st > 0), [it["g"] for it in its])
    a = arrays(its)
    recs, ops, strings = ix[st].sw_full_cs_batch(ix[3], np.full(len(its), st, dtype=np.uint8), ix[4] + a["goff"], a["glen"], a["reads"], a["rlen"], a["initbp"], a["anchors"],
                                                 a["rv"], a["thresh"], xover=a["xs"], is_rna=rna, local_alignment=local)
    return its, ix, a, recs, ops, strings


@pytest.mark.gpu
@pytest.mark.parametrize("name,kinds,local,rna,at_least", [
    ("sw_kat_cs.txt.gz", "S", False, 0, 1400), ("sw_kat_cs_local.txt.gz", "L", True, 0, 800), ("sw_kat_cs_xover.txt.gz", "X", False, 0, 1000),
    ("sw_kat_cs_xover.txt.gz", "Y", True, 0, 500), ("sw_kat_cs_rna.txt.gz", "S", False, 1, 600), ("sw_kat_cs_rna.txt.gz", "L", True, 1, 600)])
def test_full_cs_fixture_sets(gm, name, kinds, local, rna, at_least):
    items = items_cs(name, kinds)
    assert len(items) >= at_least and any(it["want"][0] > 0 for it in items)
    gm.sw_full_cs_setup(*CS_SETUP)
    for st in ((0,) if rna else (0, 1)):                                     # the RNA fixture: strand 0 with is_rna = 1
        its, ix, a, recs, ops, strings = run_full_cs(gm, (name, kinds), items, local, st, rna=rna)
        assert len(its) >= 0.9 * len(items)
        strings.prefetch()
        check_cs(its, recs, strings, ix[4])


# ---- 4: sw_vector, letter space -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_vector_V_records_both_strands_and_bounded(gm):
    recs = [r for r in oa.load_kat() if r[0] == "V"]
    assert len(recs) >= 1500
    gm.sw_vector_setup(1400, 1000, -33, -7, -33, -3, 10, -15, 0, True)
    for st in (0, 1):
        its = recs if st == 0 else [r for r in recs if no_u(r[4])]
        assert len(its) >= 0.9 * len(recs)
        ix = indexes(gm, ("V", st > 0), [r[4] for r in its])
        goff, glen, rlen, want = (np.array([r[k] for r in its], dtype=np.int64) for k in (1, 2, 3, 6))
        reads = reads_matrix([r[5] for r in its], rlen); sts = np.full(len(its), st, dtype=np.uint8)
        got = ix[st].sw_vector_batch(ix[3], sts, ix[4] + goff, glen, reads, rlen)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
        # bounded, one call per threshold value of the fixture (the threshold is a call's, the fixture's scores are the items'): threshold = score -> not stopped and
        # equal; threshold = score + 1 -> stopped with a lower bound, or equal
        for s in np.unique(want):
            if s <= 0: continue
            m = np.nonzero(want == s)[0]
            for thr in (int(s), int(s) + 1):
                g2, stopped = ix[st].sw_vector_batch_bounded(ix[3][m], sts[m], (ix[4] + goff)[m], glen[m], reads[m], rlen[m], thr)
                sb = stopped.astype(bool)
                if thr == s: assert not sb.any() and (g2 == s).all(), (st, s)
                else: assert (g2[~sb] == s).all() and (g2[sb] <= s).all() and (g2[sb] >= 0).all(), (st, s)


# ---- 5: sw_vector and sw_gapless, colour space ---------------------------------------------------------------------------------------------------------------
def gapless_records(name="sw_kat_gapless.txt.gz"):
    out = []
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", name), "rt") as f:
        for line in f:
            t = line.split()
            if t[0] != "G": continue
            glen, rlen, g_idx, r_idx, init_bp = (int(x) for x in t[1:6])
            out.append(dict(glen=glen, rlen=rlen, g_idx=g_idx, r_idx=r_idx, initbp=init_bp, g=oa.parse_words(t[6]), r=oa.parse_words(t[7]),
                            gl=None if t[8] == "-" else oa.parse_words(t[8]), score=int(t[9])))
    return out


def c_records():
    """the colour-space vector records whose window starts behind their bitfield's first colour (that colour is the record's own, not a contig's)"""
    allc = [r for r in oa.load_kat_cs() if r[0] == "C"]
    keep = [r for r in allc if r[1] >= 1]
    return allc, keep


def test_enough_C_records_start_behind_their_first_colour():
    allc, keep = c_records()
    assert len(allc) >= 700 and 2 * len(keep) >= len(allc), (len(allc), len(keep))
    for _, goff, glen, rlen, initbp, gcs, gls, rd, score in keep[:50]:                   # and behind it the fixture's colours are the translation of its letters
        assert np.array_equal(unpack(gcs)[goff:goff + glen], colours(unpack(gls), False)[goff:goff + glen])


@pytest.mark.gpu
def test_vector_cs_C_records_both_strands(gm):
    _, keep = c_records()
    gm.sw_vector_setup(1400, 1000, -33, -7, -33, -3, 10, 10 - 20, 1, True)              # mismatch = match + crossover
    for st in (0, 1):
        its = keep if st == 0 else [r for r in keep if no_u(r[6])]
        ix = indexes(gm, ("C", st > 0), [r[6] for r in its], colour=True)
        goff, glen, rlen, initbp, want = (np.array([r[k] for r in its], dtype=np.int64) for k in (1, 2, 3, 4, 8))
        got = ix[st].sw_vector_batch(ix[3], np.full(len(its), st, dtype=np.uint8), ix[4] + goff, glen, reads_matrix([r[7] for r in its], rlen), rlen, initbp=initbp)
        assert np.array_equal(got, want), (st, np.nonzero(got != want)[0][:10])


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [False, True])
def test_gapless_known_answers_both_strands(gm, colour):
    """a contig per record: sw_gapless scores against the whole contig of the strand.  Colour space: the records whose colour bitfield is the translation of their
    letters from the first colour on (the index derives its colours from the letters, first colour against T)."""
    recs = [r for r in gapless_records() if (r["gl"] is not None) == colour]
    assert len(recs) >= 1200
    if colour:
        n_all = len(recs)
        recs = [r for r in recs if np.array_equal(unpack(r["g"], r["glen"]), colours(unpack(r["gl"], r["glen"]), False))]
        print("colour-space gapless records whose first colour is T's: %d of %d" % (len(recs), n_all))
        assert 2 * len(recs) >= n_all, (len(recs), n_all)              # (as for the C records: at least half must remain; seen: all 1 200)
    gm.sw_gapless_setup(10, -24 if colour else -15)
    for st in (0, 1):
        letters = "gl" if colour else "g"
        its = recs if st == 0 else [r for r in recs if no_u(r[letters])]
        assert len(its) >= 0.9 * len(recs)
        ix = indexes(gm, ("G", colour, st > 0), [(r[letters], r["glen"]) for r in its], colour=colour, per_item=True)
        rlen, g_idx, r_idx, initbp, want = (np.array([r[k] for r in its], dtype=np.int64) for k in ("rlen", "g_idx", "r_idx", "initbp", "score"))
        got = ix[st].sw_gapless_batch(ix[3], np.full(len(its), st, dtype=np.uint8), reads_matrix([r["r"] for r in its], rlen), rlen, g_idx, r_idx,
                                      initbp=initbp if colour else None, colour_space=colour)
        assert np.array_equal(got, want), (st, np.nonzero(got != want)[0][:10], got[:10], want[:10])


def host_strand1(contigs):
    """the strand-1 contigs as host bitfields laid end to end, each on a word boundary: letters, colours, first word of each"""
    lw, cw, woff, at = [], [], [], 0
    for c in contigs:
        let, col = strand_contig(c, 1)
        lw.append(pack(let)); cw.append(pack(col)); woff.append(at); at += len(lw[-1])
    return np.concatenate(lw), np.concatenate(cw), np.array(woff, dtype=np.int64)


@pytest.mark.gpu
def test_random_colour_windows_on_strand_1_against_the_host_bitfield_entries(gm):
    """300 windows on strand 1 (offset 0 of the reverse-complement contig among them: its first colour is T against the complement of the contig's last letter),
    vector and gapless, against gm_sw_vector_batch_cs / gm_sw_gapless_batch on the numpy translation of the reverse-complement contigs; is_rna 0 and 1"""
    contigs = genome7(); lens = np.array([len(c) for c in contigs])
    rng = np.random.default_rng(5)
    n, L = 300, 50
    cn = rng.choice([0, 3, 6], size=n).astype(np.int32); st = np.ones(n, dtype=np.uint8)
    glen = rng.integers(60, 120, size=n).astype(np.int32)
    off = np.array([rng.integers(0, lens[c] - g + 1) for c, g in zip(cn, glen)], dtype=np.int64); off[::4] = 0
    let_w, col_w, woff = host_strand1(contigs)
    # reads: the window's own colours with substitutions, so that the scores are not all small
    wins = expected_windows(contigs, cn, st, off, glen, True)
    reads = np.stack([np.where(rng.random(L) < 0.1, rng.integers(0, 4, size=L), np.where(w[:L] > 3, 0, w[:L])) for w in wins]).astype(np.uint8)
    rw = np.stack([pack(r) for r in reads]); rlen = np.full(n, L, dtype=np.int32); initbp = rng.integers(0, 4, size=n).astype(np.int32)
    ix = gm.Index(contigs, params=gm.default_params_cs())
    gm.sw_vector_setup(1400, 1000, -33, -7, -33, -3, 10, 10 - 20, 1, True)
    for rna in (0, 1):
        want = gm.sw_vector_batch_cs(col_w, let_w, woff[cn] * 8 + off, glen, rw, rlen, initbp | (0x100 if rna else 0))
        got = ix.sw_vector_batch(cn, st, off, glen, rw, rlen, initbp=initbp, is_rna=rna)
        assert np.array_equal(got, want), (rna, np.nonzero(got != want)[0][:10])
        assert (want > 100).sum() > n // 2
    assert np.array_equal(ix.sw_vector_batch(cn, st, off, glen, rw, rlen, initbp=initbp), ix.sw_vector_batch(cn, st, off, glen, rw, rlen, initbp=initbp, is_rna=0))   # -1: the last contig is DNA
    gm.sw_gapless_setup(10, -24)
    g_idx = (off + rng.integers(0, 30, size=n)).astype(np.int32); r_idx = rng.integers(0, 20, size=n).astype(np.int32)
    g_idx[::4] = r_idx[::4] // 2                                                         # diagonals that start at the strand contig's position 0
    for rna in (0, 1):
        want = gm.sw_gapless_batch(col_w, woff[cn], lens[cn], rw, rlen, g_idx, r_idx, genome_ls=let_w, initbp=initbp | (0x100 if rna else 0))
        got = ix.sw_gapless_batch(cn, st, rw, rlen, g_idx, r_idx, initbp=initbp, colour_space=True, is_rna=rna)
        assert np.array_equal(got, want), (rna, np.nonzero(got != want)[0][:10])
    ix.close()


# ---- 6: post_sw ------------------------------------------------------------------------------------------------------------------------------------------
def host_contigs(contigs):
    w = [pack(c) for c in contigs]
    return np.concatenate(w), np.concatenate([[0], np.cumsum([len(x) for x in w])[:-1]]).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("use_qvs", [False, True])
def test_post_sw_known_answers_both_strands(gm, use_qvs):
    """the 1 222 + 611 known answers through Index.sw_full_cs_batch, then Index.post_sw_batch: counts, qralign and qual equal the fixture's, the posterior within the
    header's 1e-9 relative; and every field -- by_host and the posterior's bits included -- equals gm_post_sw_batch on the host bitfield of the strand's contigs.
    Seen on an MI355X, on either strand: largest relative difference from the fixture 5.4e-16 without QVs (32 of 1 222 by the host routine), 4.2e-16 with QVs (0 of 611)."""
    K, P = tp.fixture()
    want = [w for w in P if w["useq"] == int(use_qvs)]
    assert len(want) == (611 if use_qvs else 1222)
    allS = tp.s_items()
    tp.setup(gm, use_qvs=use_qvs)
    for st in (0, 1):
        sel = [w for w in want if st == 0 or no_u(allS[w["idx"]]["g"])]
        assert len(sel) >= 0.9 * len(want)
        items = [allS[w["idx"]] for w in sel]; quals = [w["qin"].encode() for w in sel] if use_qvs else None
        its, ix, a, recs, ops, strings = run_full_cs(gm, ("post", use_qvs), items, False, st)
        sts = np.full(len(items), st, dtype=np.uint8)
        post, qralign, qual = ix[st].post_sw_batch(ix[3], sts, recs, ops, a["reads"], a["rlen"], a["initbp"], quals=quals)
        res = dict(post=post, qralign=qralign, qual=qual)
        tp.check_known(res, list(enumerate(sel)), "ix strand %d, QVs %d" % (st, use_qvs))
        # the host-bitfield entry on the same records: ix[2] holds the contigs of strand 0 of the first index == strand 1 of the second
        gw, wbase = host_contigs(ix[2])
        r2 = recs.copy(); r2["genome_start"] += wbase[ix[3]] * 8
        post2, qralign2, qual2 = gm.post_sw_batch(r2, ops, gw, a["reads"], a["rlen"], a["initbp"], quals=quals)
        assert post.tobytes() == post2.tobytes(), np.nonzero([post[k].tobytes() != post2[k].tobytes() for k in range(len(post))])[0][:10]
        for k in range(len(items)): assert qralign(k) == qralign2(k) and qual(k) == qual2(k), k


# ---- 7 / 8: the pipeline's own windows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pipeline_windows_letter_space(gm):
    """cfg2s_100bp_2Mbp, the first 256 reads: every window pass 1 selected (Session.tophits, f1 cache emulation off), scored again by Index.sw_vector_batch as
    (cn, 0, g_off, w_len) with the read as given for st = 0 and its reverse complement for st = 1, has the row's score_vector"""
    contigs, reads, _ = oa.load_golden("cfg2s_100bp_2Mbp")
    reads = np.ascontiguousarray(reads[:256])
    p = gm.default_params(); p.hash_filter_calls = 0
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    rows = s.tophits(reads)
    assert len(rows) >= 256 and set(rows[:, 1].tolist()) == {0, 1}
    rc = CMPL[reads[:, ::-1]]
    rd = np.where(rows[:, 1:2] == 0, reads[rows[:, 0]], rc[rows[:, 0]])
    gm.sw_vector_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, 0, True)
    got = ix.sw_vector_batch(rows[:, 2], np.zeros(len(rows), dtype=np.uint8), rows[:, 3], rows[:, 4], np.stack([pack(r) for r in rd]), np.full(len(rows), reads.shape[1]))
    assert np.array_equal(got, rows[:, 5]), np.nonzero(got != rows[:, 5])[0][:10]
    s.close(); ix.close()


@pytest.mark.gpu
def test_pipeline_windows_colour_space(gm):
    """cfg4s_50col_2Mbp, the first 256 reads.  Row -> window, as k_pass1 loads it: a row is (read, st, cn, g_off, w_len, score_vector, ...) with g_off on the forward
    strand.  The read is always the input strand (strand 0: its colours as sequenced) and initbp is its primer.  A row with st = 0 is the window (cn, 0, g_off,
    w_len); a row with st = 1 is the same stretch turned onto the read's strand: (cn, 1, clen - g_off - w_len, w_len).
    Session.tophits gets the primers with the colours (gm_debug_tophits_cs)."""
    contigs, reads, _ = oa.load_golden("cfg4s_50col_2Mbp")
    reads = np.ascontiguousarray(reads[:256])
    p = gm.default_params_cs(); p.hash_filter_calls = 0
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    cols = np.ascontiguousarray(reads[:, 1:])
    rows = s.tophits(cols, initbp=reads[:, 0])
    assert len(rows) >= 256 and set(rows[:, 1].tolist()) == {0, 1}
    clen = ix.contig_lengths()[rows[:, 2]]
    st = rows[:, 1].astype(np.uint8)
    off = np.where(st == 0, rows[:, 3], gm.Index.strand_offset(clen, rows[:, 3], rows[:, 4]))
    gm.sw_vector_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.match_score + p.crossover_score, 1, True)
    got = ix.sw_vector_batch(rows[:, 2], st, off, rows[:, 4], np.stack([pack(r) for r in cols])[rows[:, 0]], np.full(len(rows), cols.shape[1]), initbp=reads[rows[:, 0], 0])
    assert np.array_equal(got, rows[:, 5]), np.nonzero(got != rows[:, 5])[0][:10]
    s.close(); ix.close()


# ---- 9: refusals beside answers ------------------------------------------------------------------------------------------------------------------------------
def with_bad(good, lens):
    """72 rows (cn, st, off, glen, source item): the 64 good windows with eight bad ones spread through them -> (rows, positions of the bad ones)"""
    c0 = int(good[0][0]); L = int(lens[c0]); nc = len(lens)
    bad = [(-1, 0, 0, 20), (nc, 0, 0, 20), (c0, 2, 0, 20), (c0, 0, -1, 20), (c0, 0, 0, 0), (c0, 0, L - 19, 20), (c0, 1, L - 19, 20), (nc + 5, 1, 3, 20)]
    rows, where = [], []
    for k, g in enumerate(good):
        if k % 8 == 3: where.append(len(rows)); rows.append(bad[k // 8] + (k,))
        rows.append(tuple(int(x) for x in g) + (k,))
    assert len(where) == 8 and len(rows) == 72
    cn, st, off, glen, src = (np.array([r[k] for r in rows], dtype=np.int64) for k in range(5))
    ok = np.ones(len(rows), dtype=bool); ok[where] = False
    return cn, st.astype(np.uint8), off, glen, src, ok, where


@pytest.mark.gpu
def test_refusals_beside_answers(gm):
    items = items_F()[:64]
    ix = indexes(gm, ("F", False), [it["g"] for it in items_F()])
    lens = ix[0].contig_lengths(); a = arrays(items)
    cn, st, off, glen, src, ok, where = with_bad(list(zip(ix[3][:64], np.zeros(64, dtype=np.int64), ix[4][:64] + a["goff"], a["glen"])), lens)
    rd, rl = a["reads"][src], a["rlen"][src]
    # full: per-item refusal, the 64 good answers equal a call without the bad ones
    gm.sw_full_ls_setup(*LS_SETUP)
    full = lambda m: ix[0].sw_full_ls_batch(cn[m], st[m], off[m], glen[m], rd[m], rl[m], a["anchors"][src[m]], a["rv"][src[m]], a["thresh"][src[m]], a["maxscore"][src[m]])
    recs, ops, strings = full(slice(None))
    assert (recs["status"][where] == GM_E_ARG).all() and (recs["score"][where] == 0).all() and (recs["status"][ok] == 0).all()
    assert b"refused" in gm.lib().gm_last_error()
    recs0, ops0, strings0 = full(ok)
    assert np.array_equal(recs[ok], recs0) and np.array_equal(ops, ops0)
    check_ls(items, recs0, strings0, ix[4][:64])
    # get_windows / vector / gapless have no per-item status: the call fails and names the item (here: the good items before a bad one, and that one)
    gm.sw_vector_setup(1400, 1000, -33, -7, -33, -3, 10, -15, 0, True); gm.sw_gapless_setup(10, -15)
    for kind, b in enumerate(where):
        m = ok.copy(); m[b:] = False; m[b] = True
        pos = int(m.sum()) - 1; z = np.zeros(pos + 1, dtype=np.int64)
        calls = [lambda: ix[0].get_windows(cn[m], st[m], off[m], glen[m]), lambda: ix[0].sw_vector_batch(cn[m], st[m], off[m], glen[m], rd[m], rl[m]),
                 lambda: ix[0].sw_vector_batch_bounded(cn[m], st[m], off[m], glen[m], rd[m], rl[m], 100)]
        if kind in (0, 1, 2, 7): calls.append(lambda: ix[0].sw_gapless_batch(cn[m], st[m], rd[m], rl[m], z, z))      # (it takes no g_off / glen: the contig and the strand)
        for call in calls:
            with pytest.raises(gm.GmError) as e: call()
            assert "(%d)" % GM_E_ARG in str(e.value) and "item %d:" % pos in str(e.value), (kind, str(e.value))
    # a negative glen is a glen < 1 like any other (never "the whole contig"), alone and behind good items, whatever the stride a caller computed
    for at in (0, 5):
        m = np.zeros(len(cn), dtype=bool); m[np.nonzero(ok)[0][:at + 1]] = True
        g2 = glen[m].copy(); g2[at] = -1
        for call in (lambda: ix[0].get_windows(cn[m], st[m], off[m], g2), lambda: ix[0].sw_vector_batch(cn[m], st[m], off[m], g2, rd[m], rl[m]),
                     lambda: ix[0].sw_vector_batch_bounded(cn[m], st[m], off[m], g2, rd[m], rl[m], 100)):
            with pytest.raises(gm.GmError) as e: call()
            assert "(%d)" % GM_E_ARG in str(e.value) and "item %d: glen < 1" % at in str(e.value), str(e.value)
    r1, _, _ = ix[0].sw_full_ls_batch(cn[ok][:1], st[ok][:1], off[ok][:1], np.array([-1]), rd[ok][:1], rl[ok][:1])
    assert r1["status"][0] == GM_E_ARG
    # a window longer than the setup's: the call fails and names the entry and the item
    gm.sw_vector_setup(30, 1000, -33, -7, -33, -3, 10, -15, 0, True)
    with pytest.raises(gm.GmError) as e: ix[0].sw_vector_batch(cn[ok], st[ok], off[ok], glen[ok], rd[ok], rl[ok])
    assert "gm_sw_vector_batch_ix: item " in str(e.value) and "longer than" in str(e.value), str(e.value)
    # a colour-space call on a letter index
    gm.sw_vector_setup(1400, 1000, -33, -7, -33, -3, 10, -10, 1, True)
    z = np.zeros(64, dtype=np.int64)
    for call in (lambda: ix[0].get_windows(cn[ok], st[ok], off[ok], glen[ok], colours=True),
                 lambda: ix[0].sw_vector_batch(cn[ok], st[ok], off[ok], glen[ok], rd[ok], rl[ok], initbp=z),
                 lambda: ix[0].sw_gapless_batch(cn[ok], st[ok], rd[ok], rl[ok], z, z, initbp=z, colour_space=True)):
        with pytest.raises(gm.GmError) as e: call()
        assert "(%d)" % GM_E_ARG in str(e.value) and "colour" in str(e.value), str(e.value)
    # n = 0: GM_OK, nothing written
    e0 = np.zeros(0, dtype=np.int64)
    assert ix[0].get_windows(e0, e0, e0, e0).shape[0] == 0 and ix[0].sw_vector_batch(e0, e0, e0, e0, np.zeros((0, 4)), e0).size == 0
    assert len(ix[0].sw_full_ls_batch(e0, e0, e0, e0, np.zeros((0, 4)), e0)[0]) == 0


@pytest.mark.gpu
def test_refusals_beside_answers_cs_and_post(gm):
    """colour space: sw_full_cs_batch_ix refuses the eight items one by one, post_sw_batch_ix passes those refusals on and refuses a record whose contig or strand does
    not exist; the 64 good answers equal a call without the bad ones"""
    allS = tp.s_items()
    items = [allS[w["idx"]] for w in tp.fixture()[1] if w["useq"] == 0][:64]
    ix = indexes(gm, ("S64",), [it["g"] for it in items])
    lens = ix[0].contig_lengths(); a = arrays(items)
    cn, st, off, glen, src, ok, where = with_bad(list(zip(ix[3], np.zeros(64, dtype=np.int64), ix[4] + a["goff"], a["glen"])), lens)
    rd, rl, ib = a["reads"][src], a["rlen"][src], a["initbp"][src]
    tp.setup(gm)
    full = lambda m: ix[0].sw_full_cs_batch(cn[m], st[m], off[m], glen[m], rd[m], rl[m], ib[m], a["anchors"][src[m]], a["rv"][src[m]], a["thresh"][src[m]])
    recs, ops, strings = full(slice(None)); recs0, ops0, strings0 = full(ok)
    assert (recs["status"][where] == GM_E_ARG).all() and (recs["score"][where] == 0).all() and np.array_equal(recs[ok], recs0) and np.array_equal(ops, ops0)
    check_cs(items, recs0, strings0, ix[4])
    postf = lambda m, r, o, c, s: ix[0].post_sw_batch(c, s, r, o, rd[m], rl[m], ib[m])
    post, qa, qo = postf(slice(None), recs, ops, cn, st); post0, qa0, qo0 = postf(ok, recs0, ops0, cn[ok], st[ok])
    assert (post["status"][where] == GM_E_ARG).all() and (post["status"][ok] == 0).all() and (post0["posterior"] > 0).all()
    for k0, k in enumerate(np.nonzero(ok)[0]):
        assert post[k]["posterior"] == post0[k0]["posterior"] and qa(k) == qa0(k0) and qo(k) == qo0(k0) and post[k]["matches"] == post0[k0]["matches"], k
    c2 = cn[ok].copy(); s2 = st[ok].copy(); c2[5] = len(lens); s2[9] = 2                 # good records, a contig / a strand that does not exist
    post3, _, _ = postf(ok, recs0, ops0, c2, s2)
    assert post3["status"][5] == GM_E_ARG and post3["status"][9] == GM_E_ARG and (np.delete(post3["status"], [5, 9]) == 0).all()
    assert post3[0]["posterior"] == post0[0]["posterior"]


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
    assert m and int(m.group(1)) >= 21, r.stdout[-500:]


# ---- without a device ------------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_listed():
    from shrimp_amd import gmapper
    L = gmapper.lib()
    for s in IX_SYMBOLS: assert hasattr(L, s) and s in gmapper.EXPORTS, s
    for m in ("get_windows", "sw_vector_batch", "sw_vector_batch_bounded", "sw_gapless_batch", "sw_full_ls_batch", "sw_full_cs_batch", "post_sw_batch", "contig_lengths"):
        assert callable(getattr(gmapper.Index, m)), m


def _null_calls(L):
    """every new entry with ix = NULL and n = 1 (nothing else is looked at)"""
    N = None
    return {"gm_index_genome_is_rna": lambda: L.gm_index_genome_is_rna(N),
            "gm_index_get_windows": lambda: L.gm_index_get_windows(N, 1, N, N, N, N, 0, N, 1),
            "gm_sw_vector_batch_ix": lambda: L.gm_sw_vector_batch_ix(N, 1, N, N, N, N, N, 1, N, N, -1, N),
            "gm_sw_vector_batch_bounded_ix": lambda: L.gm_sw_vector_batch_bounded_ix(N, 1, N, N, N, N, N, 1, N, 100, N, N),
            "gm_sw_gapless_batch_ix": lambda: L.gm_sw_gapless_batch_ix(N, 1, N, N, 0, N, 1, N, N, N, N, -1, N),
            "gm_sw_full_ls_batch_ix": lambda: L.gm_sw_full_ls_batch_ix(N, 1, N, N, N, N, N, 1, N, N, N, N, N, 0, N, N, N),
            "gm_sw_full_cs_batch_ix": lambda: L.gm_sw_full_cs_batch_ix(N, 1, N, N, N, N, N, 1, N, N, N, N, N, N, 0, -1, 0, N, N, N),
            "gm_post_sw_batch_ix": lambda: L.gm_post_sw_batch_ix(N, 1, N, N, N, N, 0, N, 1, N, N, N, -1, N, N, N, N)}


def test_null_index_is_refused_without_a_device():
    from shrimp_amd import gmapper
    L = gmapper.lib()
    calls = _null_calls(L)
    assert sorted(calls) == sorted(IX_SYMBOLS)
    out = {}
    def fresh():                                            # a new thread has no setup state: the NULL index is refused before that is looked at
        for s, f in calls.items(): out[s] = (f(), L.gm_last_error())
    t = threading.Thread(target=fresh); t.start(); t.join()
    for s in IX_SYMBOLS: assert out[s][0] == GM_E_ARG and b"ix is NULL" in out[s][1], (s, out[s])


def test_abi_sizes_are_what_they_were():
    from shrimp_amd import gmapper
    assert [gmapper.lib().gm_abi_sizeof(k) for k in range(6)] == [280, 40, 200, 72, 64, 40]      # (the parent commit's: no public struct changes)


def test_strand_offset_round_trips():
    from shrimp_amd import gmapper
    rng = np.random.default_rng(3)
    clen = rng.integers(1, 5000, size=1000); glen = np.array([rng.integers(1, c + 1) for c in clen]); off = np.array([rng.integers(0, c - g + 1) for c, g in zip(clen, glen)])
    m = gmapper.Index.strand_offset(clen, off, glen)
    assert np.array_equal(m, mirror(clen, off, glen)) and (m >= 0).all() and (m + glen <= clen).all()
    assert np.array_equal(gmapper.Index.strand_offset(clen, m, glen), off)
    # and it is the reversal: positions off .. off + glen of a strand are positions m .. m + glen of the other, read backwards
    c = rng.integers(0, 4, size=int(clen[0]), dtype=np.uint8)
    assert np.array_equal(revcomp(c, False)[m[0]:m[0] + glen[0]], CMPL[c[off[0]:off[0] + glen[0]][::-1]])


def test_numpy_strands_reproduce_a_reference_genome_file():
    """tests/golden/genfa/cs/idx.genome (written by the reference's gmapper-cs -S) holds, behind the forward bitfields, the reverse-complement contigs and the colour
    translation of the forward ones: revcomp() and colours() above reproduce both, an RNA contig among them"""
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", "genfa", "cs", "idx.genome"), "rb") as f: b = f.read()
    mode, hflag, nc = struct.unpack_from("<3I", b, 0)
    assert mode == 2
    lens = list(struct.unpack_from("<%dI" % nc, b, 12)); p = 12 + 8 * nc
    for _ in range(nc): (nl,) = struct.unpack_from("<I", b, p); p += 4 + nl + 1
    p += 4
    blocks = []
    for _ in range(3):
        blk = []
        for n in lens: w = (n + 7) // 8; blk.append(unpack(np.frombuffer(b, dtype="<u4", count=w, offset=p), n)); p += 4 * w
        blocks.append(blk)
    assert p == len(b)
    fwd, rc, cs = blocks
    assert any(is_rna(c) for c in fwd) and not all(is_rna(c) for c in fwd)
    for k in range(nc):
        assert np.array_equal(revcomp(fwd[k]), rc[k]), k
        assert np.array_equal(colours(fwd[k], is_rna(fwd[k])), cs[k]), k


def _not_set_up(L):
    out = {}
    def fresh():
        one = (C.c_int * 1)(0); st = (C.c_uint8 * 1)(0); off = (C.c_int64 * 1)(0); gl = (C.c_int * 1)(10)
        fake = C.c_void_p(8)                                # never dereferenced: the setup state is looked at before the index
        out["v"] = L.gm_sw_vector_batch_ix(fake, 1, one, st, off, gl, None, 1, None, None, -1, None)
        out["g"] = L.gm_sw_gapless_batch_ix(fake, 1, one, st, 0, None, 1, None, None, None, None, -1, None)
        out["f"] = L.gm_sw_full_ls_batch_ix(fake, 1, one, st, off, gl, None, 1, None, None, None, None, None, 0, None, None, None)
        out["c"] = L.gm_sw_full_cs_batch_ix(fake, 1, one, st, off, gl, None, 1, None, None, None, None, None, None, 0, -1, 0, None, None, None)
        out["p"] = L.gm_post_sw_batch_ix(fake, 1, one, st, None, None, 0, None, 1, None, None, None, -1, None, None, None, None)
        out["v0"] = L.gm_sw_vector_batch_ix(fake, 0, one, st, off, gl, None, 1, None, None, -1, None)
    t = threading.Thread(target=fresh); t.start(); t.join()
    return out


def test_a_call_before_setup_is_not_set_up():
    from shrimp_amd import gmapper
    out = _not_set_up(gmapper.lib())
    assert all(v == GM_E_NOTSETUP for v in out.values()), out      # (n = 0 too: the state is looked at first, as the host-bitfield entries do)
