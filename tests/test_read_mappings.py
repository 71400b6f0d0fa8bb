"""gm_read_mappings (Session.read_mappings): pass 2 as a seam -- packed reads to hits, second vector scores, full records, final mappings and their CIGAR / edit strings in
one call, on arrays that stay on the device.

Without a GPU: the entry and the size of its result struct; ReadMappings.table() on the records of three reference outputs parsed back into the seam's arrays
(tests/test_sam_records.py's replay): POS, NM and strand are the reference's; the rule of hit_run_full_sw per hit (thresh, the record of a hit under it, revcmpl), restated
here in Python, against ZV and ZH of the same outputs.

On the GPU the call is held to the chain of existing entries fed with its own hits (sw_vector_batch -> sw_full_ls_batch -> zeroing -> select_pass2 -> sw_full_batch_text),
to read_hits on the same session, through sam_records to the reference's bytes and to map_reads, over sub-batches with a capacity growth, on hand-made batches that put
the compaction at its wave steps, at the threshold's boundary, after every refusal, and in the release build."""
import ctypes as C
import os, re, subprocess, sys
import numpy as np
import pytest
from tests import oracle_api as oa
from tests import test_select as ts
from tests import test_sam_records as tsr

GM_E_ARG, GM_E_RANGE = -2, -4
UNGAPPED = dict(local_alignment=1, ungapped=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255, hash_filter_calls=0)


# ---- the rule of hit_run_full_sw (ref: gmapper/mapping.c:332-402), letter space, restated -----------------------------------------------------------------------
def item_rule(sw_full_threshold, tiebreak_rev, score_max, gen_st):
    """-> (thresh, revcmpl) of one hit: thresh = (int)abs_or_pct(sw_full_threshold, score_max), revcmpl = gen_st && Tflag"""
    return int(ts.abs_or_pct(sw_full_threshold, score_max)), bool(gen_st and tiebreak_rev)


def record_rule(sv, thresh, full_record):
    """the record of one hit: sw_full_ls's where sv >= thresh, else what calloc and score = 0 leave (mapping.c:365,396-398)"""
    return full_record if sv >= thresh else None


ZERO_FIELDS = ("score", "read_start", "rmapped", "gmapped", "matches", "mismatches", "insertions", "deletions", "crossovers", "status", "genome_start", "n_ops")


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_and_the_size_of_its_result():
    """fails without the feature"""
    from shrimp_amd import gmapper as G
    L = G.lib()
    header = open(os.path.join(oa.ROOT, "include", "gmapper_hip.h")).read()
    for name in ("gm_read_mappings", "gm_read_mappings_free", "gm_read_mappings_size"):
        assert hasattr(L, name) and name in G.EXPORTS and re.search(r"\b%s\(" % name, header), name
    assert L.gm_read_mappings_size() == C.sizeof(G.ReadMappingsResult) == 136
    assert [L.gm_abi_sizeof(k) for k in range(6)] == [C.sizeof(G.Params), C.sizeof(G.PairOpts), C.sizeof(G.MapStats), C.sizeof(G.MergeOptions), C.sizeof(G.SwFullRec), C.sizeof(G.PostRec)]
    assert L.gm_abi_sizeof(6) == -1                                      # (no field was added to a struct of that list)
    assert hasattr(G.Session, "read_mappings")


REPLAYS = ["cfg2s_100bp_2Mbp@extra_fields", "n1_noisy_70bp@extra_fields_rg_unal", "stress_100bp_unal@local"]


def golden_fields(golden):
    """(read, strand, contig, POS, NM, tags) of every mapped record of a reference output, in its order"""
    import gzip
    out = []
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", golden + ".sam.gz"), "rt") as fh:
        for line in fh:
            if line.startswith("@"): continue
            t = line.rstrip("\n").split("\t")
            if int(t[1]) & 4: continue
            tags = {x[:2]: x[5:] for x in t[11:]}
            out.append((int(t[0][1:]), 1 if int(t[1]) & 16 else 0, int(t[2][len("contig"):]) - 1, int(t[3]), int(tags["NM"]), tags))
    return out


@pytest.mark.parametrize("golden", REPLAYS)
def test_table_on_replayed_records_gives_pos_nm_and_strand_of_the_reference(golden):
    from shrimp_amd import gmapper as G
    I, _, _ = tsr.golden_inputs(golden)
    n = I["codes"].shape[0]
    hit_off = np.zeros(n + 1, dtype=np.uint64)                           # (the replay keeps its hits in another order than its mappings: table() goes by maps[].hit)
    R = G.ReadMappings(I["hits"], hit_off, I["hits"]["score_vector"].copy(), I["recs"], I["maps"], I["map_off"], I["cigar"][0], I["cigar"][1],
                       I["edit"][0] if I["edit"] else None, I["edit"][1] if I["edit"] else None, None, I["contig_len"])
    t = R.table()
    want = golden_fields(golden)
    assert t.dtype == G.MAPPING_TABLE_DTYPE and len(t) == len(want) > 1000
    assert t["read"].tolist() == [w[0] for w in want] and t["strand"].tolist() == [w[1] for w in want] and t["contig"].tolist() == [w[2] for w in want]
    assert t["pos"].tolist() == [w[3] for w in want]
    assert t["nm"].tolist() == [w[4] for w in want]
    assert t["mapq"].tolist() == I["maps"]["mqv"].tolist() and t["as"].tolist() == [int(w[5]["AS"]) for w in want]
    assert np.array_equal(t["hit"], I["maps"]["hit"])
    k = int(I["maps"]["hit"][0]); assert R.cigar(k) == I["cigar"][0][int(I["cigar"][1][k]):int(I["cigar"][1][k + 1])]
    # mapping_positions is a whole-array expression: the same on a shuffled index
    perm = np.random.default_rng(3).permutation(len(t))
    assert np.array_equal(G.mapping_positions(I["hits"], I["recs"], I["contig_len"], I["maps"]["hit"][perm]), t["pos"][perm])


@pytest.mark.parametrize("golden", REPLAYS)
def test_restated_item_rule_holds_on_the_records_of_the_reference(golden):
    """every mapped record of the reference passed the second threshold (ZV >= thresh) and carries sw_full_ls's score (ZH > 0, and in local mode, where no posterior
    rescales it, ZH == AS); a record under the threshold is the zero record and can be no mapping"""
    I, _, _ = tsr.golden_inputs(golden)
    fields = tsr.GOLDENS[golden].get("fields", {})
    thr = fields.get("sw_full_threshold", 50.0); tb = fields.get("tiebreak_rev", 1)
    want = golden_fields(golden)
    assert len(want) == len(I["maps"])
    seen_rev = 0
    for m, w in zip(I["maps"], want):
        h = I["hits"][int(m["hit"])]
        thresh, revcmpl = item_rule(thr, tb, int(h["score_max"]), int(h["gen_st"]))
        assert thresh == int(h["score_max"]) // 2 and revcmpl == bool(w[1])
        seen_rev += revcmpl
        if "ZV" in w[5]:
            assert record_rule(int(w[5]["ZV"]), thresh, "full") == "full", w
            assert int(w[5]["ZH"]) > 0 and int(w[5]["ZH"]) == int(I["recs"][int(m["hit"])]["score"])
        else:
            assert int(w[5]["AS"]) >= thresh                             # (--local: AS is sw_full_ls's score, at most the vector score that let it run)
    assert seen_rev > 100
    # the boundary of the rule itself, in integers and as the double expression
    assert item_rule(50.0, 1, 1000, 1) == (500, True) and item_rule(50.0, 0, 1000, 1) == (500, False) and item_rule(-437.0, 1, 1000, 0) == (437, False)
    assert item_rule(55.0, 1, 700, 0)[0] == 385 and item_rule(57.0, 1, 700, 0)[0] == int(700 * (57.0 / 100.0)) == 398      # 399 in exact arithmetic: the doubles decide
    for sv in (499, 500, 501): assert (record_rule(sv, 500, "full") is None) == (sv < 500)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------------
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


def load_case(name):
    """-> (contigs, reads, the reference's text with its header) of a fixture"""
    if name == "split_60bp":
        from tests import test_many_contigs as tmc
        F = tmc.fixture(name)
        return F["contigs"], np.ascontiguousarray(F["reads"], dtype=np.uint8), None
    contigs, reads, sam = oa.load_golden(name)
    return contigs, np.ascontiguousarray(reads, dtype=np.uint8), sam


def golden_text(name, tag):
    if name == "split_60bp":
        from tests import test_many_contigs as tmc
        return tmc.golden(name, tag)
    return oa.load_option_sam(name, tag) if tag else oa.load_golden(name)[2]


MIRNA_FIELDS, MIRNA_SEEDS = oa.MIRNA_MODE[1], oa.MIRNA_MODE[2]
# case -> (fixture, golden tag or None, gm_params_t fields, seeds, has a golden of its own)
CASES = {
    "cfg2s_100bp_2Mbp": ("cfg2s_100bp_2Mbp", None, {}, None, True),
    "cfg2s_100bp_2Mbp@local_cfg2": ("cfg2s_100bp_2Mbp", "local_cfg2", dict(local_alignment=1), None, True),
    "stress_60bp": ("stress_60bp", None, {}, None, True),
    "n1_noisy_70bp": ("n1_noisy_70bp", None, dict(match_mode=1), None, True),
    "n1_noisy_70bp-mode2": ("n1_noisy_70bp", None, dict(match_mode=2), None, False),      # (its reference output exists with the extra fields only: below)
    "f1_twins_60bp": ("f1_twins_60bp", None, {}, None, True),
    "f1_twins_60bp@no_cache": ("f1_twins_60bp", "no_cache", dict(hash_filter_calls=0), None, True),
    "split_60bp": ("split_60bp", None, {}, None, True),
    "split_60bp@local": ("split_60bp", "local", dict(local_alignment=1), None, True),
    "split_60bp@ungapped": ("split_60bp", "ungapped", UNGAPPED, None, True),
    "mirna_22bp": ("mirna_22bp", None, MIRNA_FIELDS, MIRNA_SEEDS, True),
    "stress_100bp_unal@tiebreak_off": ("stress_100bp_unal", "tiebreak_off", oa.OPTION_CASES["tiebreak_off"][2], None, True),
    "stress_100bp_unal@scores_large": ("stress_100bp_unal", "scores_large", oa.OPTION_CASES["scores_large"][2], None, True),
    # test 2 only
    "cfg2s_100bp_2Mbp@extra_fields": ("cfg2s_100bp_2Mbp", "extra_fields", dict(extra_sam_fields=1), None, True),
    "n1_noisy_70bp@extra_fields_rg_unal": ("n1_noisy_70bp", "extra_fields_rg_unal", dict(extra_sam_fields=1, read_group=b"grp1", sam_unaligned=1, match_mode=2), None, True),
    "stress_60bp@all_contigs": ("stress_60bp", "all_contigs", dict(all_contigs=1), None, True),
    "stress_100bp_unal@rg_unal": ("stress_100bp_unal", "rg_unal", dict(read_group=b"grp1", sam_unaligned=1), None, True),
}
CHAIN_CASES = list(CASES)[:13]
RELEASE_CASES = ["mirna_22bp", "split_60bp@ungapped", "stress_100bp_unal@scores_large"]
_open, _index = {}, {}


def opened(gm, case):
    """(index, session, params, reads) of a case; the cases of a fixture share its index (a small genome's index is a few GB of bucket tables), the miRNA mode has
    its own (its seeds, -H)"""
    if case not in _open:
        name, tag, fields, seeds, _ = CASES[case]
        contigs, reads, _ = load_case(name)
        p = gm.default_params()
        for k, v in fields.items(): setattr(p, k, v)
        key = (name, tuple(seeds or ()), int(p.hash_seeds))
        if key not in _index:
            pi = gm.default_params(); pi.hash_seeds = p.hash_seeds
            _index[key] = gm.Index(contigs, seeds=seeds, params=pi)
        _open[case] = (_index[key], gm.Session(_index[key], params=p, max_batch_reads=8192), p, reads)
    return _open[case]


def close_all():
    """sessions first, then their indexes: the device memory goes back before another module or a child interpreter asks for it"""
    for _, s, _, _ in _open.values(): s.close()
    for k, v in list(_hand.items()):
        if isinstance(k, tuple): v[1].close(); del _hand[k]
    for ix in _index.values(): ix.close()
    _open.clear(); _index.clear(); _answers.clear()


@pytest.fixture(scope="module", autouse=True)
def release_at_the_end():
    yield
    close_all()


def chain_of(gm, ix, s, p, reads, R):
    """the call's own hits through the existing entries (the recipe of tests/test_select.py:654-731, letter space): -> dict(sv, thresh, recs, ops, maps, map_off, cigar, edit)"""
    from shrimp_amd import synth
    hits, hit_off = R.hits, R.hit_off; n = len(hits); rlen = reads.shape[1]
    thresh = np.array([item_rule(p.sw_full_threshold, p.tiebreak_rev, int(sm), 0)[0] for sm in hits["score_max"]], dtype=np.int32)
    if n == 0:
        maps, map_off = s.select_pass2(hits, hit_off, np.zeros(0, dtype=gm.SW_FULL_REC_DTYPE))
        return dict(sv=np.zeros(0, dtype=np.int32), thresh=thresh, recs=np.zeros(0, dtype=gm.SW_FULL_REC_DTYPE), ops=b"", maps=maps, map_off=map_off, cigar=None, edit=None)
    rw = np.ascontiguousarray(synth.pack_reads(reads))[hits["read"]]; lens = np.full(n, rlen)
    anchors = [(int(h["ax"]), int(h["ay"]), int(h["alen"]), int(h["awidth"])) for h in hits]
    cn, gst, goff, wl = hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"]
    revcmpl = (hits["gen_st"] == 1).astype(np.uint8) if p.tiebreak_rev else None
    ts.vector_setup(gm, p); ts.full_setup(gm, p)
    sv = ix.sw_vector_batch(cn, gst, goff, wl, rw, lens)
    recs, ops, _ = ix.sw_full_ls_batch(cn, gst, goff, wl, rw, lens, anchors=anchors, revcmpl=revcmpl, threshscore=thresh, maxscore=sv, local_alignment=bool(p.local_alignment))
    assert (recs["status"] == 0).all()
    zeroed = recs.copy(); zeroed["score"][sv < thresh] = 0
    maps, map_off = s.select_pass2(hits, hit_off, zeroed)
    status, _, _, cigar, edit = ix.sw_full_batch_text(cn, gst, zeroed, ops, rw, lens, reverse=(hits["gen_st"] == 1).astype(np.uint8), what=("cigar", "edit"))
    assert (status == 0).all()
    return dict(sv=sv, thresh=thresh, recs=recs, ops=bytes(ops), maps=maps, map_off=map_off, cigar=cigar, edit=edit)


def assert_equals_chain(gm, p, R, c):
    """every array of the call against the chain's"""
    hits = R.hits; n = len(hits)
    assert R.hits.dtype == gm.PASS1_HIT_DTYPE and R.recs.dtype == gm.SW_FULL_REC_DTYPE and R.maps.dtype == gm.MAPPING_DTYPE
    assert len(R.recs) == len(R.score_vector) == n == int(R.hit_off[-1]) and len(R.cigar_off) == n + 1
    assert np.array_equal(R.score_vector, c["sv"])
    run = c["sv"] >= c["thresh"]
    fields = [f for f in gm.SW_FULL_REC_DTYPE.names if f not in ("ops_off",)]
    for f in fields:
        assert np.array_equal(R.recs[f][run], c["recs"][f][run]), f
    for f in ZERO_FIELDS: assert not R.recs[f][~run].any(), f
    if R.ops is not None:
        assert len(R.ops) == int(R.recs["n_ops"].sum())
        got = R.ops.tobytes(); cops = c["ops"]
        for i in np.nonzero(run & (R.recs["n_ops"] > 0))[0]:
            a, b, k = int(R.recs["ops_off"][i]), int(c["recs"]["ops_off"][i]), int(R.recs["n_ops"][i])
            assert got[a:a + k] == cops[b:b + k], i
    if n: assert np.array_equal(R.recs["ops_off"], np.concatenate([[0], np.cumsum(R.recs["n_ops"].astype(np.uint64))[:-1]]).astype(np.uint64))      # compacted in hit order
    assert np.array_equal(R.map_off, c["map_off"])
    assert R.maps.tobytes() == c["maps"].tobytes()                      # byte for byte, doubles included
    mapped = np.zeros(n, dtype=bool); mapped[R.maps["hit"]] = True
    for i in range(n):
        if mapped[i]:
            assert R.cigar(i) == c["cigar"](i), i
            if p.extra_sam_fields: assert R.edit(i) == c["edit"](i), i
        else:
            assert R.cigar(i) == b"" and (not p.extra_sam_fields or R.edit(i) == b"")
    assert (R.edit_off is not None) == bool(p.extra_sam_fields)
    return int(run.sum())


def tied_reads(s, reads):
    """reads that own a group of equal windows: which of the group a hit names (win, the anchor box) is no promise of gm_read_windows"""
    wins, _ = s.read_windows(reads)
    rows = ts.win_rows(wins)
    return set(rows[ts.tie_mask(rows)][:, 0].tolist())


def left_out(name, s, reads):
    """the reads a comparison with the reference leaves out: those of stress_60bp that own a group of equal windows, at most 33 (tests/test_select.py)"""
    if name != "stress_60bp": return set()
    skip = tied_reads(s, reads)
    assert len(skip) <= 33
    return skip


def by_read(sam, n):
    out = [b""] * n
    for l in sam.splitlines(keepends=True):
        if not l.startswith(b"@"): out[int(l.split(b"\t", 1)[0][1:])] += l
    return out


_answers = {}


def answer(gm, case):
    if case not in _answers:
        ix, s, p, reads = opened(gm, case)
        R = s.read_mappings(reads, want_ops=True)
        _answers[case] = (R, dict(s.stats))
    return _answers[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN_CASES)
def test_equal_to_the_chain_of_existing_entries(gm, case):
    ix, s, p, reads = opened(gm, case)
    R, st = answer(gm, case)
    c = chain_of(gm, ix, s, p, reads, R)
    n_run = assert_equals_chain(gm, p, R, c)
    assert len(R.hits) > 200 and len(R.maps) > 100 and n_run > 100
    assert st["full_calls"] == n_run and st["reads"] == len(reads)
    assert st["full_cells"] == int((R.hits["w_len"].astype(np.int64)[c["sv"] >= c["thresh"]] * reads.shape[1]).sum())
    # the hits against read_hits on the same session, row for row; reads that own groups of equal windows as multisets
    hits2, off2 = s.read_hits(reads)
    assert np.array_equal(off2, R.hit_off)
    skip = tied_reads(s, reads)
    assert len(skip) <= 33
    a, b = ts.hit_rows(R.hits), ts.hit_rows(hits2)
    plain = ~np.isin(a[:, 0], list(skip))
    assert np.array_equal(a[plain], b[plain])
    cols = np.ones(16, dtype=bool); cols[[2, 12, 13, 14, 15]] = False
    for r in skip:
        lo, hi = int(off2[r]), int(off2[r + 1])
        assert sorted(map(tuple, a[lo:hi][:, cols].tolist())) == sorted(map(tuple, b[lo:hi][:, cols].tolist()))
    # without the operations: the same records
    R2 = s.read_mappings(reads)
    assert R2.ops is None and R2.maps.tobytes() == R.maps.tobytes() and R2.cigar_buf == R.cigar_buf
    if not skip: assert R2.recs.tobytes() == R.recs.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_through_sam_records_to_the_bytes_of_the_reference(gm, case):
    name, tag, fields, _, has_golden = CASES[case]
    ix, s, p, reads = opened(gm, case)
    R, _ = answer(gm, case)
    got, off = s.sam_records(reads, R)
    mine = [got[int(off[r]):int(off[r + 1])] for r in range(len(reads))]
    skip = left_out(name, s, reads)
    entry_text = s.map_reads(reads)
    entry = by_read(entry_text, len(reads))
    bad = [r for r in range(len(reads)) if r not in skip and mine[r] != entry[r]]
    assert not bad, (len(bad), [(mine[r], entry[r]) for r in bad[:3]])
    if has_golden:
        sam = golden_text(name, tag)
        want = by_read(sam, len(reads))
        bad = [r for r in range(len(reads)) if r not in skip and mine[r] != want[r]]
        assert not bad, (len(bad), [(mine[r], want[r]) for r in bad[:3]])
        assert sum(1 for r in range(len(reads)) if r not in skip and want[r]) > 200
        assert oa.sam_header(load_case(name)[0]) + entry_text == sam      # afterwards the mapping entry on that session still prints the golden
    # table(): one row per record, POS as printed
    t = R.table()
    pos = [int(l.split(b"\t")[3]) for r in range(len(reads)) for l in mine[r].splitlines() if not int(l.split(b"\t")[1]) & 4]
    assert t["pos"].tolist() == pos


@pytest.mark.gpu
def test_sub_batches_with_a_capacity_growth(gm):
    """300 reads of cfg2s_100bp_2Mbp through sub-batches of 64 (five), and stress_60bp through sub-batches of 1 024 whose first window rows overflow: the result of a
    session that takes the reads in one sub-batch, offsets and hit / win indices included"""
    for case, small, n, grows in (("cfg2s_100bp_2Mbp", 64, 300, False), ("stress_60bp", 1024, None, True)):
        ix, s1, p, reads = opened(gm, case)
        reads = reads[:n] if n else reads
        one = s1.read_mappings(reads, want_ops=True)
        s = gm.Session(ix, params=p, max_batch_reads=small)
        many = s.read_mappings(reads, want_ops=True); st = dict(s.stats)
        s.close()
        assert len(reads) > 4 * small or not n
        assert st["reads"] == len(reads) and (st["retries"] >= 1 or not grows)
        skip = tied_reads(s1, reads)
        if not skip:
            for f in ("hits", "hit_off", "score_vector", "recs", "maps", "map_off", "cigar_off", "ops"):
                assert getattr(one, f).tobytes() == getattr(many, f).tobytes(), f
            assert one.cigar_buf == many.cigar_buf
        else:                                                            # (which of two equal windows a hit names is no promise: everything but win and the box)
            cols = np.ones(16, dtype=bool); cols[[2, 12, 13, 14, 15]] = False
            plain = ~np.isin(one.hits["read"], list(skip))
            assert np.array_equal(one.hit_off, many.hit_off) and np.array_equal(ts.hit_rows(one.hits)[plain], ts.hit_rows(many.hits)[plain])
            assert np.array_equal(one.score_vector[plain], many.score_vector[plain]) and np.array_equal(one.map_off, many.map_off)
            keep = ~np.isin(one.maps["read"], list(skip))
            assert one.maps[keep].tobytes() == many.maps[keep].tobytes()
        assert (many.hits["win"] >= 0).all() and (np.diff(many.hits["read"]) >= 0).all() and int(many.hits["read"].max()) >= len(reads) - small
        assert (np.diff(many.maps["hit"][np.argsort(many.maps["hit"], kind="stable")]) > 0).all() and int(many.maps["hit"].max()) < len(many.hits)
        assert np.array_equal(many.hits["read"][many.maps["hit"]], many.maps["read"])


# ---- hand-made batches on a small index ---------------------------------------------------------------------------------------------------------------------------
HAND_L = 60
_hand = {}


def hand_genome():
    """two random contigs and a tandem repeat: 70 copies of a 100-base unit"""
    if "g" not in _hand:
        rng = np.random.default_rng(20251)
        unit = rng.integers(0, 4, 100).astype(np.uint8)
        c0 = rng.integers(0, 4, 60000).astype(np.uint8); c1 = rng.integers(0, 4, 30000).astype(np.uint8)
        c2 = np.concatenate([rng.integers(0, 4, 500).astype(np.uint8), np.tile(unit, 70), rng.integers(0, 4, 500).astype(np.uint8)])
        _hand["g"] = ([c0, c1, c2], unit)
    return _hand["g"]


def cut_reads(n, L, n_perfect, seed, damaged_ends=3):
    """n reads of L bases from distinct places of contigs 0 and 1, every second one from the reverse strand; n_perfect of them exact, spread over the batch, the others
    with `damaged_ends` substitutions at either end (two bases apart): seeds still match inside, the vector score falls by the clipped ends"""
    (c0, c1, _), _ = hand_genome()
    rng = np.random.default_rng(seed)
    perfect = np.zeros(n, dtype=bool)
    if n_perfect: perfect[np.round(np.linspace(0, n - 1, n_perfect)).astype(int) if n_perfect > 1 else [n // 2]] = True
    assert int(perfect.sum()) == n_perfect
    reads = np.zeros((n, L), dtype=np.uint8)
    for k in range(n):
        c = c0 if k % 3 else c1
        at = 200 + k * ((len(c) - 400 - L) // max(n, 1))
        r = c[at:at + L].copy()
        if k & 1: r = ts.CMPL[r[::-1]]
        if not perfect[k]:
            for j in range(damaged_ends):
                r[2 * j] = (r[2 * j] + 1 + rng.integers(0, 3)) & 3; r[L - 1 - 2 * j] = (r[L - 1 - 2 * j] + 1 + rng.integers(0, 3)) & 3
        reads[k] = r
    return reads, perfect


def hand_session(gm, **fields):
    key = tuple(sorted(fields.items()))
    if ("s", key) not in _hand:
        contigs, _ = hand_genome()
        if ("hand",) not in _index: _index[("hand",)] = gm.Index(contigs, params=gm.default_params())
        p = gm.default_params()
        for k, v in fields.items(): setattr(p, k, v)
        _hand[("s", key)] = (_index[("hand",)], gm.Session(_index[("hand",)], params=p, max_batch_reads=512), p)
    return _hand[("s", key)]


def run_hand(gm, ix, s, p, reads):
    R = s.read_mappings(reads, want_ops=True)
    c = chain_of(gm, ix, s, p, reads, R)
    n_run = assert_equals_chain(gm, p, R, c)
    return R, c, n_run


@pytest.mark.gpu
@pytest.mark.parametrize("n_pass", [0, 1, 63, 64, 65, 129])
def test_compaction_at_the_wave_steps(gm, n_pass):
    """exactly n_pass hits pass a second threshold of 90 %, the others pass pass 1 (50 %) only: every passing hit is aligned, every other carries the zero record"""
    ix, s, p = hand_session(gm, sw_full_threshold=90.0)
    reads, perfect = cut_reads(200, HAND_L, n_pass, seed=7 + n_pass)
    R, c, n_run = run_hand(gm, ix, s, p, reads)
    assert np.diff(R.hit_off.astype(np.int64)).tolist() == [1] * len(reads)      # one hit a read: the damaged ones passed pass 1
    assert n_run == n_pass == int(s.stats["full_calls"])
    run = c["sv"] >= c["thresh"]
    assert np.array_equal(run, perfect[R.hits["read"]])
    assert (R.recs["score"][run] == 10 * HAND_L).all() and (c["sv"][~run] >= 300).all() and (c["thresh"] == 540).all()
    assert np.array_equal(np.diff(R.map_off.astype(np.int64)), perfect.astype(np.int64))
    assert [R.cigar(int(i)) for i in R.maps["hit"]] == [b"%dM" % HAND_L] * n_pass
    # nothing depends on the order or on a second run
    again = s.read_mappings(reads, want_ops=True)
    for f in ("hits", "score_vector", "recs", "maps", "cigar_off", "ops"): assert getattr(again, f).tobytes() == getattr(R, f).tobytes(), f


@pytest.mark.gpu
def test_hand_made_edges(gm):
    """a read with 64 hits from a tandem repeat under num_tmp_outputs = 64; a batch without a window; no reads; reads of 22 bases and of longest_read_len"""
    contigs, unit = hand_genome()
    ix, s, p = hand_session(gm, sw_full_threshold=90.0, num_tmp_outputs=64, num_outputs=64)
    damaged, _ = cut_reads(40, HAND_L, 0, seed=3)
    tandem = np.concatenate([unit[10:], unit[:10]])[:HAND_L][None, :]
    reads = np.concatenate([damaged[:20], tandem, damaged[20:]])
    R, c, n_run = run_hand(gm, ix, s, p, reads)
    per = np.diff(R.hit_off.astype(np.int64))
    assert int(per[20]) == 64 and n_run == 64 and int(np.diff(R.map_off.astype(np.int64))[20]) == 64 and len(R.maps) == 64
    assert (R.hits["cn"][R.maps["hit"]] == 2).all()
    # no read has a window: hits, maps and text are all empty
    rng = np.random.default_rng(99)
    E = s.read_mappings(rng.integers(0, 4, (50, HAND_L)).astype(np.uint8), want_ops=True)
    assert len(E.hits) == len(E.recs) == len(E.maps) == len(E.score_vector) == len(E.ops) == 0 and E.cigar_buf == b""
    assert E.hit_off.tolist() == [0] * 51 == E.map_off.tolist() and E.cigar_off.tolist() == [0] and len(E.table()) == 0
    got, off = s.sam_records(rng.integers(0, 4, (50, HAND_L)).astype(np.uint8), E)
    assert got == b"" and off.tolist() == [0] * 51
    # no reads
    Z = s.read_mappings(np.zeros((0, HAND_L), dtype=np.uint8))
    assert len(Z.hits) == len(Z.maps) == 0 and Z.hit_off.tolist() == [0] == Z.map_off.tolist() == Z.cigar_off.tolist() and Z.ops is None
    # the shortest and the longest reads: 22 bases under match mode 1, and longest_read_len
    ix1, s1, p1 = hand_session(gm, match_mode=1)
    short, _ = cut_reads(150, 22, 150, seed=5)
    R, c, n_run = run_hand(gm, ix1, s1, p1, short)
    assert len(R.hits) > 0 and n_run > 0 and (R.recs["score"][c["sv"] >= c["thresh"]] <= 220).all()
    ixl, sl, pl = hand_session(gm, longest_read_len=150)
    long_, perfect = cut_reads(70, 150, 35, seed=6, damaged_ends=8)
    R, c, n_run = run_hand(gm, ixl, sl, pl, long_)
    assert n_run >= 35 and int((R.recs["score"] == 1500).sum()) == 35 and set(R.hits["read"][R.recs["score"] == 1500].tolist()) == set(np.nonzero(perfect)[0].tolist())
    with pytest.raises(gm.GmError) as e: sl.read_mappings(np.zeros((2, 151), dtype=np.uint8))
    assert "(%d)" % GM_E_RANGE in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("absolute", [False, True])
def test_threshold_boundary(gm, absolute):
    """hits whose second vector score is thresh - 1, thresh and thresh + 1, under a percentage and under an absolute threshold"""
    reads, _ = cut_reads(64, HAND_L, 0, seed=11)
    ix0, s0, p0 = hand_session(gm)
    base = s0.read_mappings(reads)
    assert len(base.hits) == 64
    sv0 = int(base.score_vector[5]); score_max = int(base.hits["score_max"][5])
    assert 300 <= sv0 < 10 * HAND_L and score_max == 10 * HAND_L
    seen = set()
    for want in (sv0 + 1, sv0, sv0 - 1):                                  # thresh: the hit's sv is thresh - 1, thresh, thresh + 1
        thr = -float(want) if absolute else (want + 0.5) * 100.0 / score_max
        assert item_rule(thr, 1, score_max, 0)[0] == want
        ix, s, p = hand_session(gm, sw_full_threshold=thr)
        R, c, n_run = run_hand(gm, ix, s, p, reads)
        assert np.array_equal(R.score_vector, base.score_vector) and (c["thresh"] == want).all()
        aligned = R.recs["rmapped"] > 0
        assert np.array_equal(aligned, R.score_vector >= want) and bool(aligned[5]) == (sv0 >= want)
        assert n_run == int((base.score_vector >= want).sum())
        seen.add(bool(aligned[5]))
    assert seen == {False, True}
    if not absolute:                                                      # a percentage whose product is an integer: the compare is >=, the truncation exact
        thr = sv0 * 100.0 / score_max
        if item_rule(thr, 1, score_max, 0)[0] == sv0:
            ix, s, p = hand_session(gm, sw_full_threshold=thr)
            R, _, _ = run_hand(gm, ix, s, p, reads)
            assert R.recs["rmapped"][5] > 0


@pytest.mark.gpu
def test_every_refusal_is_followed_by_a_good_call(gm):
    ix, s, p, reads = opened(gm, "cfg2s_100bp_2Mbp")
    reads = reads[:200]
    good = s.read_mappings(reads)

    def refused(call, code, word, session=s):
        with pytest.raises(gm.GmError) as e: call()
        assert "(%d)" % code in str(e.value) and word in str(e.value), str(e.value)
        if session is s:
            again = s.read_mappings(reads)
            assert again.maps.tobytes() == good.maps.tobytes() and again.cigar_buf == good.cigar_buf
    # a colour-space session: the message points to the chain of seams
    contigs, creads, _ = oa.load_golden("cfg4s_50col_2Mbp")
    pc = gm.default_params_cs(); cix = gm.Index(contigs, params=pc); cs_ = gm.Session(cix, params=pc, max_batch_reads=1024)
    creads = np.ascontiguousarray(creads[:100], dtype=np.uint8)
    refused(lambda: cs_.read_mappings(np.ascontiguousarray(creads[:, 1:])), GM_E_ARG, "gm_sw_full_cs_batch_ix", session=cs_)
    h, _ = cs_.read_hits(np.ascontiguousarray(creads[:, 1:]), initbp=creads[:, 0])      # the session serves the next call
    assert len(h) > 50
    cs_.close(); cix.close()
    # (a session has no pair mode of its own -- the paired entries take theirs as an argument, see gm_read_windows -- so there is no paired session to hand to the entry)
    # num_tmp_outputs = 65
    s65 = gm.Session(ix, params=ts.params_of(gm, "cfg2s_100bp_2Mbp", num_tmp_outputs=65), max_batch_reads=1024)
    refused(lambda: s65.read_mappings(reads), GM_E_RANGE, "num_tmp_outputs", session=s65)
    s65.close()
    # a read length out of range
    refused(lambda: s.read_mappings(np.zeros((4, s.params.longest_read_len + 1), dtype=np.uint8)), GM_E_RANGE, "out of range")
    refused(lambda: s.read_mappings(np.zeros((4, 4000), dtype=np.uint8)), GM_E_RANGE, "out of range")
    # missing outputs, missing reads: the C entry itself
    from shrimp_amd import synth
    L = gm.lib(); packed = np.ascontiguousarray(synth.pack_reads(reads), dtype=np.uint32); rd = packed.ctypes.data_as(C.POINTER(C.c_uint32))
    res = gm.ReadMappingsResult()
    refused(lambda: gm._check(L.gm_read_mappings(s.h, len(reads), 100, rd, None, 0, None, None), "gm_read_mappings"), GM_E_ARG, "bad arguments")
    refused(lambda: gm._check(L.gm_read_mappings(None, len(reads), 100, rd, None, 0, C.byref(res), None), "gm_read_mappings"), GM_E_ARG, "bad arguments")
    refused(lambda: gm._check(L.gm_read_mappings(s.h, len(reads), 100, None, None, 0, C.byref(res), None), "gm_read_mappings"), GM_E_ARG, "bad arguments")
    ib = np.zeros(len(reads), dtype=np.uint8)
    refused(lambda: gm._check(L.gm_read_mappings(s.h, len(reads), 100, rd, ib.ctypes.data_as(C.POINTER(C.c_uint8)), 0, C.byref(res), None), "gm_read_mappings"), GM_E_ARG, "colour-space")
    assert not res.hits and not res.maps and res.n_hits == 0            # after a failure the struct holds nothing to free
    L.gm_read_mappings_free(C.byref(res))
    # the mapping entry on the same session, then the call again
    assert s.map_reads(reads) == b"".join(by_read(oa.load_golden("cfg2s_100bp_2Mbp")[2], len(opened(gm, "cfg2s_100bp_2Mbp")[3]))[:len(reads)])
    again = s.read_mappings(reads)
    assert again.maps.tobytes() == good.maps.tobytes() and again.recs.tobytes() == good.recs.tobytes()


@pytest.mark.gpu
def test_release_build_gives_the_same_answers():
    """`make release` (the build bench.py measures): the chain and the reference's bytes on three fixtures in a fresh child interpreter with GM_LIB_PATH on
    libgmapper_hip_release.so"""
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    close_all()
    ids = ["[%s]" % c for c in RELEASE_CASES]
    sel = "(test_equal_to_the_chain_of_existing_entries or test_through_sam_records_to_the_bytes_of_the_reference) and (" + " or ".join(c.replace("@", " and ") for c in RELEASE_CASES) + ")"
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=dict(os.environ, GM_LIB_PATH=rel), cwd=oa.ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) == 2 * len(ids), p.stdout[-500:]
