"""gm_read_mappings_cs (Session.read_mappings_cs): colour-space pass 2 as a seam -- packed colour reads to hits, sw_full_cs records, post_sw's answers, final mappings and
their CIGAR / edit strings in one call, on arrays that stay on the device.

Without a GPU: the entry, the ctypes mirror against a C sizeof / offsetof program, the header's words; the colour-space item rule restated in Python (thresh, revcmpl, no
second score: ZV = pass 1's score, ZH = the record's score) against ZV / ZH of two reference outputs that carry --extra-sam-fields, and table() on the same records.

On the GPU the call is held to the chain of existing entries fed with its own hits (read_hits -> Index.sw_full_cs_batch -> post_sw_batch under a Python post_setup -> the
guard recipe -> select_pass2 -> sw_full_batch_text with 'H'), through sam_records to the reference's bytes and to the mapping entries, over sub-batches with a capacity
growth, with the guard forced on every read, on hand-made batches, after every refusal, and in the release build."""
import ctypes as C
import math, os, re, subprocess, sys
import numpy as np
import pytest
from tests import oracle_api as oa
from tests import test_select as ts
from tests import test_read_mappings as trm

GM_E_ARG, GM_E_RANGE = -2, -4
POST_REL = 1e-9      # the header's bound for a device posterior against the single seam's (include/gmapper_hip.h, gm_post_sw_batch "Exactness")


# ---- the rule of hit_run_full_sw for colour space (ref: gmapper/mapping.c:375-379), restated ------------------------------------------------------------------------
def item_rule_cs(sw_full_threshold, tiebreak_rev, score_max, gen_st):
    """-> (thresh, revcmpl): thresh = (int)abs_or_pct(sw_full_threshold, score_max), revcmpl = gen_st && Tflag; every hit goes through sw_full_cs, there is no second score"""
    return int(ts.abs_or_pct(sw_full_threshold, score_max)), bool(gen_st and tiebreak_rev)


def xover_rows(p, quals, qual_delta):
    """the per-position crossover scores of reads with QVs (ref: gmapper.c:532-544), as gm_map_reads_cs_fastq makes them"""
    alpha = ts.rules_of(p)["alpha"]
    out = np.zeros((len(quals), len(quals[0])), dtype=np.int32)
    for i, q in enumerate(quals):
        for j, c in enumerate(q):
            qv = c - qual_delta
            pe = .99999999 if qv <= 0 else (1E-25 if qv >= 250 else math.pow(10.0, -float(qv) / 10.0))
            cx = int(alpha * math.log(pe / 3.0) / math.log(2.0))
            out[i, j] = -1 if cx > -1 else max(cx, 2 * p.crossover_score)
    return out


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_and_the_mirror_matches_the_header(tmp_path):
    """fails without the feature; the mirror's size and field order against sizeof / offsetof of the header's struct"""
    from shrimp_amd import gmapper as G
    L = G.lib()
    hpath = os.path.join(oa.ROOT, "include", "gmapper_hip.h")
    header = open(hpath).read()
    for name in ("gm_read_mappings_cs", "gm_read_mappings_cs_free", "gm_read_mappings_cs_size"):
        assert hasattr(L, name) and name in G.EXPORTS and re.search(r"\b%s\(" % name, header), name
    assert L.gm_read_mappings_cs_size() == C.sizeof(G.ReadMappingsCsResult) == 168
    assert L.gm_read_mappings_size() == 136                              # (the letter-space struct is what it was)
    assert hasattr(G.Session, "read_mappings_cs") and issubclass(G.ReadMappingsCs, G.ReadMappings)
    fields = [f[0] for f in G.ReadMappingsCsResult._fields_]
    assert fields[:len(G.ReadMappingsResult._fields_)] == [f[0] for f in G.ReadMappingsResult._fields_]
    src = tmp_path / "m.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gmapper_hip.h"\nint main(void) {\n  printf("%zu\\n", sizeof(gm_read_mappings_cs_t));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(gm_read_mappings_cs_t, %s));\n' % (f, f) for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "m"
    subprocess.run(["cc", "-I", os.path.dirname(hpath), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(G.ReadMappingsCsResult)
    assert [tuple(l.split()) for l in out[1:] if l] == [(f, str(getattr(G.ReadMappingsCsResult, f).offset)) for f in fields]
    # the header documents every field and the rule
    doc = header[header.index("/* gm_read_mappings_cs:"):header.index("void gm_read_mappings_cs_free")]
    for f in fields: assert re.search(r"\b%s\b" % f, doc), f
    for word in ("thresh", "revcmpl", "SESSION's constants", "by_host", "flag bit 0", "GM_POST_GUARD_TOL", "post_sw_host_redo", "'H'", "gm_read_mappings)"):
        assert word in doc, word


REPLAYS = ["cfg4s_50col_2Mbp@cs_extra_rg", "stress_cs_60col_unal@seeds_contiguous"]


@pytest.mark.parametrize("golden", REPLAYS)
def test_restated_colour_rule_and_table_on_the_records_of_the_reference(golden):
    """every mapped record of the reference: ZV, pass 1's score of the hit (no second vector call), is at or above the threshold of pass 1; ZH, sw_full_cs's score, at or
    above thresh (threshscore = thresh).  table(): POS, NM and strand are the reference's on records rebuilt from its CIGAR and tags by the inverse of output.c:626-634.
    (What pins ZV and ZH of the call itself is the GPU test through gm_sam_records on cs_extra_rg.)"""
    import gzip
    from shrimp_amd import gmapper as G
    name, _, tag = golden.partition("@")
    want = []
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", golden + ".sam.gz"), "rt") as fh:
        for line in fh:
            if line.startswith("@"): continue
            t = line.rstrip("\n").split("\t")
            if int(t[1]) & 4: continue
            tags = {x[:2]: x[5:] for x in t[11:]}
            want.append((int(t[0][1:]), 1 if int(t[1]) & 16 else 0, int(t[2][len("contig"):]) - 1, int(t[3]), t[5], tags))
    assert len(want) > 500
    contigs, reads, _ = oa.load_golden(name)
    clen = np.array([len(c) for c in contigs], dtype=np.int64); L = reads.shape[1] - 1
    score_max = 10 * L
    thresh, _ = item_rule_cs(50.0, 1, score_max, 0)
    assert thresh == score_max // 2
    n = len(want)
    hits = np.zeros(n, dtype=G.PASS1_HIT_DTYPE); recs = np.zeros(n, dtype=G.SW_FULL_REC_DTYPE); maps = np.zeros(n, dtype=G.MAPPING_DTYPE)
    for i, (r, st, cn, pos, cigar, tags) in enumerate(want):
        zv, zh = int(tags["ZV"]), int(tags["ZH"])
        assert zv >= thresh and zh >= thresh, (i, zv, zh)                # pass 1's score let the hit in, sw_full_cs's score let the record out (threshscore = thresh)
        ops = [(int(a), b) for a, b in re.findall(r"(\d+)([MIDH])", cigar)]
        rmapped = sum(a for a, b in ops if b in "MI"); ins = sum(a for a, b in ops if b == "I"); dele = sum(a for a, b in ops if b == "D")
        hits[i]["read"], hits[i]["cn"], hits[i]["gen_st"], hits[i]["score_vector"], hits[i]["score_max"] = r, cn, st, zv, score_max
        recs[i]["score"], recs[i]["rmapped"], recs[i]["insertions"], recs[i]["deletions"] = zh, rmapped, ins, dele
        recs[i]["mismatches"] = int(tags["NM"]) - ins - dele; recs[i]["crossovers"] = int(tags["CM"])
        recs[i]["genome_start"] = pos - 1 if st == 0 else int(clen[cn]) - pos - (rmapped - 1 - dele + ins)      # POS turned round (ref: output.c:626-634)
        maps[i]["read"], maps[i]["hit"], maps[i]["score_full"] = r, i, int(tags["AS"])
    R = G.ReadMappingsCs(hits, np.zeros(1, dtype=np.uint64), hits["score_vector"].copy(), recs, maps, np.zeros(1, dtype=np.uint64), b"", np.zeros(n + 1, dtype=np.uint64), None, None,
                         None, clen, post=None, post_quals=b"", qralign=b"")
    t = R.table()
    assert t["pos"].tolist() == [w[3] for w in want] and t["strand"].tolist() == [w[1] for w in want] and t["contig"].tolist() == [w[2] for w in want]
    assert t["nm"].tolist() == [int(w[5]["NM"]) for w in want] and recs["crossovers"].tolist() == [int(w[5]["CM"]) for w in want]
    assert sum(w[1] for w in want) > 100


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


def _fq():
    from tests.test_oracle import _cs_fastq_case
    return _cs_fastq_case()


def load_case(name):
    """-> dict(contigs, cnames, reads [n, 1 + colours], names, quals, qual_delta) of a fixture"""
    if name == "cfg4s_50col_fq":
        contigs, reads, quals, delta, _ = _fq()
        return dict(contigs=contigs, cnames=None, reads=np.ascontiguousarray(reads, dtype=np.uint8), names=None, quals=quals, qual_delta=delta)
    if name == "split_cs_50col":
        from tests import test_many_contigs as tmc
        F = tmc.fixture(name)
        return dict(contigs=F["contigs"], cnames=None, reads=np.ascontiguousarray(F["reads"], dtype=np.uint8), names=None, quals=None, qual_delta=33)
    if name in ("rna_cs", "rna_cs_fq"):
        g = oa.load_rna_case(name); names, codes, quals = g["reads"][0]
        return dict(contigs=g["contigs"], cnames=g["contig_names"], reads=np.ascontiguousarray(codes, dtype=np.uint8), names=names, quals=quals, qual_delta=33)
    contigs, reads, _ = oa.load_golden(name)
    return dict(contigs=contigs, cnames=None, reads=np.ascontiguousarray(reads, dtype=np.uint8), names=None, quals=None, qual_delta=33)


def golden_text(name, tag):
    import gzip
    if name == "split_cs_50col":
        from tests import test_many_contigs as tmc
        return tmc.golden(name, tag)
    if name in ("rna_cs", "rna_cs_fq"): return oa.load_rna_case(name)["sam"]
    if name == "cfg4s_50col_fq" and not tag: return _fq()[4]
    if tag: return oa.load_option_sam(name, tag)
    return oa.load_golden(name)[2]


CSO = oa.CS_OPTION_CASES
UNAL = dict(sam_unaligned=1)
# case -> (fixture, golden tag or None, gm_params_t fields)
CASES = {
    "cfg4s_50col_2Mbp": ("cfg4s_50col_2Mbp", None, {}),
    "cfg4s_50col_2Mbp@cs_extra_rg": ("cfg4s_50col_2Mbp", "cs_extra_rg", dict(extra_sam_fields=1, read_group=b"grp1", sam_unaligned=1)),
    "cfg4s_50col_2Mbp@cs_local": ("cfg4s_50col_2Mbp", "cs_local", CSO["cs_local"][2]),
    "cfg4s_50col_2Mbp@cs_no_mapq": ("cfg4s_50col_2Mbp", "cs_no_mapq", CSO["cs_no_mapq"][2]),
    "cfg4s_50col_2Mbp@cs_ungapped": ("cfg4s_50col_2Mbp", "cs_ungapped", CSO["cs_ungapped"][2]),
    "cfg4s_50col_fq": ("cfg4s_50col_fq", None, UNAL),
    "cfg4s_50col_fq@cs_fq_local": ("cfg4s_50col_fq", "cs_fq_local", dict(sam_unaligned=1, local_alignment=1)),
    "stress_cs_60col_unal": ("stress_cs_60col_unal", None, UNAL),
    "stress_cs_60col_unal@cs_tiebreak_off": ("stress_cs_60col_unal", "cs_tiebreak_off", CSO["cs_tiebreak_off"][2]),
    "stress_cs_60col_unal@cs_single_best": ("stress_cs_60col_unal", "cs_single_best", CSO["cs_single_best"][2]),
    "stress_cs_60col_unal@cs_xover_taboo": ("stress_cs_60col_unal", "cs_xover_taboo", CSO["cs_xover_taboo"][2]),
    "stress_cs_60col_unal@cs_scores_swapped": ("stress_cs_60col_unal", "cs_scores_swapped", CSO["cs_scores_swapped"][2]),
    "stress_cs_60col_unal@cs_gate_under": ("stress_cs_60col_unal", "cs_gate_under", CSO["cs_gate_under"][2]),
    "stress_cs_60col_unal@cs_gate_over": ("stress_cs_60col_unal", "cs_gate_over", CSO["cs_gate_over"][2]),
    "split_cs_50col": ("split_cs_50col", None, {}),
    "rna_cs": ("rna_cs", None, UNAL),
    "rna_cs_fq": ("rna_cs_fq", None, UNAL),
}
RELEASE_CASES = ["cfg4s_50col_fq", "stress_cs_60col_unal@cs_xover_taboo"]
_open, _index, _answers, _hand = {}, {}, {}, {}


def opened(gm, case, max_batch_reads=8192):
    """(index, session, params, fixture dict) of a case; the cases of a genome share its index"""
    if case not in _open:
        name, tag, fields = CASES[case]
        F = load_case(name)
        p = gm.default_params_cs()
        for k, v in fields.items(): setattr(p, k, v)
        key = "cfg4s_50col_2Mbp" if name == "cfg4s_50col_fq" else ("rna_cs" if name == "rna_cs_fq" else name)
        if key not in _index: _index[key] = gm.Index(F["contigs"], names=F["cnames"], params=gm.default_params_cs())
        _open[case] = (_index[key], gm.Session(_index[key], params=p, max_batch_reads=max_batch_reads), p, F)
    return _open[case]


def close_all():
    for _, s, _, _ in _open.values(): s.close()
    for k, v in _hand.items():
        if k != "g": v[0].close()
    for ix in _index.values(): ix.close()
    _open.clear(); _index.clear(); _answers.clear(); _hand.clear()


@pytest.fixture(scope="module", autouse=True)
def release_at_the_end():
    yield
    close_all()


def use_q(p, F): return F["quals"] is not None and not p.ignore_qvs


def chain_of(gm, ix, s, p, F, R, reads=None, quals=None):
    """the call's own hits through the existing entries (the recipe of tests/test_select.py:654-731, colour space) -> dict(recs, ops, post, qralign, quals, maps,
    map_off, cigar, edit, redone)"""
    from shrimp_amd import synth
    reads = F["reads"] if reads is None else reads; quals = F["quals"] if quals is None else quals
    hits, hit_off = R.hits, R.hit_off; n = len(hits); cols = np.ascontiguousarray(reads[:, 1:]); L = cols.shape[1]
    mqv_on = not p.local_alignment and not p.no_mapping_qualities
    qv = quals is not None and not p.ignore_qvs
    empty = dict(recs=np.zeros(0, dtype=gm.SW_FULL_REC_DTYPE), ops=b"", post=None, qralign=b"", quals=None, cigar=None, edit=None, redone=0)
    if n == 0:
        maps, map_off = s.select_pass2(hits, hit_off, empty["recs"], np.zeros(0, dtype=gm.POST_REC_DTYPE) if mqv_on else None)
        return dict(empty, maps=maps, map_off=map_off)
    rw = np.ascontiguousarray(synth.pack_reads(cols))[hits["read"]]; ib = reads[hits["read"], 0]; lens = np.full(n, L)
    thresh = np.array([item_rule_cs(p.sw_full_threshold, p.tiebreak_rev, int(sm), 0)[0] for sm in hits["score_max"]], dtype=np.int32)
    anchors = [(int(h["ax"]), int(h["ay"]), int(h["alen"]), int(h["awidth"])) for h in hits]
    cn, gst, goff, wl = hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"]
    revcmpl = (hits["gen_st"] == 1).astype(np.uint8) if p.tiebreak_rev else None
    xover = xover_rows(p, quals, F["qual_delta"])[hits["read"]] if qv else None
    hq = [quals[int(r)] for r in hits["read"]] if qv else None
    gm.sw_full_cs_setup(max(1400, 2 * L), max(1000, L), p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score,
                        p.crossover_score, True, p.anchor_width, p.indel_taboo_len)      # (ts.full_setup with sizes that follow the reads)
    recs, ops, strings = ix.sw_full_cs_batch(cn, gst, goff, wl, rw, lens, ib, anchors, revcmpl=revcmpl, threshscore=thresh, xover=xover, local_alignment=bool(p.local_alignment))
    assert (recs["status"] == 0).all()
    post = None; qbuf = None; pq = None; redone = 0
    if mqv_on:
        Rl = ts.rules_of(p); a, b = Rl["alpha"], Rl["beta"]
        pr_mm = 1.0 / (1.0 + 1.0 / 3.0 * math.pow(2.0, (float(p.match_score) - float(p.mismatch_score)) / a))
        gm.post_sw_setup(max(1400, 3 * L), pr_mm, p.pr_xover, math.pow(2.0, float(p.a_gap_open_score) / a), math.pow(2.0, float(p.a_gap_extend_score) / a),
                         math.pow(2.0, float(p.b_gap_open_score) / a), math.pow(2.0, (float(p.b_gap_extend_score) - b) / a), use_read_qvs=qv, use_sanger_qvs=True,
                         qual_vector_offset=0, qual_delta=F["qual_delta"])
        post, qralign, qual = ix.post_sw_batch(cn, gst, recs, ops, rw, lens, ib, quals=hq)
        assert (post["status"] == 0).all()
        qbuf = bytes(qralign.buffer); pq = bytes(qual.buffer)
        maps, map_off = s.select_pass2(hits, hit_off, recs, post)
        flagged = sorted(set(maps["read"][(maps["flags"] & 1) != 0].tolist()))
        if flagged:                                                      # the header's recipe
            strings.prefetch(); post = post.copy(); qb = bytearray(qbuf); pqb = bytearray(pq)
            for r in flagged:
                for i in range(int(hit_off[r]), int(hit_off[r + 1])):
                    if recs[i]["score"] <= 0 or post[i]["by_host"]: continue
                    db, qr = strings(i)
                    one = gm.post_sw(rw[i], int(ib[i]), db, qr, int(recs[i]["read_start"]), qual=hq[i] if qv else None)
                    post[i]["posterior"] = one["posterior"]; post[i]["by_host"] = 1; redone += 1
                    post[i]["matches"], post[i]["mismatches"], post[i]["crossovers"] = one["matches"], one["mismatches"], one["crossovers"]
                    qb[int(recs[i]["ops_off"]):int(recs[i]["ops_off"]) + int(recs[i]["n_ops"])] = one["qralign"].encode()
                    pqb[int(post[i]["qual_off"]):int(post[i]["qual_off"]) + int(post[i]["qual_len"])] = one["qual"].encode()[:int(post[i]["qual_len"])]
            qbuf = bytes(qb); pq = bytes(pqb)
            maps, map_off = s.select_pass2(hits, hit_off, recs, post)
            assert not (maps["flags"] & 1).any()
    else:
        maps, map_off = s.select_pass2(hits, hit_off, recs, None)
    status, _, qra, cigar, edit = ix.sw_full_batch_text(cn, gst, recs, ops, rw, lens, initbp=ib, qralign=qbuf, reverse=(hits["gen_st"] == 1).astype(np.uint8), clip="H",
                                                        what=("align", "cigar", "edit"), colour_space=True)
    assert (status == 0).all()
    if qbuf is None: qbuf = bytes(qra.buffer)
    return dict(recs=recs, ops=bytes(ops), post=post, qralign=qbuf, quals=pq, maps=maps, map_off=map_off, cigar=cigar, edit=edit, redone=redone)


INT_FIELDS = ("read", "hit", "score_full", "pct_score_full", "mqv", "flags")


def single_seam_posteriors(gm, ix, p, F, R, idx):
    """post_sw, the single seam, under a Python post_setup on the hits idx of R: sw_full_cs's own strings from Index.sw_full_cs_batch -> their posteriors (float64)"""
    from shrimp_amd import synth
    reads, quals = F["reads"], F["quals"]; hits = R.hits[idx]; n = len(hits); cols = np.ascontiguousarray(reads[:, 1:]); L = cols.shape[1]
    qv = quals is not None and not p.ignore_qvs
    rw = np.ascontiguousarray(synth.pack_reads(cols))[hits["read"]]; ib = reads[hits["read"], 0]
    thresh = np.array([item_rule_cs(p.sw_full_threshold, p.tiebreak_rev, int(sm), 0)[0] for sm in hits["score_max"]], dtype=np.int32)
    anchors = [(int(h["ax"]), int(h["ay"]), int(h["alen"]), int(h["awidth"])) for h in hits]
    ts.full_setup(gm, p)
    recs, ops, strings = ix.sw_full_cs_batch(hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"], rw, np.full(n, L), ib, anchors,
                                             revcmpl=(hits["gen_st"] == 1).astype(np.uint8) if p.tiebreak_rev else None, threshscore=thresh,
                                             xover=xover_rows(p, quals, F["qual_delta"])[hits["read"]] if qv else None)
    Rl = ts.rules_of(p); a, b = Rl["alpha"], Rl["beta"]
    pr_mm = 1.0 / (1.0 + 1.0 / 3.0 * math.pow(2.0, (float(p.match_score) - float(p.mismatch_score)) / a))
    gm.post_sw_setup(1400, pr_mm, p.pr_xover, math.pow(2.0, float(p.a_gap_open_score) / a), math.pow(2.0, float(p.a_gap_extend_score) / a),
                     math.pow(2.0, float(p.b_gap_open_score) / a), math.pow(2.0, (float(p.b_gap_extend_score) - b) / a), use_read_qvs=qv, use_sanger_qvs=True,
                     qual_vector_offset=0, qual_delta=F["qual_delta"])
    strings.prefetch()
    out = np.zeros(n, dtype=np.float64)
    for i in range(n):
        db, qr = strings(i)
        out[i] = gm.post_sw(rw[i], int(ib[i]), db, qr, int(recs[i]["read_start"]), qual=quals[int(hits["read"][i])] if qv else None)["posterior"]
    return out


def assert_equals_chain(gm, p, R, c):
    """every array of the call against the chain's: bytes and integers equal, the doubles within the header's bound; -> were the doubles bit-equal"""
    n = len(R.hits); mqv_on = not p.local_alignment and not p.no_mapping_qualities
    assert R.hits.dtype == gm.PASS1_HIT_DTYPE and R.recs.dtype == gm.SW_FULL_REC_DTYPE and R.maps.dtype == gm.MAPPING_DTYPE
    assert len(R.recs) == len(R.score_vector) == n == int(R.hit_off[-1]) and len(R.cigar_off) == n + 1
    assert np.array_equal(R.score_vector, R.hits["score_vector"])      # ZV: pass 1's score
    for f in gm.SW_FULL_REC_DTYPE.names: assert np.array_equal(R.recs[f], c["recs"][f]), f      # (the chain's operations are compacted in hit order too: ops_off included)
    if R.ops is not None: assert R.ops.tobytes() == c["ops"]
    assert len(R.qralign) == int(R.recs["n_ops"].sum())
    mapped = np.zeros(n, dtype=bool); mapped[R.maps["hit"]] = True
    if mqv_on:
        assert R.post is not None and R.post.dtype == gm.POST_REC_DTYPE
        for f in ("matches", "mismatches", "crossovers", "qual_len", "status", "by_host"): assert np.array_equal(R.post[f], c["post"][f]), f
        assert R.qralign == c["qralign"] and R.post_quals == c["quals"]
        got, want = R.post["posterior"], c["post"]["posterior"]
        assert (np.abs(got - want) <= POST_REL * np.abs(want)).all()
    else:
        assert R.post is None and R.post_quals == b""
        for i in range(n):
            a, k = int(R.recs["ops_off"][i]), int(R.recs["n_ops"][i])
            assert R.qralign[a:a + k] == (c["qralign"][a:a + k] if mapped[i] else b"\0" * k), i
    assert np.array_equal(R.map_off, c["map_off"])
    for f in INT_FIELDS: assert np.array_equal(R.maps[f], c["maps"][f]), f
    assert not (R.maps["flags"] & 1).any()
    for f in ("posterior", "z0", "z1"): assert (np.abs(R.maps[f] - c["maps"][f]) <= POST_REL * np.abs(c["maps"][f])).all(), f
    for i in range(n):
        if mapped[i]:
            assert R.cigar(i) == c["cigar"](i), i
            if p.extra_sam_fields: assert R.edit(i) == c["edit"](i), i
        else:
            assert R.cigar(i) == b"" and (not p.extra_sam_fields or R.edit(i) == b"")
    assert (R.edit_off is not None) == bool(p.extra_sam_fields)
    return R.maps.tobytes() == c["maps"].tobytes() and (not mqv_on or R.post["posterior"].tobytes() == c["post"]["posterior"].tobytes())


def answer(gm, case):
    if case not in _answers:
        ix, s, p, F = opened(gm, case)
        R = s.read_mappings_cs(F["reads"], quals=F["quals"], qual_delta=F["qual_delta"], want_ops=True)
        _answers[case] = (R, dict(s.stats))
    return _answers[case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_equal_to_the_chain_of_existing_entries(gm, case):
    ix, s, p, F = opened(gm, case)
    R, st = answer(gm, case)
    c = chain_of(gm, ix, s, p, F, R)
    bit_equal = assert_equals_chain(gm, p, R, c)
    print("posteriors bit-equal to the chain's:", case, bit_equal, "host re-dos:", st["post_sw_host_redo"])
    assert len(R.hits) > 200 and len(R.maps) > 100
    assert st["full_calls"] == len(R.hits) and st["reads"] == len(F["reads"])
    hits2, off2 = s.read_hits(np.ascontiguousarray(F["reads"][:, 1:]), initbp=F["reads"][:, 0])
    assert np.array_equal(off2, R.hit_off)
    skip = tied(s, F)
    plain = ~np.isin(R.hits["read"], list(skip))
    assert np.array_equal(ts.hit_rows(R.hits)[plain], ts.hit_rows(hits2)[plain])
    # without the operations: the same records
    R2 = s.read_mappings_cs(F["reads"], quals=F["quals"], qual_delta=F["qual_delta"])
    assert R2.ops is None and R2.maps.tobytes() == R.maps.tobytes() and R2.cigar_buf == R.cigar_buf and R2.qralign == R.qralign
    if not skip: assert R2.recs.tobytes() == R.recs.tobytes()


def tied(s, F):
    """reads that own a group of equal windows (which of the group a hit names is no promise of gm_read_windows): at most 33 on any fixture used"""
    wins, _ = s.read_windows(np.ascontiguousarray(F["reads"][:, 1:]), initbp=F["reads"][:, 0])
    rows = ts.win_rows(wins)
    skip = set(rows[ts.tie_mask(rows)][:, 0].tolist())
    assert len(skip) <= 33
    return skip


def sam_of(s, F, R, reads=None):
    reads = F["reads"] if reads is None else reads
    got, off = s.sam_records(np.ascontiguousarray(reads[:, 1:]), R, initbp=reads[:, 0], names=F["names"], quals=F["quals"], qual_delta=F["qual_delta"])
    return [got[int(off[r]):int(off[r + 1])] for r in range(len(reads))]


def by_read(sam, names, n):
    if names is None: return trm.by_read(sam, n)
    index = {nm: i for i, nm in enumerate(names)}; out = [b""] * n
    for l in sam.splitlines(keepends=True):
        if not l.startswith(b"@"): out[index[l.split(b"\t", 1)[0]]] += l
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_through_sam_records_to_the_bytes_of_the_reference(gm, case):
    name, tag, fields = CASES[case]
    ix, s, p, F = opened(gm, case)
    R, _ = answer(gm, case)
    n = len(F["reads"])
    mine = sam_of(s, F, R)
    skip = tied(s, F)
    entry_text = s.map_reads_cs_fastq(F["reads"], F["quals"], F["qual_delta"], names=F["names"]) if F["quals"] is not None else s.map_reads_cs(F["reads"], names=F["names"])
    entry = by_read(entry_text, F["names"], n)
    bad = [r for r in range(n) if r not in skip and mine[r] != entry[r]]
    assert not bad, (len(bad), [(mine[r], entry[r]) for r in bad[:3]])
    want = by_read(golden_text(name, tag), F["names"], n)
    bad = [r for r in range(n) if r not in skip and mine[r] != want[r]]
    assert not bad, (len(bad), [(mine[r], want[r]) for r in bad[:3]])
    assert sum(1 for r in range(n) if r not in skip and want[r]) > 200
    assert oa.sam_header(F["contigs"], F["cnames"]) + entry_text == golden_text(name, tag)      # afterwards the mapping entry on that session still prints the golden


@pytest.mark.gpu
def test_sub_batches_with_a_capacity_growth(gm):
    """five sub-batches, and sub-batches one of which holds a read of a tandem repeat whose window row overflows (the capacity grows and the sub-batch runs again):
    the result of a session that takes the reads in one sub-batch"""
    _, unit = hand_genome()
    tandem = colour_read(np.concatenate([unit[10:], unit[:10]])[:HAND_L], 2)[None, :]
    hand_reads = np.concatenate([cut_colour_reads(70, HAND_L, 21, errors=1), tandem, cut_colour_reads(57, HAND_L, 22, errors=1)])
    for case, small, n, grows in (("cfg4s_50col_fq", 64, 300, False), ("hand", 32, None, True)):
        if case == "hand":
            ix, s1, p = hand_session(gm); F = dict(reads=hand_reads, quals=None, qual_delta=33)
        else: ix, s1, p, F = opened(gm, case)
        reads = F["reads"][:n] if n else F["reads"]; quals = F["quals"][:len(reads)] if F["quals"] is not None else None
        one = s1.read_mappings_cs(reads, quals=quals, qual_delta=F["qual_delta"], want_ops=True)
        s = gm.Session(ix, params=p, max_batch_reads=small)
        many = s.read_mappings_cs(reads, quals=quals, qual_delta=F["qual_delta"], want_ops=True); st = dict(s.stats)
        s.close()
        assert len(reads) > 4 * small or not n
        print(case, "retries", st["retries"])
        assert st["reads"] == len(reads) and (st["retries"] >= 1 or not grows)
        skip = tied(s1, dict(F, reads=reads))
        if not skip:
            for f in ("hits", "hit_off", "score_vector", "recs", "maps", "map_off", "cigar_off", "ops", "post"):
                assert getattr(one, f).tobytes() == getattr(many, f).tobytes(), f
            assert one.cigar_buf == many.cigar_buf and one.qralign == many.qralign and one.post_quals == many.post_quals
        else:
            keep = ~np.isin(one.maps["read"], list(skip))
            assert np.array_equal(one.hit_off, many.hit_off) and np.array_equal(one.map_off, many.map_off) and one.maps[keep].tobytes() == many.maps[keep].tobytes()
        assert np.array_equal(many.hits["read"][many.maps["hit"]], many.maps["read"]) and (np.diff(many.hits["read"]) >= 0).all()
        assert np.array_equal(many.post["qual_off"], np.concatenate([[0], np.cumsum(many.post["qual_len"].astype(np.uint64))[:-1]]).astype(np.uint64))


GUARD_CHILD = r"""
import os, sys, pickle
import numpy as np
sys.path.insert(0, sys.argv[1])
from shrimp_amd import gmapper as gm
from tests import test_read_mappings_cs as T
out = {}
for case in ("cfg4s_50col_2Mbp", "cfg4s_50col_fq"):
    ix, s, p, F = T.opened(gm, case)
    R = s.read_mappings_cs(F["reads"], quals=F["quals"], qual_delta=F["qual_delta"], want_ops=True)
    k = R.maps["hit"][:40]
    seam = T.single_seam_posteriors(gm, ix, p, F, R, k) if os.environ.get("GM_POST_GUARD_TOL") else None
    out[case] = dict(seam=seam, seam_hits=k, maps=R.maps, post=R.post, recs=R.recs, cigar=R.cigar_buf, qralign=R.qralign, post_quals=R.post_quals, redo=s.stats["post_sw_host_redo"], sam=b"".join(T.sam_of(s, F, R)))
T.close_all()
pickle.dump(out, open(sys.argv[2], "wb"))
"""


@pytest.mark.gpu
def test_the_guard_forced_on_every_read_changes_no_byte(gm, tmp_path):
    """GM_POST_GUARD_TOL huge (set before the tuning library is loaded, in a child interpreter): every read with a mapping goes through the re-do; bytes and integers
    are the default run's, the posteriors the single seam's bits, no mapping is flagged in either run"""
    import pickle
    close_all()
    res = {}
    for tol in (None, "0.49"):
        env = dict(os.environ); env.pop("GM_LIB_PATH", None); env.pop("GM_POST_GUARD_TOL", None)
        if tol: env["GM_POST_GUARD_TOL"] = tol
        out = str(tmp_path / ("g%s.pkl" % (tol or "d")))
        p = subprocess.run([sys.executable, "-c", GUARD_CHILD, oa.ROOT, out], capture_output=True, text=True, env=env, cwd=oa.ROOT, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        res[tol] = pickle.load(open(out, "rb"))
    for case in res[None]:
        d, g = res[None][case], res["0.49"][case]
        print(case, "host re-dos: default", d["redo"], "forced", g["redo"])
        assert g["redo"] > d["redo"] >= 0 and g["redo"] > 0
        assert not (d["maps"]["flags"] & 1).any() and not (g["maps"]["flags"] & 1).any()
        for f in INT_FIELDS: assert np.array_equal(d["maps"][f], g["maps"][f]), f
        for f in ("matches", "mismatches", "crossovers", "qual_len", "qual_off", "status"): assert np.array_equal(d["post"][f], g["post"][f]), f
        assert d["recs"].tobytes() == g["recs"].tobytes() and d["cigar"] == g["cigar"] and d["qralign"] == g["qralign"] and d["post_quals"] == g["post_quals"] and d["sam"] == g["sam"]
        mapped = np.zeros(len(g["post"]), dtype=bool); mapped[g["maps"]["hit"]] = True
        assert (g["post"]["by_host"][mapped] == 1).all()               # every mapping's posterior is the host routine's:
        assert len(g["seam"]) == 40 and g["post"]["posterior"][g["seam_hits"]].tobytes() == g["seam"].tobytes()      # the single seam's bits, under a Python post_setup
        for f in ("posterior", "z0", "z1"): assert (np.abs(d["maps"][f] - g["maps"][f]) <= POST_REL * np.abs(g["maps"][f])).all(), f


# ---- hand-made batches on a small index ---------------------------------------------------------------------------------------------------------------------------
HAND_L = 50
CS_XOR = np.array([[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]], dtype=np.uint8)


def colour_read(letters, primer):
    """letters (codes 0..3) sequenced in colour space behind primer letter `primer`: [primer, colours...]"""
    seq = np.concatenate([[primer], letters]).astype(np.uint8)
    return np.concatenate([[primer], CS_XOR[seq[:-1], seq[1:]]]).astype(np.uint8)


def hand_genome():
    if "g" not in _hand:
        rng = np.random.default_rng(20252)
        unit = rng.integers(0, 4, 100).astype(np.uint8)
        c0 = rng.integers(0, 4, 40000).astype(np.uint8); c1 = rng.integers(0, 4, 20000).astype(np.uint8)
        c2 = np.concatenate([rng.integers(0, 4, 500).astype(np.uint8), np.tile(unit, 300), rng.integers(0, 4, 500).astype(np.uint8)])      # a tandem repeat: 300 copies of a unit
        _hand["g"] = ([c0, c1, c2], unit)
    return _hand["g"]


def hand_session(gm, **fields):
    key = tuple(sorted(fields.items()))
    if key not in _hand:
        contigs, _ = hand_genome()
        ix = _index.get("hand")
        if ix is None: ix = _index["hand"] = gm.Index(contigs, params=gm.default_params_cs())
        p = gm.default_params_cs()
        for k, v in fields.items(): setattr(p, k, v)
        _hand[key] = (gm.Session(ix, params=p, max_batch_reads=256), p)
    return _index["hand"], _hand[key][0], _hand[key][1]


def cut_colour_reads(n, L, seed, errors=0, contig=None, contigs=None):
    """n reads of L colours from distinct places, every second one from the reverse strand, every primer letter; `errors` colour errors in the middle third"""
    if contigs is None: contigs, _ = hand_genome()
    rng = np.random.default_rng(seed)
    out = np.zeros((n, L + 1), dtype=np.uint8)
    for k in range(n):
        c = contigs[contig if contig is not None else (0 if k % 3 else 1)]
        at = 100 + k * ((len(c) - 300 - L) // max(n, 1))
        letters = c[at:at + L].copy(); letters[letters == 4] = 3           # (a read of an RNA contig is sequenced as T)
        if k & 1: letters = ts.CMPL[letters[::-1]]
        primer = k % 4
        r = colour_read(letters, primer)
        for j in range(errors): r[1 + L // 3 + 3 * j] = (r[1 + L // 3 + 3 * j] + 1 + rng.integers(0, 3)) & 3
        out[k] = r
    return out


def run_hand(gm, ix, s, p, reads, quals=None, qual_delta=33):
    F = dict(reads=reads, quals=quals, qual_delta=qual_delta)
    R = s.read_mappings_cs(reads, quals=quals, qual_delta=qual_delta, want_ops=True)
    c = chain_of(gm, ix, s, p, F, R)
    assert_equals_chain(gm, p, R, c)
    return R, c


@pytest.mark.gpu
def test_hand_made_edges(gm):
    contigs, unit = hand_genome()
    ix, s, p = hand_session(gm)
    # every primer letter, both strands
    reads = cut_colour_reads(40, HAND_L, 3, errors=1)
    R, c = run_hand(gm, ix, s, p, reads)
    assert len(R.maps) >= 35 and set(R.hits["gen_st"][R.maps["hit"]].tolist()) == {0, 1}
    assert set(reads[R.maps["read"], 0].tolist()) == {0, 1, 2, 3}
    # RNA contigs (U and no T), in a small genome of their own: the last contig's flag is the genome's (ref: genome.c:1063-1064).  U is rare in them, as in the rna_cs
    # fixtures: reads planted on random contigs with a quarter of U found no hit at all, neither here nor among the DNA contigs
    rng = np.random.default_rng(20253)
    rna = [rng.choice(np.array([0, 1, 2, 4], dtype=np.uint8), size=n_, p=[.32, .33, .32, .03]) for n_ in (9000, 7000)]
    rix = gm.Index(rna, params=gm.default_params_cs()); rs = gm.Session(rix, params=gm.default_params_cs(), max_batch_reads=256)
    try:
        assert rix.genome_is_rna()
        R, c = run_hand(gm, rix, rs, gm.default_params_cs(), cut_colour_reads(24, HAND_L, 4, errors=1, contigs=rna))
        print("RNA genome: mapped reads", sorted(set(R.maps["read"].tolist())), "of 24 (odd: planted on the reverse strand)")
        assert set(R.hits["cn"][R.maps["hit"]].tolist()) == {0, 1}      # (the comparison with the chain above is not vacuous: mappings on either RNA contig)
    finally:
        rs.close(); rix.close()
    # a batch without a window, and no reads
    rng = np.random.default_rng(99)
    noise = np.concatenate([rng.integers(0, 4, (50, 1)), rng.integers(0, 4, (50, HAND_L))], axis=1).astype(np.uint8)
    E = s.read_mappings_cs(noise, want_ops=True)
    assert len(E.hits) == len(E.recs) == len(E.maps) == len(E.ops) == len(E.post) == 0 and E.cigar_buf == E.qralign == E.post_quals == b""
    assert E.hit_off.tolist() == [0] * 51 == E.map_off.tolist() and E.cigar_off.tolist() == [0] and len(E.table()) == 0
    Z = s.read_mappings_cs(np.zeros((0, HAND_L + 1), dtype=np.uint8))
    assert len(Z.hits) == len(Z.maps) == 0 and Z.hit_off.tolist() == [0] == Z.map_off.tolist() == Z.cigar_off.tolist() and Z.ops is None
    # a read with 64 hits from a tandem repeat
    ix64, s64, p64 = hand_session(gm, num_tmp_outputs=64, num_outputs=64)
    tandem = colour_read(np.concatenate([unit[10:], unit[:10]])[:HAND_L], 2)[None, :]
    reads = np.concatenate([cut_colour_reads(10, HAND_L, 5), tandem, cut_colour_reads(10, HAND_L, 6)])
    R, c = run_hand(gm, ix64, s64, p64, reads)
    assert int(np.diff(R.hit_off.astype(np.int64))[10]) == 64 and int(np.diff(R.map_off.astype(np.int64))[10]) >= 60
    # every hit under the threshold of the full alignment: zero records, no post item
    ixh, sh, ph = hand_session(gm, sw_full_threshold=99.0)
    reads = cut_colour_reads(30, HAND_L, 7, errors=3)
    R, c = run_hand(gm, ixh, sh, ph, reads)
    assert len(R.hits) >= 20 and not R.recs["score"].any() and len(R.maps) == 0 and R.post_quals == b"" and not R.post["qual_len"].any() and R.qralign == b""
    # the first and the last base of a contig, either strand
    ends = []
    for c_ in (contigs[0], contigs[1]):
        for letters in (c_[:HAND_L], c_[-HAND_L:]):
            ends.append(colour_read(letters, 1)); ends.append(colour_read(ts.CMPL[letters[::-1]], 3))
    R, c = run_hand(gm, ix, s, p, np.array(ends, dtype=np.uint8))
    assert len(R.maps) >= 6
    # QVs at the ends of the accepted range, and ignore_qvs
    reads = cut_colour_reads(40, HAND_L, 8, errors=1)
    quals = [bytes([33] * 10 + [33 + 93] * 10 + [33 + 20] * (HAND_L - 20)) if k % 2 else bytes([33 + 93] * HAND_L) for k in range(40)]
    R, c = run_hand(gm, ix, s, p, reads, quals=quals)
    assert len(R.maps) >= 30
    ixi, si, pi = hand_session(gm, ignore_qvs=1)
    Ri, ci = run_hand(gm, ixi, si, pi, reads, quals=quals)
    plain = s.read_mappings_cs(reads, want_ops=True)
    assert Ri.maps.tobytes() == plain.maps.tobytes() and Ri.recs.tobytes() == plain.recs.tobytes() and Ri.qralign == plain.qralign
    # the shortest reads the default seeds admit
    R, c = run_hand(gm, ix, s, p, cut_colour_reads(60, 25, 10))
    assert len(R.hits) > 0


@pytest.mark.gpu
def test_the_longest_reads_the_entry_admits(gm):
    """The largest length the entry's admission tests accept on this index, found by bisection on the entry itself (gm_sw_full_cs_batch_lds, gm_score_windows_lds and
    the front's prune-kernel bound, which on an index this small binds first): planted reads of that length against the chain -- windows of 1.4 times the read, a
    back scratch whose 512 MB budget leaves fewer waves than hits, a post_sw column scratch of that many columns -- and that length + 1 refused, then a good call"""
    ix, s, p = hand_session(gm, longest_read_len=3000)
    def admitted(L):
        try: s.read_mappings_cs(np.zeros((2, L + 1), dtype=np.uint8)); return True
        except gm.GmError as e:
            assert "(%d)" % GM_E_RANGE in str(e) and "LDS" in str(e), str(e)
            return False
    lo, hi = 150, 3000
    assert admitted(lo) and not admitted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if admitted(mid): lo = mid
        else: hi = mid
    print("the longest reads admitted:", lo, "colours")
    assert lo >= 500
    reads = cut_colour_reads(48, lo, 9, errors=5)
    R, c = run_hand(gm, ix, s, p, reads)
    W = int(R.hits["w_len"].max()); stride = W * lo * 12 + 256
    print("hits", len(R.hits), "mappings", len(R.maps), "longest window", W, "waves the back scratch leaves", (512 << 20) // stride)
    assert len(R.maps) >= 40 and len(R.hits) > (512 << 20) // stride      # the budget, not the hits, set the grid
    with pytest.raises(gm.GmError) as e: s.read_mappings_cs(np.zeros((2, lo + 2), dtype=np.uint8))
    assert "(%d)" % GM_E_RANGE in str(e.value)
    again = s.read_mappings_cs(reads, want_ops=True)
    assert again.maps.tobytes() == R.maps.tobytes() and again.recs.tobytes() == R.recs.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("absolute", [False, True])
def test_threshold_boundary(gm, absolute):
    """records whose score is thresh - 1, thresh and thresh + 1, under a percentage and under an absolute threshold (local mode: no posterior rescales the score)"""
    reads = cut_colour_reads(48, HAND_L, 11, errors=2)
    ix0, s0, p0 = hand_session(gm, local_alignment=1, sw_full_threshold=30.0)
    base = s0.read_mappings_cs(reads)
    k = int(np.argmax(base.recs["score"] > 0)); sc = int(base.recs["score"][k]); score_max = int(base.hits["score_max"][k])
    assert 0 < sc <= score_max == 10 * HAND_L
    seen = set()
    for want in (sc + 1, sc, sc - 1):
        thr = -float(want) if absolute else (want + 0.5) * 100.0 / score_max
        assert item_rule_cs(thr, 1, score_max, 0)[0] == want
        ix, s, p = hand_session(gm, local_alignment=1, sw_full_threshold=thr)
        R, c = run_hand(gm, ix, s, p, reads)
        if len(R.hits) == len(base.hits): assert np.array_equal(R.recs["score"] > 0, base.recs["score"] >= want)
        j = np.nonzero((R.hits["read"] == base.hits["read"][k]) & (R.hits["g_off"] == base.hits["g_off"][k]))[0]
        if len(j): seen.add(bool(R.recs["score"][j[0]] > 0)); assert bool(R.recs["score"][j[0]] > 0) == (sc >= want)
    assert seen == {False, True}


@pytest.mark.gpu
def test_every_refusal_is_followed_by_a_good_call(gm):
    from shrimp_amd import synth
    ix, s, p, F = opened(gm, "cfg4s_50col_fq")
    reads = F["reads"][:200]; quals = F["quals"][:200]; qd = F["qual_delta"]
    # a post_sw_setup with other constants on the calling thread: neither read nor disturbed
    gm.post_sw_setup(77, 0.2, 0.3, 0.01, 0.5, 0.02, 0.6)
    good = s.read_mappings_cs(reads, quals=quals, qual_delta=qd)
    ts.post_setup(gm, p)
    again = s.read_mappings_cs(reads, quals=quals, qual_delta=qd)
    assert again.maps.tobytes() == good.maps.tobytes() and again.post.tobytes() == good.post.tobytes() and len(good.maps) > 100
    gm.post_sw_setup(77, 0.2, 0.3, 0.01, 0.5, 0.02, 0.6)
    other = gm.post_sw(synth.pack_reads(reads[:1, 1:])[0], int(reads[0, 0]), "ACGT", "ACGT", 0)
    s.read_mappings_cs(reads, quals=quals, qual_delta=qd)
    assert gm.post_sw(synth.pack_reads(reads[:1, 1:])[0], int(reads[0, 0]), "ACGT", "ACGT", 0) == other

    def refused(call, code, word, session=s):
        with pytest.raises(gm.GmError) as e: call()
        assert "(%d)" % code in str(e.value) and word in str(e.value), str(e.value)
        if session is s:
            again = s.read_mappings_cs(reads, quals=quals, qual_delta=qd)
            assert again.maps.tobytes() == good.maps.tobytes() and again.cigar_buf == good.cigar_buf
    L = gm.lib(); cols = np.ascontiguousarray(reads[:, 1:]); ib = np.ascontiguousarray(reads[:, 0])
    packed = np.ascontiguousarray(synth.pack_reads(cols), dtype=np.uint32); rd = packed.ctypes.data_as(C.POINTER(C.c_uint32)); ibp = ib.ctypes.data_as(C.POINTER(C.c_uint8))
    res = gm.ReadMappingsCsResult(); n = len(reads); nc = cols.shape[1]
    call = lambda *a: gm._check(L.gm_read_mappings_cs(*a), "gm_read_mappings_cs")
    refused(lambda: call(s.h, n, nc, rd, ibp, None, 33, 0, None, None), GM_E_ARG, "bad arguments")
    refused(lambda: call(None, n, nc, rd, ibp, None, 33, 0, C.byref(res), None), GM_E_ARG, "bad arguments")
    refused(lambda: call(s.h, n, nc, None, ibp, None, 33, 0, C.byref(res), None), GM_E_ARG, "bad arguments")
    refused(lambda: call(s.h, n, nc, rd, None, None, 33, 0, C.byref(res), None), GM_E_ARG, "initbp")
    bad_ib = ib.copy(); bad_ib[3] = 4
    refused(lambda: s.read_mappings_cs(cols, initbp=bad_ib), GM_E_ARG, "primer letter")
    refused(lambda: s.read_mappings_cs(np.zeros((4, s.params.longest_read_len + 2), dtype=np.uint8)), GM_E_RANGE, "out of range")
    refused(lambda: call(s.h, n, nc, rd, ibp, b"\n".join(quals[:n - 1]), qd, 0, C.byref(res), None), GM_E_ARG, "QUAL string")
    refused(lambda: s.read_mappings_cs(reads, quals=[quals[0][:-1]] + quals[1:], qual_delta=qd), GM_E_ARG, "QUAL string")
    assert not res.hits and not res.maps and not res.post and res.n_hits == 0      # after a failure the struct holds nothing to free
    L.gm_read_mappings_cs_free(C.byref(res))
    # a crossover score whose doubled value does not fit 8 bits, with QVs: the mapping entry's code and message
    pc = gm.default_params_cs(); pc.crossover_score = -70
    good_plain = s.read_mappings_cs(reads)
    sx = gm.Session(ix, params=pc, max_batch_reads=1024)
    refused(lambda: sx.read_mappings_cs(reads, quals=quals, qual_delta=qd), GM_E_RANGE, "kept in 8 bits", session=sx)
    with pytest.raises(gm.GmError) as e: sx.map_reads_cs_fastq(reads, quals, qd)
    assert "(%d)" % GM_E_RANGE in str(e.value) and "kept in 8 bits" in str(e.value)
    assert len(sx.read_mappings_cs(reads).maps) > 100                    # the good call on that session: without QVs
    sx.close()
    # num_tmp_outputs = 65
    pk = gm.default_params_cs(); pk.num_tmp_outputs = 65
    s65 = gm.Session(ix, params=pk, max_batch_reads=1024)
    refused(lambda: s65.read_mappings_cs(reads), GM_E_RANGE, "num_tmp_outputs", session=s65)
    assert len(s65.read_windows(cols, initbp=ib)[0]) > 100              # (no call of the entry is good under such a session: it serves the front's seam)
    s65.close()
    # a read length beyond the full-alignment kernel's LDS
    pl = gm.default_params_cs(); pl.longest_read_len = 3000
    sl = gm.Session(ix, params=pl, max_batch_reads=256)
    refused(lambda: sl.read_mappings_cs(np.zeros((2, 2501), dtype=np.uint8)), GM_E_RANGE, "LDS", session=sl)
    assert sl.read_mappings_cs(reads).maps.tobytes() == good_plain.maps.tobytes()      # the good call on that session: reads of 50 colours
    sl.close()
    # (the table's last row, a read beyond one post_sw thread's column scratch -- 59 918 colours -- cannot be reached: the LDS tests refuse such a read first; the header says so)
    # a letter-space session is sent to gm_read_mappings; gm_read_mappings on the colour-space session is refused as before
    contigs, lreads, _ = oa.load_golden("cfg1_36bp_1Mbp")
    lix = gm.Index(contigs, params=gm.default_params()); ls = gm.Session(lix, params=gm.default_params(), max_batch_reads=1024)
    refused(lambda: ls.read_mappings_cs(np.ascontiguousarray(lreads[:50], dtype=np.uint8)), GM_E_ARG, "gm_read_mappings", session=ls)
    assert len(ls.read_mappings(np.ascontiguousarray(lreads[:200], dtype=np.uint8)).maps) > 100      # the good call on that session: the entry the message names
    ls.close(); lix.close()
    refused(lambda: s.read_mappings(cols), GM_E_ARG, "gm_sw_full_cs_batch_ix")
    # the mapping entry on the same session, then the call again
    want = trm.by_read(_fq()[4], len(F["reads"]))
    assert s.map_reads_cs_fastq(reads, quals, qd) == b"".join(want[:len(reads)])
    again = s.read_mappings_cs(reads, quals=quals, qual_delta=qd)
    assert again.maps.tobytes() == good.maps.tobytes() and again.recs.tobytes() == good.recs.tobytes()


@pytest.mark.gpu
def test_release_build_gives_the_same_answers():
    """the release build in a fresh child interpreter with GM_LIB_PATH on libgmapper_hip_release.so: the chain and the reference's bytes on two sets, one with QVs"""
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    close_all()
    sel = "(test_equal_to_the_chain_of_existing_entries or test_through_sam_records_to_the_bytes_of_the_reference) and (" + " or ".join("(%s)" % c.replace("@", " and ") for c in RELEASE_CASES) + ")"
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=dict(os.environ, GM_LIB_PATH=rel), cwd=oa.ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) >= 2 * len(RELEASE_CASES), p.stdout[-500:]
