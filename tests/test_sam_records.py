"""gm_sam_records (Session.sam_records): the SAM text of a chunk's mappings, made on the device from the arrays of the batch seams -- the last link of the chain
gm_read_windows -> ... -> gm_select_pass2 -> gm_sw_full_batch_text_ix -> gm_sam_records.

The rule set of the header (hit_output for an unpaired read, ref: gmapper/output.c:227-774) is restated here in Python (restate_records).  Without a GPU the restatement
is pinned to the REFERENCE by replay: every record of the reference's own outputs is parsed back into the seam's inputs (golden_inputs: clips, rmapped, insertions and
deletions from the CIGAR, genome_start from POS by the strand formula solved backwards, mismatches = NM - ins - del, a z whose truncated log is the printed integer,
qralign from XX:Z, post_quals from QUAL turned back), restated, and must give the golden's bytes.  On the GPU the library is held to the same replay, to the restatement
on hand-made shapes, and -- chained from reads -- to the reference outputs byte for byte."""
import gzip, math, os, re
import numpy as np
import pytest
from tests import oracle_api as oa
from shrimp_amd import gmapper as G

GM_E_ARG = -2
GOLD = os.path.join(oa.ROOT, "tests", "golden")
LETTERS = b"ACGTUMRWSYKVHDBN"
# reference output -> its inputs and the gm_params_t fields it was written under (oracle_api.OPTION_CASES / CS_OPTION_CASES / SAM_TAIL_CASES, tests/test_gpu_parity.py)
GOLDENS = {
    "cfg2s_100bp_2Mbp": dict(base="cfg2s_100bp_2Mbp"),
    "cfg2s_100bp_2Mbp@extra_fields": dict(base="cfg2s_100bp_2Mbp", fields=dict(extra_sam_fields=1)),
    "n1_noisy_70bp@extra_fields_rg_unal": dict(base="n1_noisy_70bp", fields=dict(extra_sam_fields=1, read_group=b"grp1", sam_unaligned=1)),
    "stress_100bp_unal@rg_unal": dict(base="stress_100bp_unal", fields=dict(read_group=b"grp1", sam_unaligned=1)),
    "stress_100bp_unal@local": dict(base="stress_100bp_unal", fields=dict(local_alignment=1, sam_unaligned=1)),
    "stress_60bp": dict(base="stress_60bp"),
    "stress_60bp@all_contigs": dict(base="stress_60bp", fields=dict(all_contigs=1)),
    "stress_100bp_unal@no_mapq": dict(base="stress_100bp_unal", fields=dict(no_mapping_qualities=1, sam_unaligned=1)),
    "stress_100bp_fq33": dict(base="stress_100bp_unal", fields=dict(sam_unaligned=1), fq="stress_100bp_fq33"),
    "stress_100bp_fq64": dict(base="stress_100bp_unal", fields=dict(sam_unaligned=1), fq="stress_100bp_fq64"),
    "cfg4s_50col_2Mbp@cs_extra_rg": dict(base="cfg4s_50col_2Mbp", colour=True, fields=dict(extra_sam_fields=1, read_group=b"grp1", sam_unaligned=1)),
    "cfg4s_50col_fq": dict(base="cfg4s_50col_2Mbp", colour=True, fields=dict(sam_unaligned=1), fq="cfg4s_50col_fq"),
    "cfg4s_50col_2Mbp@cs_local": dict(base="cfg4s_50col_2Mbp", colour=True, fields=dict(local_alignment=1)),
    "text_ls_unal": dict(base="stress_100bp_unal", fields=dict(sam_unaligned=1), text="text_ls_reads"),
    "text_cs_unal": dict(base="stress_cs_60col_unal", colour=True, fields=dict(sam_unaligned=1), text="text_cs_reads"),
}


def rules_of(colour, fields):
    """what the record text depends on of a gm_params_t"""
    f = fields or {}
    return dict(colour=bool(colour), mqv_on=not f.get("local_alignment") and not f.get("no_mapping_qualities"), all_contigs=bool(f.get("all_contigs")),
                extra=bool(f.get("extra_sam_fields")), read_group=f.get("read_group", b""), sam_unaligned=bool(f.get("sam_unaligned")))


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------------------------------------
def seq_from_text(c):                                                   # gmapper/output.c:326-351
    return ord("N") if c in b"RYSWKMBDHV" else (c - 32 if c >= ord("a") else c)


def rc_char(c): return {65: 84, 67: 71, 71: 67, 84: 65}.get(c, 78)      # A C G T, anything else N


def neglog(x): return int(1000.0 * -math.log(x))                        # double_to_neglog, util.h:297-301


def csfasta(I, r):
    if I["seqs"] is not None: return I["seqs"][r]
    return bytes([b"ACGT"[I["initbp"][r] & 3]]) + bytes(48 + c if c < 4 else 46 for c in I["codes"][r].tolist())


def tail(I, extra):
    R = I["rules"]; t = b""
    if R["read_group"]: t += b"\tRG:Z:" + R["read_group"]
    if extra is not None: t += b"\tZM:i:%d\tZR:i:%d\tZV:i:%d\tZH:i:%d\tZE:Z:%s" % extra
    return t + b"\n"


def restate_unaligned(I, r, name):
    R = I["rules"]; q = None if I["quals"] is None else I["quals"][r]
    out = name + b"\t4\t*\t0\t0\t*\t*\t0\t0\t"
    if R["colour"]: return out + b"*\t*\tCQ:Z:" + (q if q is not None else b"*") + b"\tCS:Z:" + csfasta(I, r) + tail(I, None)
    if I["seqs"] is not None: seq = bytes(seq_from_text(c) for c in I["seqs"][r])
    else: seq = bytes(LETTERS[c] for c in I["codes"][r].tolist())
    return out + seq + b"\t" + (q if q is not None else b"*") + tail(I, None)


def restate_mapped(I, r, name, m):
    R = I["rules"]; i = int(m["hit"]); h = I["hits"][i]; rec = I["recs"][i]; L = I["codes"].shape[1]
    rev = int(h["gen_st"]) == 1; cn = int(h["cn"])
    ins, dele, rmapped, rs = int(rec["insertions"]), int(rec["deletions"]), int(rec["rmapped"]), int(rec["read_start"])
    if not rev: pos = int(rec["genome_start"]) + 1
    else: pos = (int(I["contig_len"][cn]) - int(rec["genome_start"])) - (rmapped - 1 - dele + ins)      # output.c:626-634
    cbuf, coff = I["cigar"]
    out = [name, b"16" if rev else b"0", I["contig_names"][cn], b"%d" % (pos & 0xFFFFFFFF), b"%d" % int(m["mqv"]), cbuf[int(coff[i]):int(coff[i + 1])], b"*", b"0", b"0"]
    q = None if I["quals"] is None else I["quals"][r]
    mism, xov = int(rec["mismatches"]), int(rec["crossovers"])
    if R["colour"]:
        qr = I["qralign"][int(rec["ops_off"]):int(rec["ops_off"]) + int(rec["n_ops"])]
        up = lambda c: (c - 32 if c >= 97 else c)
        seq = [c if c in b"ACGTN" else 78 for c in (up(c) for c in qr if c != 45)]
        if rev: seq = [rc_char(c) for c in reversed(seq)]
        qual = b"*"
        if I["post"] is not None:
            mism, xov = int(I["post"][i]["mismatches"]), int(I["post"][i]["crossovers"])
            if q is not None and I["post_quals"] is not None and int(I["post"][i]["qual_len"]):
                o = int(I["post"][i]["qual_off"]); qual = I["post_quals"][o:o + int(I["post"][i]["qual_len"])]
                if rev: qual = qual[::-1]
        out += [bytes(seq), qual]
    else:
        codes = I["codes"][r].tolist()
        seq = [b"ACGT"[c] if c < 4 else 78 for c in codes]
        if I["seqs"] is not None:
            for k in range(L):
                if k < rs or k >= rs + rmapped: seq[k] = seq_from_text(I["seqs"][r][k])
        if rev: seq = [46 if c == 46 else rc_char(c) for c in reversed(seq)]
        if q is None: qual = b"*"
        else:
            qual = bytes((c + 33 - I["qual_delta"]) & 255 for c in q)
            if rev: qual = qual[::-1]
        out += [bytes(seq), qual]
    out.append(b"AS:i:%d" % int(m["score_full"]))
    if R["mqv_on"] and not R["all_contigs"]: out += [b"Z0:i:%d" % neglog(float(m["z0"])), b"Z1:i:%d" % neglog(float(m["z1"]))]
    out.append(b"NM:i:%d" % (mism + dele + ins))
    if R["colour"]:
        if q is not None: out.append(b"CQ:Z:" + q)
        out += [b"CS:Z:" + csfasta(I, r), b"CM:i:%d" % xov, b"XX:Z:" + qr]
    extra = None
    if R["extra"]:
        ebuf, eoff = I["edit"]
        zv = int(h["score_vector"]) if I["score_vector"] is None else int(I["score_vector"][i])
        extra = (int(h["matches"]), int(h["score_window_gen"]), zv, int(rec["score"]), ebuf[int(eoff[i]):int(eoff[i + 1])])
    return b"\t".join(out) + tail(I, extra)


def restate_records(I):
    """-> (the text, read_off): one record per mapping in maps order, the unaligned record for a read without any when sam_unaligned is set"""
    parts, off = [], [0]
    for r in range(I["codes"].shape[0]):
        name = I["names"][r] if I["names"] is not None else b"r%d" % r
        lo, hi = int(I["map_off"][r]), int(I["map_off"][r + 1])
        if lo == hi: text = restate_unaligned(I, r, name) if I["rules"]["sam_unaligned"] else b""
        else: text = b"".join(restate_mapped(I, r, name, I["maps"][k]) for k in range(lo, hi))
        parts.append(text); off.append(off[-1] + len(text))
    return b"".join(parts), np.array(off, dtype=np.uint64)


# ---- the reference's records, parsed back into the seam's inputs ----------------------------------------------------------------------------------------------
def offsets(slices):
    return b"".join(slices), np.concatenate([[0], np.cumsum([len(x) for x in slices])]).astype(np.uint64)


def zinv(z):
    """a double whose truncated log is the printed integer"""
    return math.exp(-(z + (0.5 if z >= 0 else -0.5)) / 1000.0)


def text_codes(lines, colour):
    def ls(c):
        k = LETTERS.find(bytes([c]).upper()); return k if k >= 0 else 15
    if not colour: return np.array([[ls(c) for c in t] for t in lines], dtype=np.uint8)
    return np.array([[b"ACGT".find(bytes([t[0]]).upper())] + [c - 48 if 48 <= c <= 51 else 15 for c in t[1:]] for t in lines], dtype=np.uint8)


_inputs = {}


def golden_inputs(golden):
    """-> (inputs, the golden's records as bytes, its per-read groups)"""
    if golden in _inputs: return _inputs[golden]
    spec = GOLDENS[golden]; colour = spec.get("colour", False); R = rules_of(colour, spec.get("fields"))
    contigs, reads, _ = oa.load_golden(spec["base"])
    with gzip.open(os.path.join(GOLD, golden + ".sam.gz"), "rb") as f: lines = [l for l in f.read().splitlines(keepends=True) if not l.startswith(b"@")]
    quals, delta, seqs = None, 33, None
    if "fq" in spec:
        z = np.load(os.path.join(GOLD, spec["fq"] + ".npz")); reads = reads[:int(z["n_reads"])]
        quals = [bytes(q.tobytes()) for q in z["quals"]]; delta = int(z["qual_delta"])
    if "text" in spec:
        with gzip.open(os.path.join(GOLD, spec["text"] + ".txt.gz"), "rb") as f: seqs = f.read().split(b"\n")[:-1]
        reads = text_codes(seqs, colour)
    reads = np.ascontiguousarray(reads, dtype=np.uint8); n = len(reads)
    initbp, codes = (reads[:, 0].copy(), np.ascontiguousarray(reads[:, 1:])) if colour else (None, reads)
    L = codes.shape[1]
    cnames = [b"contig%d" % (k + 1) for k in range(len(contigs))]; clen = np.array([len(c) for c in contigs], dtype=np.int64)
    groups = [b""] * n; per_read = [[] for _ in range(n)]
    for l in lines:
        t = l.rstrip(b"\n").split(b"\t"); r = int(t[0][1:]); groups[r] += l
        if int(t[1]) & 4: continue
        per_read[r].append(t)
    K = sum(len(x) for x in per_read)
    hits = np.zeros(K, dtype=G.PASS1_HIT_DTYPE); recs = np.zeros(K, dtype=G.SW_FULL_REC_DTYPE); maps = np.zeros(K, dtype=G.MAPPING_DTYPE)
    post = np.zeros(K, dtype=G.POST_REC_DTYPE) if colour and R["mqv_on"] else None
    cig, ed, qrs, pqs = [b""] * K, [b""] * K, [b""] * K, [b""] * K
    map_off = np.zeros(n + 1, dtype=np.uint64); k = 0
    for r in range(n):
        for t in per_read[r]:
            i = K - 1 - k                                                # (the hits in another order than the mappings)
            rev = bool(int(t[1]) & 16); cn = cnames.index(t[2]); tags = {x[:2]: x[5:] for x in t[11:]}
            runs = [(int(a), o) for a, o in re.findall(rb"(\d+)([MIDSH])", t[5])]
            assert b"".join(b"%d%s" % x for x in runs) == t[5]
            if rev: runs = runs[::-1]
            rs = runs[0][0] if runs[0][1] in b"SH" else 0
            nM = sum(a for a, o in runs if o == b"M"); dele = sum(a for a, o in runs if o == b"I"); ins = sum(a for a, o in runs if o == b"D")
            rmapped = nM + dele; pos = int(t[3])
            gs = pos - 1 if not rev else int(clen[cn]) - pos - (rmapped - 1 - dele + ins)
            h, rec, m = hits[i], recs[i], maps[k]
            h["read"], h["st"], h["gen_st"], h["cn"], h["score_max"] = r, int(rev), int(rev), cn, 10 * L
            rec["read_start"], rec["rmapped"], rec["gmapped"], rec["insertions"], rec["deletions"], rec["genome_start"] = rs, rmapped, rmapped - dele + ins, ins, dele, gs
            mism = int(tags[b"NM"]) - ins - dele
            rec["score"] = int(tags[b"ZH"]) if R["extra"] else 1
            if R["extra"]: h["matches"], h["score_window_gen"], h["score_vector"] = int(tags[b"ZM"]), int(tags[b"ZR"]), int(tags[b"ZV"]); ed[i] = tags[b"ZE"]
            m["read"], m["hit"], m["score_full"], m["mqv"] = r, i, int(tags[b"AS"]), int(t[4])
            if b"Z0" in tags: m["z0"], m["z1"] = zinv(int(tags[b"Z0"])), zinv(int(tags[b"Z1"]))
            assert (b"Z0" in tags) == (R["mqv_on"] and not R["all_contigs"])
            cig[i] = t[5]
            if colour:
                qrs[i] = tags[b"XX"]; rec["n_ops"] = len(qrs[i])
                if post is not None:
                    post[i]["mismatches"], post[i]["crossovers"] = mism, int(tags[b"CM"])
                    if t[10] != b"*": pqs[i] = t[10][::-1] if rev else t[10]
                else: rec["mismatches"], rec["crossovers"] = mism, int(tags[b"CM"])
            else: rec["mismatches"] = mism
            k += 1
        map_off[r + 1] = k
    qralign = None; post_quals = None
    if colour:
        qralign, qoff = offsets(qrs); recs["ops_off"] = qoff[:-1]
        if post is not None and quals is not None:
            post_quals, poff = offsets(pqs); post["qual_off"] = poff[:-1]; post["qual_len"] = np.diff(poff.astype(np.int64))
    I = dict(rules=R, codes=codes, initbp=initbp, names=None, seqs=seqs, quals=quals, qual_delta=delta, hits=hits, recs=recs, maps=maps, map_off=map_off,
             cigar=offsets(cig), edit=offsets(ed) if R["extra"] else None, qralign=qralign, post=post, post_quals=post_quals, score_vector=None,
             contig_names=cnames, contig_len=clen, spec=spec)
    _inputs[golden] = (I, b"".join(lines), groups)
    return _inputs[golden]


# ---- CPU --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("golden", sorted(GOLDENS))
def test_restated_records_are_the_bytes_of_the_reference(golden):
    """every record of the reference's output, parsed back into the seam's inputs and restated: the golden's bytes, all records, and the per-read groups"""
    I, want, groups = golden_inputs(golden)
    got, off = restate_records(I)
    assert len(want) > 10000 and got == want, first_diff(got, want)
    assert [got[int(off[r]):int(off[r + 1])] for r in range(len(groups))] == groups
    if I["rules"]["sam_unaligned"]: assert all(groups)


def first_diff(a, b):
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    lo = max(0, a.rfind(b"\n", 0, k) + 1)
    return (len(a), len(b), k, a[lo:k + 200], b[lo:k + 200])


def test_library_exports_the_entry_and_the_size_of_its_input():
    L = G.lib()
    assert hasattr(L, "gm_sam_records") and hasattr(L, "gm_sam_input_size")
    assert {"gm_sam_records", "gm_sam_input_size"} <= set(G.EXPORTS)
    import ctypes as C
    assert L.gm_sam_input_size() == C.sizeof(G.SAM_INPUT)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gm():
    try:
        import torch
        torch.cuda.init()
    except Exception:
        pass
    if G.lib().gm_device_count() < 1:
        pytest.fail("no HIP device: the product path has no CPU fallback")
    return G


def params_of(gm, colour, fields):
    p = gm.default_params_cs() if colour else gm.default_params()
    for k, v in (fields or {}).items(): setattr(p, k, v)
    return p


_ix = {}


def index_of(gm, base, colour):
    if base not in _ix:
        contigs, _, _ = oa.load_golden(base)
        _ix[base] = gm.Index(contigs, params=params_of(gm, colour, None))
    return _ix[base]


def device_records(s, I):
    return s.sam_records(I["codes"], I["hits"], I["recs"], I["maps"], I["map_off"], I["cigar"], initbp=I["initbp"], names=I["names"], seqs=I["seqs"], quals=I["quals"],
                         qual_delta=I["qual_delta"], score_vector=I["score_vector"], post=I["post"], post_quals=I["post_quals"], qralign=I["qralign"], edit=I["edit"])


def session_of(gm, golden):
    spec = GOLDENS[golden]; colour = spec.get("colour", False)
    return gm.Session(index_of(gm, spec["base"], colour), params=params_of(gm, colour, spec.get("fields")), max_batch_reads=8192)


@pytest.mark.gpu
@pytest.mark.parametrize("golden", sorted(GOLDENS))
def test_replay_on_the_device_gives_the_bytes_of_the_reference(gm, golden):
    I, want, groups = golden_inputs(golden)
    s = session_of(gm, golden)
    got, off = device_records(s, I)
    s.close()
    assert got == want, first_diff(got, want)
    assert [got[int(off[r]):int(off[r + 1])] for r in range(len(groups))] == groups


# ---- the chain to bytes -------------------------------------------------------------------------------------------------------------------------------------------
def chain_cases():
    from tests import test_select as ts
    cases = dict(ts.CHAINS)
    cases["stress_60bp@single_best"] = dict(single_best_mapping=1)
    cases["stress_60bp@max3_o5"] = dict(max_alignments=3, num_outputs=5)
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("golden", ["cfg2s_100bp_2Mbp@extra_fields", "cfg4s_50col_2Mbp@cs_extra_rg", "n1_noisy_70bp@extra_fields_rg_unal", "stress_60bp", "stress_60bp@max3_o5",
                                    "stress_60bp@single_best"])
def test_chain_from_reads_to_the_bytes_of_the_reference(gm, golden):
    """the chain of tests/test_select.py (its helpers, its fixtures) with gm_sam_records at its end: read by read the reference's bytes, for every read but those that
    own a group of equal windows (tie_mask: at most 33 on stress_60bp, none elsewhere); then the mapping entry on the same session"""
    from tests import test_select as ts
    fields = chain_cases()[golden]
    name, _, tag = golden.partition("@")
    ix, s, p, reads = ts.opened(gm, name, fields)
    colour = bool(p.colour_space)
    c = ts.library_pass1(gm, name, fields)
    hits, hit_off, rlen = c["hits"], c["hit_off"], c["rlen"]; n = len(hits)
    ts.full_setup(gm, p)
    thresh = np.array([int(ts.abs_or_pct(p.sw_full_threshold, sm)) for sm in hits["score_max"]], dtype=np.int32)
    anchors = [(int(h["ax"]), int(h["ay"]), int(h["alen"]), int(h["awidth"])) for h in hits]
    rw = c["rw"][hits["read"]]; lens = np.full(n, rlen)
    cn, gst, goff, wl = hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"]
    revcmpl = (hits["gen_st"] == 1).astype(np.uint8) if p.tiebreak_rev else None
    post = None; qbuf = None; ib = None
    if colour:
        ib = reads[hits["read"], 0]
        recs, ops, strings = ix.sw_full_cs_batch(cn, gst, goff, wl, rw, lens, ib, anchors, revcmpl=revcmpl, threshscore=thresh)
        ts.post_setup(gm, p)
        post, qralign, _ = ix.post_sw_batch(cn, gst, recs, ops, rw, lens, ib)
        qbuf = qralign.buffer; sv = hits["score_vector"]
    else:
        ts.vector_setup(gm, p)
        sv = ix.sw_vector_batch(cn, gst, goff, wl, rw, lens)
        recs, ops, strings = ix.sw_full_ls_batch(cn, gst, goff, wl, rw, lens, anchors=anchors, revcmpl=revcmpl, threshscore=thresh, maxscore=sv)
        recs = recs.copy(); recs["score"][sv < thresh] = 0
    maps, map_off = s.select_pass2(hits, hit_off, recs, post)
    flagged = sorted(set(maps["read"][(maps["flags"] & 1) != 0].tolist()))
    if flagged:                                                          # the header's recipe for the rounding guard (gm_select_pass2)
        strings.prefetch(); post = post.copy(); qb = bytearray(qbuf)
        for r in flagged:
            for i in range(int(hit_off[r]), int(hit_off[r + 1])):
                if recs[i]["score"] <= 0 or post[i]["by_host"]: continue
                db, qr = strings(i)
                one = gm.post_sw(rw[i], int(ib[i]), db, qr, int(recs[i]["read_start"]))
                post[i]["posterior"] = one["posterior"]; post[i]["by_host"] = 1
                qb[int(recs[i]["ops_off"]):int(recs[i]["ops_off"]) + int(recs[i]["n_ops"])] = one["qralign"].encode()
        qbuf = bytes(qb)
        maps, map_off = s.select_pass2(hits, hit_off, recs, post)
    status, _, _, cigar, edit = ix.sw_full_batch_text(cn, gst, recs, ops, rw, lens, initbp=ib, qralign=qbuf, reverse=(hits["gen_st"] == 1).astype(np.uint8),
                                                      clip="H" if colour else "S", what=("cigar", "edit"), colour_space=colour)
    assert (status == 0).all()
    kw = dict(initbp=reads[:, 0], post=post, qralign=qbuf) if colour else dict(score_vector=sv)
    got, off = s.sam_records(reads[:, 1:] if colour else reads, hits, recs, maps, map_off, cigar, edit=edit if p.extra_sam_fields else None, **kw)
    contigs, _, sam = oa.load_golden(name)
    if tag: sam = oa.load_option_sam(name, tag)
    want = [b""] * len(reads)
    for l in sam.splitlines(keepends=True):
        if not l.startswith(b"@"): want[int(l.split(b"\t", 1)[0][1:])] += l
    skip = set(c["rows"][ts.tie_mask(c["rows"])][:, 0].tolist())        # reads that own a group of equal windows (stress_60bp only)
    assert len(skip) <= (33 if name == "stress_60bp" else 0)
    mine = [got[int(off[r]):int(off[r + 1])] for r in range(len(reads))]
    bad = [r for r in range(len(reads)) if r not in skip and mine[r] != want[r]]
    assert not bad, (len(bad), [(mine[r], want[r]) for r in bad[:3]])
    assert sum(1 for r in range(len(reads)) if r not in skip and want[r]) > 1000
    assert {r for r in range(len(reads)) if mine[r]} - skip == {r for r in range(len(reads)) if want[r]} - skip
    # ... and the mapping entry on the same session afterwards: the same bytes for those reads, the reference's for all
    out = s.map_reads_cs(reads) if colour else s.map_reads(reads)
    assert oa.sam_header(contigs) + out == sam
    entry = [b""] * len(reads)
    for l in out.splitlines(keepends=True): entry[int(l.split(b"\t", 1)[0][1:])] += l
    assert all(mine[r] == entry[r] for r in range(len(reads)) if r not in skip)


# ---- hand-made shapes ---------------------------------------------------------------------------------------------------------------------------------------------
NAME_LENS = (1, 63, 64, 65, 255)
SLICE_LENS = (1, 64, 65, 4000)
INTS = (0, 7, 42, 512, 9999, 12345, 654321, 7654321, 87654321, 987654321, 2147483647, -1, -2147483648)      # every digit count 1 .. 10, and the sign
STARTS = (0, 8, 98, 998, 9998, 99998, 999998, 9999998, 99999998, 999999998, 2999999999, 4294967294)         # POS of 1 .. 10 digits, above 2^31, and the wrap
MISMATCHES = tuple(min(v, 2147483640) for v in INTS[:11])                # (NM adds the gaps to it in 32 bits)
MQVS = (0, 4, 255, 37)
_tiny = {}


def tiny(gm, colour):
    """a small index whose contig names are 1 and 200 bytes long"""
    if colour not in _tiny:
        from shrimp_amd import synth
        contigs = synth.make_genome([5000, 3000], seed=5)
        _tiny[colour] = (gm.Index(contigs, names=[b"c", b"N" * 200], params=params_of(gm, colour, None)), [b"c", b"N" * 200], np.array([5000, 3000], dtype=np.int64))
    return _tiny[colour]


def qr_pattern(rmapped, gaps, k):
    """a qralign of `rmapped` read positions with '-' at the columns of `gaps`: upper and lower case, N, and letters post_sw never writes"""
    alphabet = b"ACGTacgtNnAXx"; out = bytearray(); left = rmapped; col = 0
    while left > 0 or (gaps and col <= max(gaps) and col < 400):
        if col in gaps or left == 0: out.append(45)
        else: out.append(alphabet[(col * 7 + k) % len(alphabet)]); left -= 1
        col += 1
    return bytes(out)


QR_GAPS = [set(), {63}, {64}, {62, 63, 64, 65}, set(range(64, 128)), {0, 1, 127, 128}, set(range(0, 64)) | {130}]


def hand_made(rules, L, colour, cnames, clen, maps_per_read, seed, quals, seqs, names=True, post=True):
    """reads with maps_per_read[r] mappings each; every printed integer, slice length and strand is walked through"""
    rng = np.random.default_rng(seed); n = len(maps_per_read); K = sum(maps_per_read)
    codes = rng.integers(0, 4, (n, L)).astype(np.uint8); codes[rng.random((n, L)) < 0.1] = 15; codes[rng.random((n, L)) < 0.05] = 5
    initbp = rng.integers(0, 4, n).astype(np.uint8) if colour else None
    nm = [bytes(rng.integers(97, 123, NAME_LENS[r % 5]).astype(np.uint8)) for r in range(n)] if names else None
    qv = [bytes(rng.integers(66, 105, L).astype(np.uint8)) for _ in range(n)] if quals else None      # (offset 64: printable once re-based)
    if not seqs: sq = None
    elif colour: sq = [bytes([b"ACGTacgt"[rng.integers(0, 8)]]) + bytes(rng.choice(np.frombuffer(b"0123.4N", dtype=np.uint8), L)) for _ in range(n)]
    else: sq = [bytes(rng.choice(np.frombuffer(b"ACGTacgtNnXx.URYKMSWBDHVu", dtype=np.uint8), L)) for _ in range(n)]
    hits = np.zeros(K, dtype=G.PASS1_HIT_DTYPE); recs = np.zeros(K, dtype=G.SW_FULL_REC_DTYPE); maps = np.zeros(K, dtype=G.MAPPING_DTYPE)
    pst = np.zeros(K, dtype=G.POST_REC_DTYPE) if colour and post else None
    cig, ed, qrs, pqs = [], [], [], []
    sv = np.zeros(K, dtype=np.int32)
    map_off = np.zeros(n + 1, dtype=np.uint64); k = 0
    for r in range(n):
        for _ in range(maps_per_read[r]):
            h, rec, m = hits[k], recs[k], maps[k]
            rs = (k * 3) % L; rm = max(1, L - rs - (k % 3 if L - rs > 3 else 0))
            h["read"], h["cn"], h["gen_st"], h["st"], h["score_max"] = r, k % 2, (k // 2) % 2, (k // 2) % 2, 1000
            h["matches"], h["score_window_gen"], h["score_vector"] = INTS[k % 13], INTS[(k + 1) % 13], INTS[(k + 2) % 13]
            sv[k] = INTS[(k + 3) % 13]
            rec["score"], rec["read_start"], rec["rmapped"], rec["insertions"], rec["deletions"] = max(1, abs(INTS[(k + 4) % 13]) % 2147483647), rs, rm, k % 4, (k // 4) % 3
            rec["mismatches"], rec["crossovers"], rec["genome_start"] = MISMATCHES[(k + 5) % 11], INTS[(k + 6) % 11], STARTS[k % 12]
            m["read"], m["hit"], m["score_full"], m["mqv"] = r, k, INTS[(k + 7) % 13], MQVS[k % 4]
            m["z0"], m["z1"] = (0.5, 1.5) if k % 5 == 0 else (math.exp(-(INTS[k % 11] % 700000) / 1000.0 - 1e-4), math.exp(-(INTS[(k + 1) % 11] % 700000) / 1000.0 - 1e-4))
            cig.append((b"12M3I4D" * 600)[:SLICE_LENS[k % 4]]); ed.append((b"7xA(CG)-9" * 500)[:SLICE_LENS[(k + 1) % 4]])
            if colour:
                q = qr_pattern(rm, QR_GAPS[k % len(QR_GAPS)], k); qrs.append(b"#" * (k % 3) + q); rec["n_ops"] = len(q)      # (bytes between the slices belong to nobody)
                if pst is not None:
                    pst[k]["mismatches"], pst[k]["crossovers"] = MISMATCHES[(k + 8) % 11], INTS[(k + 9) % 11]
                    pqs.append(b"!" * (k % 2) + bytes(rng.integers(33, 127, rm if k % 7 else 0).astype(np.uint8))); pst[k]["qual_len"] = len(pqs[-1]) - k % 2
            k += 1
        map_off[r + 1] = k
    qralign = None; post_quals = None
    if colour:
        qralign, qoff = offsets(qrs); recs["ops_off"] = qoff[:-1] + np.arange(K, dtype=np.uint64) % 3
        if pst is not None: post_quals, poff = offsets(pqs); pst["qual_off"] = poff[:-1] + np.arange(K, dtype=np.uint64) % 2
    return dict(rules=rules, codes=codes, initbp=initbp, names=nm, seqs=sq, quals=qv, qual_delta=64 if quals else 33, hits=hits, recs=recs, maps=maps, map_off=map_off,
                cigar=offsets(cig), edit=offsets(ed) if rules["extra"] else None, qralign=qralign, post=pst, post_quals=post_quals, score_vector=sv,
                contig_names=cnames, contig_len=clen)


# reads with 0, 1 and 64 mappings in one call; unaligned reads first, last and adjacent
MAPS_PER_READ = [0, 1, 0, 0, 64, 2, 1, 3, 0]


def check_shape(gm, s, I):
    got, off = device_records(s, I)
    want, want_off = restate_records(I)
    assert got == want, first_diff(got, want)
    assert np.array_equal(off, want_off)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [False, True])
def test_hand_made_shapes_equal_the_restatement(gm, colour):
    ix, cnames, clen = tiny(gm, colour)
    variants = [dict(extra_sam_fields=1, read_group=b"g", sam_unaligned=1), dict(read_group=b"G" * 63, sam_unaligned=0), dict(extra_sam_fields=1, all_contigs=1, sam_unaligned=1),
                dict(local_alignment=1, sam_unaligned=1)]
    seen = set()
    for L in (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000):
        for v, fields in enumerate(variants):
            if v >= 2 and L not in (9, 65, 129): continue
            s = gm.Session(ix, params=params_of(gm, colour, fields), max_batch_reads=1024)
            R = rules_of(colour, fields)
            for quals in (False, True):
                I = hand_made(R, L, colour, cnames, clen, MAPS_PER_READ, seed=L * 8 + v * 2 + quals, quals=quals, seqs=quals, names=not (quals and v == 1),
                              post=R["mqv_on"])
                text = check_shape(gm, s, I)
                assert text.count(b"\n") == sum(m if m else R["sam_unaligned"] for m in MAPS_PER_READ)
                seen |= {len(x) for x in re.findall(rb"-?\d+", text)}
                if R["mqv_on"] and not R["all_contigs"]: assert b"\tZ1:i:-405\t" in text      # posteriors summing above 1
            s.close()
    assert set(range(1, 11)) <= seen


@pytest.mark.gpu
def test_hand_made_shapes_where_nothing_maps(gm):
    """no mapping at all: only unaligned records, or no text"""
    ix, cnames, clen = tiny(gm, False)
    for unal in (1, 0):
        fields = dict(sam_unaligned=unal, read_group=b"rg")
        s = gm.Session(ix, params=params_of(gm, False, fields), max_batch_reads=1024)
        I = hand_made(rules_of(False, fields), 33, False, cnames, clen, [0, 0, 0], seed=3, quals=True, seqs=True)
        got = check_shape(gm, s, I)
        assert (got.count(b"\n") == 3) == bool(unal) and (got == b"") == (not unal)
        e, eo = s.sam_records(I["codes"][:0], I["hits"], I["recs"], I["maps"], np.zeros(1, dtype=np.uint64), I["cigar"])
        assert e == b"" and eo.tolist() == [0]
        s.close()


# ---- order and reuse ------------------------------------------------------------------------------------------------------------------------------------------------
def times3(I):
    """the inputs three times over, end to end"""
    n = I["codes"].shape[0]; K = len(I["hits"]); J = dict(I)
    rep = lambda x: None if x is None else x * 3
    J["codes"] = np.concatenate([I["codes"]] * 3); J["initbp"] = None if I["initbp"] is None else np.concatenate([I["initbp"]] * 3)
    J["names"], J["seqs"], J["quals"] = rep(I["names"]), rep(I["seqs"]), rep(I["quals"])
    hits = np.concatenate([I["hits"]] * 3); recs = np.concatenate([I["recs"]] * 3); maps = np.concatenate([I["maps"]] * 3)
    for t in range(3):
        hits["read"][t * K:(t + 1) * K] += t * n; maps["read"][t * len(I["maps"]):(t + 1) * len(I["maps"])] += t * n; maps["hit"][t * len(I["maps"]):(t + 1) * len(I["maps"])] += t * K
        if I["qralign"] is not None: recs["ops_off"][t * K:(t + 1) * K] += t * len(I["qralign"])
    J["hits"], J["recs"], J["maps"] = hits, recs, maps
    J["map_off"] = np.concatenate([[0]] + [I["map_off"][1:].astype(np.int64) + t * len(I["maps"]) for t in range(3)]).astype(np.uint64)
    def text3(x):
        if x is None: return None
        buf, off = x
        return buf * 3, np.concatenate([[0]] + [off[1:].astype(np.int64) + t * len(buf) for t in range(3)]).astype(np.uint64)
    J["cigar"], J["edit"] = text3(I["cigar"]), text3(I["edit"])
    J["qralign"] = rep(I["qralign"])
    if I["post"] is not None:
        post = np.concatenate([I["post"]] * 3)
        if I["post_quals"] is not None:
            for t in range(3): post["qual_off"][t * K:(t + 1) * K] += t * len(I["post_quals"])
        J["post"] = post
    J["post_quals"] = rep(I["post_quals"])
    J["score_vector"] = None if I["score_vector"] is None else np.concatenate([I["score_vector"]] * 3)
    return J


@pytest.mark.gpu
@pytest.mark.parametrize("golden", ["stress_60bp", "cfg4s_50col_fq"])
def test_order_and_reuse(gm, golden):
    I, want, groups = golden_inputs(golden)
    s = session_of(gm, golden)
    one, off = device_records(s, I)
    again, off2 = device_records(s, I)
    assert one == want and again == one and np.array_equal(off, off2)
    # one call over three times the reads equals three calls (the names apart: r<index> counts on)
    I3 = times3(I); n = I["codes"].shape[0]
    I3["names"] = [b"r%d" % (r % n) for r in range(3 * n)]
    three, off3 = device_records(s, I3)
    assert three == one * 3 and np.array_equal(off3.astype(np.int64), np.concatenate([[0]] + [off[1:].astype(np.int64) + t * len(one) for t in range(3)]))
    # another order of a read's mappings is honoured
    J = dict(I); maps = I["maps"].copy(); rng = np.random.default_rng(1); moved = 0
    for r in range(n):
        lo, hi = int(I["map_off"][r]), int(I["map_off"][r + 1])
        if hi - lo > 1: maps[lo:hi] = maps[lo:hi][::-1]; moved += 1
    J["maps"] = maps
    assert moved > (50 if golden == "stress_60bp" else -1)
    got, offj = device_records(s, J)
    want_j, want_off = restate_records(J)
    assert got == want_j and (got != one) == (moved > 0) and np.array_equal(offj, want_off) and np.array_equal(offj, off)
    # the mapping entry on the same session still prints the golden
    spec = GOLDENS[golden]; contigs, reads, sam = oa.load_golden(spec["base"])
    if spec.get("colour"):
        reads = reads[:n]
        out = s.map_reads_cs_fastq(reads, I["quals"], I["qual_delta"])
    else: out = s.map_reads(reads)
    assert out == want
    assert device_records(s, I)[0] == one
    s.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("colour", [False, True])
def test_every_refusal_is_followed_by_a_good_call(gm, colour):
    ix, cnames, clen = tiny(gm, colour)
    fields = dict(extra_sam_fields=1, read_group=b"g", sam_unaligned=1)
    s = gm.Session(ix, params=params_of(gm, colour, fields), max_batch_reads=1024)
    I = hand_made(rules_of(colour, fields), 65, colour, cnames, clen, [2, 0, 3, 1], seed=9, quals=True, seqs=True)
    good = check_shape(gm, s, I)
    def refused(word, **change):
        J = dict(I); J.update(change)
        with pytest.raises(gm.GmError) as e: device_records(s, J)
        assert "(%d)" % GM_E_ARG in str(e.value) and word in str(e.value), str(e.value)
        assert device_records(s, I)[0] == good                           # the session is usable after every refusal
    def with_field(arr, k, field, value):
        a = I[arr].copy(); a[field][k] = value
        return {arr: a}
    def with_off(key, k, value):
        buf, off = I[key]; o = off.copy(); o[k] = value
        return {key: (buf, o)}
    bad = I["map_off"].copy(); bad[1], bad[2] = I["map_off"][2] + 1, I["map_off"][1]
    refused("ascending", map_off=bad)
    first = I["map_off"].copy(); first[0] = 1
    refused("map_off runs", map_off=first)
    last = I["map_off"].copy(); last[-1] -= 1
    refused("map_off runs", map_off=last)
    refused("says read", **with_field("maps", 0, "read", 2))
    refused("hit 6 of 6", **with_field("maps", 1, "hit", 6))
    refused("hit -1 of 6", **with_field("maps", 1, "hit", -1))
    refused("contig 2 of 2", **with_field("hits", 2, "cn", 2))
    refused("contig -1 of 2", **with_field("hits", 2, "cn", -1))
    refused("strand 2", **with_field("hits", 3, "gen_st", 2))
    refused("no alignment", **with_field("recs", 4, "status", GM_E_ARG))
    refused("no alignment", **with_field("recs", 5, "score", 0))
    refused("cigar slice", **with_off("cigar", 3, int(I["cigar"][1][-1]) + 1))
    refused("cigar slice", **with_off("cigar", 6, int(I["cigar"][1][5]) - 1))
    refused("edit slice", **with_off("edit", 2, int(I["edit"][1][-1]) + 5))
    refused("edit is missing", edit=None)
    refused("names: 3 lines", names=I["names"][:3])
    refused("seqs: 3 lines", seqs=I["seqs"][:3])
    refused("quals: 2 lines", quals=I["quals"][:2])
    refused("seqs: line 1", seqs=[I["seqs"][0], I["seqs"][1][:-1]] + I["seqs"][2:])
    refused("quals: line 3", quals=I["quals"][:3] + [I["quals"][3] + b"I"])
    if colour:
        refused("qralign slice lies outside", **with_field("recs", 5, "ops_off", len(I["qralign"])))
        refused("qralign slice lies outside", **with_field("recs", 0, "n_ops", len(I["qralign"]) + 1))
        refused("post_quals slice", **with_field("post", 1, "qual_off", len(I["post_quals"])))
        refused("read positions", **with_field("recs", 1, "rmapped", int(I["recs"]["rmapped"][1]) - 1))
        refused("read positions", **with_field("recs", 1, "read_start", 65))
        refused("qralign is missing", qralign=None)
        refused("needs initbp", initbp=None)
    else:
        refused("initbp belongs", initbp=np.zeros(4, dtype=np.uint8))
    s.close()
    # --shrimp-format: no SAM records to make
    fmt = gm.Session(ix, params=params_of(gm, colour, dict(output_format=1)), max_batch_reads=1024)
    with pytest.raises(gm.GmError) as e: device_records(fmt, I)
    assert "(%d)" % GM_E_ARG in str(e.value) and "SHRiMP format" in str(e.value)
    fmt.close()
    s = gm.Session(ix, params=params_of(gm, colour, fields), max_batch_reads=1024)
    assert device_records(s, I)[0] == good
    s.close()
