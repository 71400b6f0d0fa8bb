"""gm_sw_full_batch_text / gm_sw_full_batch_text_ix: dbalign / qralign, CIGAR and edit string of every record of one gm_sw_full_*_batch call, made on the device.

The yardstick is a Python restatement of the reference's three rules (make_cigar + reverse_cigar, ref: gmapper/output.c:15-80; alignment_edit_string, ref:
common/output.c:60-121; reverse_alignment_edit_string, ref: gmapper/output.c:83-122), pinned without a GPU to the reference's own SAM output committed under
tests/golden/.  The GPU tests compare the library with gm_sw_full_batch_strings / the fixtures' strings and with the restatement applied to them."""
import ctypes as C
import gzip, os, re, subprocess, sys, threading
import numpy as np
import pytest
from tests import oracle_api as oa
from tests.test_sw_full_batch import LS_SETUP, CS_SETUP, items_F, items_local, items_cs, pack, run_ls, run_cs
from tests import test_post_sw_batch as tp
from tests import test_seam_batch_ix as tx

GM_E_ARG = -2
NEW_SYMBOLS = ["gm_sw_full_batch_text", "gm_sw_full_batch_text_ix"]


# ---- the restatement (written from the reference's text) -------------------------------------------------------------------------------------------------------
def edit_string(db, qr):
    """alignment_edit_string"""
    assert len(db) == len(qr)
    out, consec, refgap, n = [], 0, False, len(db)
    for i in range(n + 1):
        if i != n and db[i] == qr[i] and db[i] != "-":
            consec += 1; continue
        if refgap and (consec != 0 or (db[i] if i < n else "\0") != "-"):
            out.append(")"); refgap = False
        if consec != 0:
            out.append("%d" % consec); consec = 0
        if i == n: break
        if db[i] == "-":
            if qr[i].islower(): out.append("x")
            if not refgap: out.append("(")
            out.append(qr[i].upper()); refgap = True
            continue
        if qr[i] == "-": out.append("-")
        elif db[i] == qr[i].upper(): out.append("x"); consec += 1
        elif qr[i].islower(): out.append("x"); out.append(qr[i].upper())
        else: out.append(qr[i])
    return "".join(out)


def reverse_edit(e):
    """reverse_alignment_edit_string; a character the reference asserts on passes through"""
    n, res, i = len(e), [""] * len(e), 0
    swap = {")": "(", "(": ")", "A": "T", "C": "G", "G": "C", "T": "A"}
    while i < n:
        if e[n - 1 - i].isdigit():
            j = i + 1
            while j < n and e[n - 1 - j].isdigit(): j += 1
            j -= 1
            res[i:j + 1] = e[n - 1 - j:n - i]
            i = j + 1
        else:
            res[i] = swap.get(e[n - 1 - i], e[n - 1 - i]); i += 1
    return "".join(res)


def cigar(db, qr, read_start, rlen, clip="S", reverse=False):
    """make_cigar (read_start 0-based here: the clipped positions in front), then reverse_cigar"""
    runs = []
    if read_start > 0: runs.append((read_start, clip))
    i, n = 0, len(qr)
    while i < n:
        if qr[i] == "-": op, same = "D", lambda k: qr[k] == "-"
        elif db[i] == "-": op, same = "I", lambda k: db[k] == "-"
        else: op, same = "M", lambda k: db[k] != "-" and qr[k] != "-"
        ln = 0
        while i + ln < n and same(i + ln): ln += 1
        runs.append((ln, op)); i += ln
    read_end = read_start + sum(c != "-" for c in qr)
    if read_end != rlen: runs.append((rlen - read_end, clip))
    if reverse: runs.reverse()
    return "".join("%d%s" % r for r in runs)


_memo = {}


def expected(db, qr, read_start, rlen, clip, rev):
    key = (db, qr, read_start, rlen, clip, rev)
    if key not in _memo:
        e = edit_string(db, qr)
        _memo[key] = (cigar(db, qr, read_start, rlen, clip, rev).encode(), (reverse_edit(e) if rev else e).encode())
    return _memo[key]


# ---- 1: the restatement against the reference's SAM output (no GPU) ----------------------------------------------------------------------------------------------
LETTERS = "ACGTUMRWSYKVHDBN"
RC = {"A": "T", "C": "G", "G": "C", "T": "A", "-": "-", "N": "N"}


def sam_records(tag_file):
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", tag_file), "rt") as f:
        for line in f:
            if line.startswith("@"): continue
            t = line.rstrip("\n").split("\t")
            if int(t[1]) & 4: continue
            yield dict(flag=int(t[1]), cn=int(t[2][len("contig"):]) - 1, pos=int(t[3]) - 1, cigar=t[5], seq=t[9], tags={x[:2]: x[5:] for x in t[11:]})


def walk(rec, contig, read_letters):
    """field 6 walked over the contig (and SEQ, letter space) -> (dbalign, qralign or None, leading clip, trailing clip), all in the genome's forward orientation"""
    runs = [(int(a), b) for a, b in re.findall(r"(\d+)([MIDSH])", rec["cigar"])]
    assert "".join("%d%s" % r for r in runs) == rec["cigar"]
    lead = runs[0][0] if runs[0][1] in "SH" else 0
    tail = runs[-1][0] if len(runs) > 1 and runs[-1][1] in "SH" else 0
    db, qr, g, r = [], [], rec["pos"], lead
    for ln, op in runs:
        if op in "SH": continue
        for _ in range(ln):
            if op == "M": db.append(LETTERS[contig[g]]); g += 1; qr.append(read_letters[r] if read_letters else "?"); r += 1
            elif op == "D": db.append(LETTERS[contig[g]]); g += 1; qr.append("-")
            else: db.append("-"); qr.append(read_letters[r] if read_letters else "?"); r += 1
    if read_letters: assert r + tail == len(read_letters)
    return "".join(db), "".join(qr) if read_letters else None, lead, tail


def check_cigar_rule(rec, db, qr, lead, tail):
    """field 6 from the strings and clip lengths: as printed (forward orientation), and for a reverse record also from the read's orientation with reverse = True"""
    rl = lead + tail + sum(c != "-" for c in qr)
    assert cigar(db, qr, lead, rl, "S", False) == rec["cigar"], rec
    if rec["flag"] & 16: assert cigar(db[::-1], qr[::-1], tail, rl, "S", True) == rec["cigar"], rec


def test_restatement_reproduces_the_reference_letter_space():
    """every mapped record of cfg2s_100bp_2Mbp@extra_fields: ZE:Z and field 6; and field 6 of every record of @local_cfg2 (soft clips)"""
    contigs, _, _ = oa.load_golden("cfg2s_100bp_2Mbp")
    n = n_rev = n_gap = 0
    for rec in sam_records("cfg2s_100bp_2Mbp@extra_fields.sam.gz"):
        db, qr, lead, tail = walk(rec, contigs[rec["cn"]], rec["seq"])
        assert edit_string(db, qr) == rec["tags"]["ZE"], (rec, db, qr)
        check_cigar_rule(rec, db, qr, lead, tail)
        n += 1; n_rev += bool(rec["flag"] & 16); n_gap += "-" in db or "-" in qr
    assert (n, n_rev, n_gap) == (5000, 2507, 1527)
    n = n_clip = 0
    for rec in sam_records("cfg2s_100bp_2Mbp@local_cfg2.sam.gz"):
        db, qr, lead, tail = walk(rec, contigs[rec["cn"]], rec["seq"])
        check_cigar_rule(rec, db, qr, lead, tail)
        n += 1; n_clip += lead > 0 or tail > 0
    assert n >= 4000 and n_clip >= 100, (n, n_clip)


def test_restatement_reproduces_the_reference_colour_space():
    """every mapped record of cfg4s_50col_2Mbp@cs_extra_rg: XX:Z is qralign in the read's orientation; forward: edit_string(db, XX) == ZE:Z; reverse: db turned onto
    the read's strand, then reverse_edit(edit_string(db_rc, XX)) == ZE:Z; field 6 from those strings"""
    contigs, _, _ = oa.load_golden("cfg4s_50col_2Mbp")
    n = n_fwd = n_x = 0
    for rec in sam_records("cfg4s_50col_2Mbp@cs_extra_rg.sam.gz"):
        db, _, lead, tail = walk(rec, contigs[rec["cn"]], None)
        xx = rec["tags"]["XX"]
        if rec["flag"] & 16:
            db_rc = "".join(RC[c] for c in reversed(db))
            assert len(db_rc) == len(xx) and reverse_edit(edit_string(db_rc, xx)) == rec["tags"]["ZE"], (rec, db_rc)
            rl = lead + tail + sum(c != "-" for c in xx)
            assert cigar(db_rc, xx, tail, rl, "S", True) == rec["cigar"], rec
            assert cigar(db, xx[::-1], lead, rl, "S", False) == rec["cigar"], rec
        else:
            assert len(db) == len(xx) and edit_string(db, xx) == rec["tags"]["ZE"], (rec, db)
            check_cigar_rule(rec, db, xx, lead, tail)
            n_fwd += 1
        n += 1; n_x += "x" in rec["tags"]["ZE"]
    assert (n, n_fwd, n - n_fwd, n_x) == (2942, 1437, 1505, 2539)


def test_reverse_edit_on_hand_made_strings():
    assert reverse_edit("46-33(T)1A18") == "18T1(A)33-46" and reverse_edit("") == "" and reverse_edit("x(AC)12xG") == "Cx12(GT)x" and reverse_edit("5N3") == "3N5"
    assert edit_string("ACGT", "ACGT") == "4" and edit_string("A-CG", "AtCG") == "1x(T)2" and edit_string("ACG", "AcG") == "1x2" and edit_string("AC--", "ACGT") == "2(GT)"
    assert cigar("AC-GT", "A-TGT", 2, 8, "H", False) == "2H1M1D1I2M2H" and cigar("AC-GT", "A-TGT", 2, 8, "S", True) == "2S2M1I1D1M2S" and cigar("", "", 0, 0) == ""


# ---- 2: symbols and refusals (no GPU) ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_listed():
    from shrimp_amd import gmapper
    L = gmapper.lib()
    with open(os.path.join(oa.ROOT, "include", "gmapper_hip.h")) as f: header = f.read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in gmapper.EXPORTS and re.search(r"\bint %s\(" % s, header), s
    for name, v in (("GM_TEXT_ALIGN", 1), ("GM_TEXT_CIGAR", 2), ("GM_TEXT_EDIT", 4)): assert re.search(r"#define %s\s+%d\b" % (name, v), header), name
    assert callable(gmapper.sw_full_batch_text) and callable(gmapper.Index.sw_full_batch_text)


def _raw(L, ix_form, what, n=1, ix=None):
    rec = np.zeros(1, dtype=np.dtype([("x", np.uint8, 64)])); z = np.zeros(2, dtype=np.uint32); one = np.ones(1, dtype=np.int32); st = np.zeros(1, dtype=np.int32)
    u = z.ctypes.data_as(C.POINTER(C.c_uint32)); ip = one.ctypes.data_as(C.POINTER(C.c_int)); u8 = np.zeros(1, dtype=np.uint8)
    p = [C.c_void_p(0x1234) for _ in range(4)]; off = np.full(2, 99, dtype=np.uint64); o64 = off.ctypes.data_as(C.POINTER(C.c_uint64))
    tail = [u, 1, ip, None, 0, None, None, ord("S"), st.ctypes.data_as(C.POINTER(C.c_int)), C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), o64, C.byref(p[3]), o64]
    if ix_form: rc = L.gm_sw_full_batch_text_ix(ix, 0, what, n, ip, u8.ctypes.data_as(C.POINTER(C.c_uint8)), rec.ctypes.data, None, 0, *tail)
    else: rc = L.gm_sw_full_batch_text(0, what, n, rec.ctypes.data, None, 0, u, 2, *tail)
    return rc, [x.value for x in p], list(off)


def test_refusals_without_a_device():
    from shrimp_amd import gmapper
    L = gmapper.lib()
    out = {}
    def fresh():                                            # a new thread: no setup state is needed, and none is looked at
        out["null"] = (_raw(L, True, 7)[0], L.gm_last_error())
        out["what0"] = (_raw(L, False, 0)[0], L.gm_last_error())
        out["what8"] = _raw(L, False, 8)[0]
        out["what0_n0"] = _raw(L, False, 0, n=0)[0]
        out["n0"] = _raw(L, False, 7, n=0)
        out["one"] = _raw(L, False, 7)                      # a record without alignment (score 0): answered on the host, empty slices
    t = threading.Thread(target=fresh); t.start(); t.join()
    assert out["null"][0] == GM_E_ARG and b"ix is NULL" in out["null"][1]
    assert out["what0"][0] == GM_E_ARG and b"what" in out["what0"][1] and out["what8"] == GM_E_ARG and out["what0_n0"] == GM_E_ARG
    assert out["n0"] == (0, [0x1234] * 4, [99, 99])         # n = 0: GM_OK, nothing written
    rc, ptrs, off = out["one"]
    assert rc == 0 and off == [0, 0] and all(p not in (None, 0x1234) for p in ptrs)
    for p in ptrs: L.gm_free(C.c_void_p(p))
    assert [L.gm_abi_sizeof(k) for k in range(6)] == [280, 40, 200, 72, 64, 40] and L.gm_abi_sizeof(6) == -1


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------------------------------
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
    for v in tx._idx.values(): v.close()
    tx._idx.clear()


SETS = {"F": (False, False, False), "local": (False, True, False), "cs_S": (True, False, False), "cs_L": (True, True, False), "cs_X": (True, False, False),
        "cs_Y": (True, True, False), "rna_S": (True, False, True), "rna_L": (True, True, True)}      # name -> (colour, local, rna)
_sets = {}


def fixture_items(name):
    return {"F": items_F, "local": items_local, "cs_S": lambda: items_cs("sw_kat_cs.txt.gz", "S"), "cs_L": lambda: items_cs("sw_kat_cs_local.txt.gz", "L"),
            "cs_X": lambda: items_cs("sw_kat_cs_xover.txt.gz", "X"), "cs_Y": lambda: items_cs("sw_kat_cs_xover.txt.gz", "Y"),
            "rna_S": lambda: items_cs("sw_kat_cs_rna.txt.gz", "S"), "rna_L": lambda: items_cs("sw_kat_cs_rna.txt.gz", "L")}[name]()


def known(gm, name):
    """a fixture set through its batch SW call, once per module: dict(items, recs, ops, p, want = the fixture's own (dbalign, qralign) per item)"""
    if name not in _sets:
        colour, local, rna = SETS[name]
        items = fixture_items(name)
        if colour: gm.sw_full_cs_setup(*CS_SETUP); recs, ops, strings, bases = run_cs(gm, items, local=local, is_rna=rna)
        else: gm.sw_full_ls_setup(*LS_SETUP); recs, ops, strings, bases = run_ls(gm, items, local=local)
        want = [(it["db"], it["qr"]) if it["want"][0] > 0 else ("", "") for it in items]
        for k in range(0, len(items), 97): assert tuple(x or "" for x in strings(k)) == want[k], (name, k)      # (the SW tests hold every item; here a sample ties the two)
        _sets[name] = dict(items=items, recs=recs, ops=ops, p=pack(items), want=want, colour=colour, rna=rna)
    return _sets[name]


def check_text(got, recs, rlen, want, rev, clip, what=7, only=None):
    """status 0 and the four slices of every item (only: those) against the wanted strings and the restatement on them"""
    status, db, qr, cg, ed = got
    for k in (range(len(recs)) if only is None else only):
        assert status[k] == 0, (k, status[k])
        wdb, wqr = want[k]
        if what & 1: assert (db(k), qr(k)) == (wdb.encode(), wqr.encode()), (k, db(k), qr(k), wdb, wqr)
        if recs[k]["score"] <= 0:
            assert (what & 2 == 0 or cg(k) == b"") and (what & 4 == 0 or ed(k) == b""), k; continue
        wc, we = expected(wdb, wqr, int(recs[k]["read_start"]), int(rlen[k]), clip, bool(rev))
        if what & 2: assert cg(k) == wc, (k, cg(k), wc, wdb, wqr)
        if what & 4: assert ed(k) == we, (k, ed(k), we, wdb, wqr)


def text_of(gm, S, rev=None, clip="S", what=("align", "cigar", "edit"), **kw):
    p = S["p"]
    return gm.sw_full_batch_text(S["colour"], kw.get("recs", S["recs"]), kw.get("ops", S["ops"]), p["genome"], kw.get("reads", p["reads"]), kw.get("rlen", p["rlen"]),
                                 initbp=kw.get("initbp", p["initbp"]) if S["colour"] else None, is_rna=S["rna"], reverse=rev, clip=clip, what=what)


# ---- 3: known answers ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,at_least", [("F", 2990), ("local", 2260), ("cs_S", 1400), ("cs_L", 800), ("cs_X", 1000), ("cs_Y", 500), ("rna_S", 600), ("rna_L", 600)])
def test_known_answers(gm, name, at_least):
    """one call a set, what = 7: every dbalign / qralign slice is the fixture's, every CIGAR and edit string the restatement's; reverse none / all, clip S / H"""
    S = known(gm, name)
    n = len(S["items"]); assert n >= at_least and sum(r["score"] > 0 for r in S["recs"]) >= 0.8 * n
    for rev in (None, np.ones(n, dtype=np.uint8)):
        for clip in "SH":
            got = text_of(gm, S, rev=rev, clip=clip)
            check_text(got, S["recs"], S["p"]["rlen"], S["want"], rev is not None, clip)
            assert got[3].offsets[0] == 0 and len(got[3].offsets) == n + 1 and len(got[4].offsets) == n + 1
    if S["rna"]: assert any("U" in w[0] for w in S["want"])


# ---- 4: with post_sw ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("use_qvs", [False, True])
def test_with_post_sw(gm, use_qvs):
    """the 1 222 + 611 posterior records: gm_sw_full_cs_batch, gm_post_sw_batch, then the text with qralign_in = qralign_out -- the qralign slice is the re-called one,
    CIGAR and edit string the restatement on (dbalign, re-called qralign)"""
    K, P = tp.fixture()
    sel = [w for w in P if w["useq"] == int(use_qvs)]
    assert len(sel) == (611 if use_qvs else 1222)
    tp.setup(gm, use_qvs=use_qvs)
    res = tp.chain(gm, [tp.s_items()[w["idx"]] for w in sel], quals=[w["qin"].encode() for w in sel] if use_qvs else None)
    recs, ops, p = res["recs"], res["ops"], res["p"]
    buf = bytearray(ops.size); want = []
    for k, w in enumerate(sel):
        q = res["qralign"](k); assert q == w["qralign"]
        buf[int(recs[k]["ops_off"]):int(recs[k]["ops_off"]) + int(recs[k]["n_ops"])] = q.encode()
        want.append((res["strings"](k)[0], q))
    assert any(want[k][1] != res["strings"](k)[1] for k in range(len(sel)))                   # post_sw did re-call letters
    for rev in (None, np.ones(len(sel), dtype=np.uint8)):
        got = gm.sw_full_batch_text(True, recs, ops, p["genome"], p["reads"], p["rlen"], initbp=p["initbp"], qralign=bytes(buf), reverse=rev)
        check_text(got, recs, p["rlen"], want, rev is not None, "S")
        got = gm.sw_full_batch_text(True, recs, ops, p["genome"], None, p["rlen"], qralign=bytes(buf), reverse=rev, what=("edit",))      # (the reads are not read then)
        check_text(got, recs, p["rlen"], want, rev is not None, "S", what=4)
    bad = bytearray(buf); k = next(k for k in range(len(sel)) if "-" in want[k][1]); bad[int(recs[k]["ops_off"]) + want[k][1].index("-")] = ord("A")
    got = gm.sw_full_batch_text(True, recs, ops, p["genome"], p["reads"], p["rlen"], initbp=p["initbp"], qralign=bytes(bad))
    assert got[0][k] == GM_E_ARG and got[3](k) == b"" and (np.delete(got[0], k) == 0).all()      # a slice whose gaps are not the operations'


# ---- 5: the index form -----------------------------------------------------------------------------------------------------------------------------------------------
def _ix_legs(gm, S, key, colour_index, strands=(0, 1), is_rna=-1):
    """the set's records made on the index (strand 0; strand 1 of the index of the reverse complements), then text_ix == the fixture's strings + the restatement,
    and byte for byte the host-bitfield entry on the contigs of that strand"""
    items = S["items"]
    for st in strands:
        its = items if st == 0 else [it for it in items if tx.no_u(it["g"])]
        assert len(its) >= 0.9 * len(items)
        ix = tx.indexes(gm, (key, st > 0, colour_index), [it["g"] for it in its], colour=colour_index)
        a = tx.arrays(its); sts = np.full(len(its), st, dtype=np.uint8)
        if S["colour"]:
            gm.sw_full_cs_setup(*CS_SETUP)
            recs, ops, _ = ix[st].sw_full_cs_batch(ix[3], sts, ix[4] + a["goff"], a["glen"], a["reads"], a["rlen"], a["initbp"], a["anchors"], a["rv"], a["thresh"], xover=a["xs"], is_rna=is_rna)
        else:
            gm.sw_full_ls_setup(*LS_SETUP)
            recs, ops, _ = ix[st].sw_full_ls_batch(ix[3], sts, ix[4] + a["goff"], a["glen"], a["reads"], a["rlen"], a["anchors"], a["rv"], a["thresh"], a["maxscore"])
        want = [(it["db"], it["qr"]) if it["want"][0] > 0 else ("", "") for it in its]
        ib = a["initbp"] if S["colour"] else None
        rev = (np.arange(len(its)) % 2).astype(np.uint8)
        got = ix[st].sw_full_batch_text(ix[3], sts, recs, ops, a["reads"], a["rlen"], initbp=ib, is_rna=is_rna, reverse=rev, colour_space=S["colour"])
        for r in (0, 1): check_text(got, recs, a["rlen"], want, r, "S", only=range(r, len(its), 2))
        gw, wbase = tx.host_contigs(ix[2])                    # ix[2]: the contigs of strand 0 of the first index == strand 1 of the second
        r2 = recs.copy(); r2["genome_start"] += wbase[ix[3]] * 8
        host = gm.sw_full_batch_text(S["colour"], r2, ops, gw, a["reads"], a["rlen"], initbp=ib, is_rna=bool(S["rna"]), reverse=rev)
        assert np.array_equal(got[0], host[0])
        for f, h in zip(got[1:], host[1:]): assert f.buffer == h.buffer and (f.offsets is None or np.array_equal(f.offsets, h.offsets))


@pytest.mark.gpu
@pytest.mark.parametrize("name,colour_index,strands,rna", [("F", False, (0, 1), -1), ("cs_S", False, (0, 1), -1), ("cs_S", True, (0, 1), -1), ("rna_S", False, (0,), 1)])
def test_index_form(gm, name, colour_index, strands, rna):
    S = dict(known(gm, name)) if name in _sets else dict(items=fixture_items(name), colour=SETS[name][0], rna=SETS[name][2])
    _ix_legs(gm, S, "text_" + name, colour_index, strands=strands, is_rna=rna)


@pytest.mark.gpu
def test_index_form_strand_1_of_an_rna_contig_and_refusals(gm):
    """hand-made records on both strands of every contig of a seven-contig genome (an RNA contig, every code): strand 1 of the RNA contig shows U for A.  The host
    entry on the numpy statement of that strand gives the same bytes.  A contig or strand that does not exist and a record past the contig are refused alone."""
    contigs = tx.genome7(); lens = [len(c) for c in contigs]
    rng = np.random.default_rng(11)
    rows = [(c, st) for c in (0, 3, 6) for st in (0, 1) for _ in range(6)]
    n = len(rows); nops = 90; rlen = np.full(n, 100, dtype=np.int32)
    cn = np.array([r[0] for r in rows], dtype=np.int32); st = np.array([r[1] for r in rows], dtype=np.uint8)
    recs = np.zeros(n, dtype=gm.SW_FULL_REC_DTYPE); ops = []
    for i in range(n):
        o = rng.choice(np.frombuffer(b"MMMMMMMID", dtype=np.uint8), size=nops); o[0] = o[-1] = ord("M")
        recs[i]["score"] = 1; recs[i]["ops_off"] = len(ops); recs[i]["n_ops"] = nops; recs[i]["read_start"] = 3
        recs[i]["genome_start"] = int(rng.integers(0, lens[cn[i]] - 100)) if i % 3 else lens[cn[i]] - int((o != ord("D")).sum())      # (every third ends at the contig's last base)
        ops += list(o)
    ops = np.array(ops, dtype=np.uint8)
    reads = np.stack([tx.pack(rng.integers(0, 16, size=104, dtype=np.uint8)) for _ in range(n)])
    ix = gm.Index(contigs)
    got = ix.sw_full_batch_text(cn, st, recs, ops, reads, rlen)
    assert (got[0] == 0).all()
    for s in (0, 1):
        words = [tx.pack(tx.strand_contig(c, s)[0]) for c in contigs]; wbase = np.concatenate([[0], np.cumsum([len(w) for w in words])[:-1]])
        m = st == s; r2 = recs[m].copy(); r2["genome_start"] += wbase[cn[m]] * 8
        host = gm.sw_full_batch_text(False, r2, ops, np.concatenate(words), reads[m], rlen[m])
        for j, k in enumerate(np.nonzero(m)[0]):
            assert (got[1](k), got[2](k), got[3](k), got[4](k)) == (host[1](j), host[2](j), host[3](j), host[4](j)), (s, k)
            db, qr = gm.sw_full_batch_strings(False, r2[j], ops, np.concatenate(words), reads[k], rlen=100)
            assert got[1](k) == db.encode() and got[4](k) == edit_string(db, qr).encode()
    assert any(b"U" in got[1](k) for k in range(n) if cn[k] == 3 and st[k] == 1)
    c2 = cn.copy(); s2 = st.copy(); r3 = recs.copy(); c2[2] = len(contigs); s2[5] = 2; r3[7]["genome_start"] = lens[cn[7]] - 10
    bad = ix.sw_full_batch_text(c2, s2, r3, ops, reads, rlen)
    assert list(np.nonzero(bad[0])[0]) == [2, 5, 7] and (bad[0][[2, 5, 7]] == GM_E_ARG).all() and bad[3](2) == b"" and b"item 7 refused" in gm.lib().gm_last_error()
    for k in set(range(n)) - {2, 5, 7}: assert (bad[1](k), bad[3](k), bad[4](k)) == (got[1](k), got[3](k), got[4](k)), k
    ix.close()


# ---- 6: the shapes where the wave kernel can go wrong (hand-made records) -------------------------------------------------------------------------------------------
class Hand:
    """hand-made records in the public encoding.  An alignment is a list of columns: ("m" | "x" | "I" | "D", lower).  m: the read letter is the genome's; x: another
    one; I: a genome letter against a gap in the read; D: a read letter against a gap in the genome; lower: the colour-space crossover mark (bit 7)."""
    def __init__(self, gm, colour, seed):
        self.gm, self.colour, self.rng = gm, colour, np.random.default_rng(seed)
        self.genome, self.reads, self.rlen, self.initbp, self.recs, self.ops = [], [], [], [], [], []

    def add(self, cols, lead=0, tail=0, initbp=None, read_codes=None, genome_codes=None):
        rng = self.rng; cols = [(c, False) if isinstance(c, str) else c for c in cols]
        n_g = sum(c != "D" for c, _ in cols); n_r = sum(c != "I" for c, _ in cols)
        G = rng.integers(0, 4, size=n_g, dtype=np.uint8) if genome_codes is None else np.asarray(genome_codes, dtype=np.uint8)
        want, gi = [], 0                                        # the letters the read shows in its columns
        for c, _ in cols:
            if c == "m": want.append(int(G[gi]) if G[gi] < 4 else 0)
            elif c == "x": want.append((int(G[gi]) + 1 + int(rng.integers(0, 3))) % 4 if G[gi] < 4 else 1)
            elif c == "D": want.append(int(rng.integers(0, 4)))
            gi += c != "D"
        ib = int(rng.integers(0, 4)) if initbp is None else initbp
        ops = []
        if not self.colour:
            body = np.array(want, dtype=np.uint8) if read_codes is None else np.asarray(read_codes, dtype=np.uint8)
            read = np.concatenate([rng.integers(0, 4, size=lead, dtype=np.uint8), body, rng.integers(0, 4, size=tail, dtype=np.uint8)])
            ops = [ord("M") if c in "mx" else ord(c) for c, _ in cols]
        else:
            # colours such that translation layer `lay` of the column's read position is the wanted letter: X(j) = want ^ ((lay + initbp) & 3), colour(j) = X(j) ^ X(j - 1)
            lays = rng.integers(0, 4, size=n_r); head = rng.integers(0, 4, size=lead)
            x_prev = 0
            for c in head: x_prev ^= int(c)
            body, j = [], 0
            for c, low in cols:
                if c == "I": ops.append(1 | (0x80 if low else 0)); continue
                x = want[j] ^ ((int(lays[j]) + ib) & 3); body.append(x ^ x_prev); x_prev = x
                ops.append(((2 if c == "D" else 6) + int(lays[j])) | (0x80 if low else 0)); j += 1
            read = np.concatenate([head, np.array(body, dtype=np.int64), rng.integers(0, 4, size=tail)]).astype(np.uint8) if read_codes is None else np.asarray(read_codes, dtype=np.uint8)
        rec = np.zeros(1, dtype=self.gm.SW_FULL_REC_DTYPE)
        pad = int(rng.integers(1, 9))
        rec["score"] = 1; rec["read_start"] = lead; rec["genome_start"] = sum(len(g) for g in self.genome) + pad; rec["n_ops"] = len(ops); rec["ops_off"] = len(self.ops)
        self.genome.append(np.concatenate([rng.integers(0, 16, size=pad, dtype=np.uint8), G])); self.ops += ops
        self.reads.append(read); self.rlen.append(len(read)); self.initbp.append(ib); self.recs.append(rec[0])

    def arrays(self):
        rw = max((len(r) + 7) // 8 for r in self.reads) + 1
        reads = np.zeros((len(self.reads), rw), dtype=np.uint32)
        for i, r in enumerate(self.reads): w = tx.pack(r); reads[i, :len(w)] = w
        return dict(genome=tx.pack(np.concatenate(self.genome + [np.zeros(8, dtype=np.uint8)])), reads=reads, rlen=np.array(self.rlen, dtype=np.int32),
                    initbp=np.array(self.initbp, dtype=np.uint8), recs=np.array(self.recs, dtype=self.gm.SW_FULL_REC_DTYPE), ops=np.array(self.ops, dtype=np.uint8))


def _fix_cs_random(gm, rng):
    """the colour-space items with colours of every code, built directly (Hand.add sizes the genome from the columns)"""
    H = Hand(gm, True, 77)
    for _ in range(6):
        kinds = rng.choice(["m"] * 12 + ["x", "x", "I", "D"], size=130); kinds[0] = kinds[-1] = "m"
        cols = [(str(k), bool(rng.random() < 0.15)) for k in kinds]
        n_g = sum(k != "D" for k, _ in cols); n_r = sum(k != "I" for k, _ in cols)
        c = rng.integers(0, 4, size=7 + n_r + 13).astype(np.uint8); c[rng.integers(0, len(c), size=6)] = rng.integers(4, 16, size=6); c[rng.integers(0, len(c), size=4)] = 15
        g = np.where(rng.random(n_g) < 0.1, rng.integers(4, 16, size=n_g), rng.integers(0, 4, size=n_g)).astype(np.uint8)
        H.add(cols, lead=7, tail=13, read_codes=c, genome_codes=g)
    H.add(["m"] * 70, read_codes=np.array([15] * 70, dtype=np.uint8))
    return H


def shapes(gm, colour):
    """the hand-made set of one space: (arrays, wanted strings from gm_sw_full_batch_strings)"""
    key = ("shapes", colour)
    if key not in _sets:
        H = Hand(gm, colour, 5 if colour else 6); rng = np.random.default_rng(9)
        def rnd(n):                                             # a random alignment of n columns that begins and ends in a pair
            kinds = rng.choice(["m"] * 12 + ["x", "x", "I", "D"], size=n); kinds[0] = kinds[-1] = "m"
            return [(str(k), bool(colour and rng.random() < 0.15)) for k in kinds]
        for n in (1, 63, 64, 65, 127, 128, 129, 1400):
            H.add(rnd(n)); H.add(rnd(n), lead=int(rng.integers(1, 12)), tail=int(rng.integers(1, 12)))
        for L in (9, 10, 99, 100, 999, 1000):                   # digit counts, in the edit string and (the whole alignment one run) in the CIGAR
            H.add(["x"] + ["m"] * L + ["x"]); H.add(["m"] * L, lead=L, tail=L)
        H.add(["x"] * 60 + ["m"] * 11 + ["x"] * 3)              # a match run from column 60 to column 70
        H.add(["m"] * 62 + ["D"] * 5 + ["m"] * 10)              # an insertion group over columns 62-66
        H.add(["m"] * 20 + ["D"] * 3)                           # ... one that ends the alignment
        H.add(["m"] * 63 + ["D"]); H.add(["m"] * 64 + ["D"] * 64 + ["m"]); H.add(["D"] * 2 + ["m"] * 62 + ["D"] * 2 + ["m"] * 62 + ["D"] * 2)
        H.add(["m"] * 60 + ["I"] * 8 + ["m"] * 10)              # a deletion run across column 64
        H.add(["I"] * 3 + ["m"] * 61 + ["I"] * 64 + ["m"] * 3 + ["I"])
        H.add(["m"] * 5 + ["D", "I", "D", "I"] + ["m"] * 5)     # groups one column apart
        for lead, tail in ((0, 0), (7, 0), (0, 9), (7, 9), (123, 1), (1, 1234)): H.add(["m"] * 30 + ["x"] + ["m"] * 30, lead=lead, tail=tail)
        if colour:
            for at in (10, 62, 63, 64):                         # x immediately before ( -- a lower-case letter opens the group --, a crossover on a matching letter in front of a group
                H.add(["m"] * at + [("D", True), ("D", False), ("D", True)] + ["m"] * 5)
                H.add(["m"] * at + [("m", True), ("D", False)] + ["m"] * 5)
                H.add(["m"] * at + [("m", True)] + ["m"] * 70 + [("x", True), ("I", True), ("m", True)])      # x at column 63 / 64, a count that starts at it and crosses a step
            for ib in range(4): H.add(rnd(40), lead=3, initbp=ib)
            R = _fix_cs_random(gm, rng)                         # colours of every code: 15 (the translations start again), 4-14 (N from there to the next 15); genome letters of every code
            base = sum(len(g) for g in H.genome)
            for k in range(len(R.recs)):
                rec = R.recs[k].copy(); rec["genome_start"] += base; rec["ops_off"] += len(H.ops); H.recs.append(rec)
            H.genome += R.genome; H.ops += R.ops; H.reads += R.reads; H.rlen += R.rlen; H.initbp += R.initbp
        else:
            H.add(["m"] * 256, read_codes=np.tile(np.arange(16), 16), genome_codes=np.repeat(np.arange(16), 16))      # every genome code against every read code
        a = H.arrays()
        want = [gm.sw_full_batch_strings(colour, a["recs"][k], a["ops"], a["genome"], a["reads"][k], int(a["initbp"][k]), False, rlen=int(a["rlen"][k])) for k in range(len(a["recs"]))]
        _sets[key] = (a, want)
    return _sets[key]


@pytest.mark.gpu
@pytest.mark.parametrize("colour", [False, True])
def test_wave_shapes(gm, colour):
    """alignments of 1 ... 1 400 columns, runs of 9 ... 1 000, runs, groups and crossovers at the 64-column step boundary, clips at either end, every letter and colour
    code, every primer: strings, CIGAR and edit string against gm_sw_full_batch_strings and the restatement, forward and reversed, alone (n = 1) and in one call"""
    a, want = shapes(gm, colour)
    n = len(a["recs"])
    lens = sorted({len(w[0]) for w in want}); assert {1, 63, 64, 65, 127, 128, 129, 1400} <= set(lens)
    eds = [edit_string(*w) for w in want]
    assert all(any(re.search(r"(?<!\d)%d(?!\d)" % L, e) for e in eds) for L in (9, 10, 99, 100, 999, 1000))
    if colour: assert any("x(" in e for e in eds) and any("N" in w[1] or "n" in w[1] for w in want)
    else: assert {c for w in want for c in w[0]} >= set(LETTERS) and {c for w in want for c in w[1]} >= set(LETTERS)
    for rev in (None, np.ones(n, dtype=np.uint8)):
        for clip in "SH":
            got = gm.sw_full_batch_text(colour, a["recs"], a["ops"], a["genome"], a["reads"], a["rlen"], initbp=a["initbp"] if colour else None, reverse=rev, clip=clip)
            check_text(got, a["recs"], a["rlen"], want, rev is not None, clip)
    for k in (0, 15, n - 1):                                    # n = 1
        got = gm.sw_full_batch_text(colour, a["recs"][k:k + 1], a["ops"], a["genome"], a["reads"][k:k + 1], a["rlen"][k:k + 1], initbp=a["initbp"][k:k + 1] if colour else None)
        check_text(got, a["recs"][k:k + 1], a["rlen"][k:k + 1], want[k:k + 1], False, "S")


# ---- 7: layout ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_layout_of_a_shuffled_call(gm):
    """the F records three times over in a shuffled order (8 970 items; ops_off not monotonic, slices shared, three junk bytes in front of every slice): the offsets are
    non-decreasing, tight and n + 1 long, every slice is right, dbalign is 0 between the slices, and what = 2 / what = 4 alone give the bytes of what = 7"""
    S = known(gm, "F"); recs, p = S["recs"], S["p"]
    ops2, off2 = [], np.zeros(len(recs), dtype=np.uint64)
    for k in range(len(recs)):
        ops2 += [0x58] * 3; off2[k] = len(ops2); ops2 += list(S["ops"][int(recs[k]["ops_off"]):int(recs[k]["ops_off"]) + int(recs[k]["n_ops"])])
    ops2 = np.array(ops2, dtype=np.uint8); r1 = recs.copy(); r1["ops_off"] = off2
    order = np.random.default_rng(20261018).permutation(np.tile(np.arange(len(recs)), 3))
    assert order.size == 8970
    r2 = r1[order]; want = [S["want"][k] for k in order]; rlen = p["rlen"][order]
    assert (np.diff(r2["ops_off"].astype(np.int64)) < 0).any()
    rev = (np.arange(order.size) % 3 == 0).astype(np.uint8)
    got = gm.sw_full_batch_text(False, r2, ops2, p["genome"], p["reads"][order], rlen, reverse=rev, clip="H")
    for r in (0, 1): check_text(got, r2, rlen, want, r, "H", only=np.nonzero(rev == r)[0])
    covered = np.zeros(ops2.size, dtype=bool)
    for k in range(len(r1)): covered[int(r1[k]["ops_off"]):int(r1[k]["ops_off"]) + (int(r1[k]["n_ops"]) if r1[k]["score"] > 0 else 0)] = True
    for f in got[1:3]:
        b = np.frombuffer(f.buffer, dtype=np.uint8); assert b.size == ops2.size and not b[~covered].any() and b[covered].all()
    for f in got[3:]:
        off = f.offsets.astype(np.int64); assert off.size == order.size + 1 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(f.buffer)
    only_c = gm.sw_full_batch_text(False, r2, ops2, p["genome"], p["reads"][order], rlen, reverse=rev, clip="H", what=("cigar",))
    only_e = gm.sw_full_batch_text(False, r2, ops2, p["genome"], p["reads"][order], rlen, reverse=rev, clip="H", what="edit")
    assert only_c[1] is None and only_c[4] is None and only_c[3].buffer == got[3].buffer and np.array_equal(only_c[3].offsets, got[3].offsets)
    assert only_e[2] is None and only_e[3] is None and only_e[4].buffer == got[4].buffer and np.array_equal(only_e[4].offsets, got[4].offsets)
    only_a = gm.sw_full_batch_text(False, r2, ops2, p["genome"], p["reads"][order], rlen, what=("align",))
    assert only_a[3] is None and only_a[1].buffer == got[1].buffer and only_a[2].buffer == got[2].buffer


# ---- 8: refusals beside answers -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_beside_answers(gm):
    S = known(gm, "cs_S")
    sel = [k for k in range(len(S["recs"])) if S["recs"][k]["score"] > 0][:60]
    p = S["p"]; recs = S["recs"][sel].copy(); ops = S["ops"].copy(); rlen = p["rlen"][sel].copy(); initbp = p["initbp"][sel].astype(np.uint8).copy(); want = [S["want"][k] for k in sel]
    cols = lambda k, f: sum(1 for b in ops[int(recs[k]["ops_off"]):int(recs[k]["ops_off"]) + int(recs[k]["n_ops"])] if f(b & 15))
    recs[3]["ops_off"] = ops.size - int(recs[3]["n_ops"]) + 1                                   # its operations pass ops_len by one byte
    recs[9]["genome_start"] = p["genome"].size * 8 - cols(9, lambda t: not 2 <= t <= 5) + 1     # the alignment runs past the genome by one position
    rlen[14] = int(recs[14]["read_start"]) + cols(14, lambda t: t != 1) - 1                     # ... past the read
    ops[int(recs[17]["ops_off"]) + 2] = 0x0b                                                    # no operation of the encoding
    initbp[22] = 4
    recs[31]["status"] = -4; recs[31]["score"] = 0
    recs[40]["score"] = 0
    bad = {3: GM_E_ARG, 9: GM_E_ARG, 14: GM_E_ARG, 17: GM_E_ARG, 22: GM_E_ARG, 31: -4, 40: 0}
    got = gm.sw_full_batch_text(True, recs, ops, p["genome"], p["reads"][sel], rlen, initbp=initbp, clip="S")
    msg = gm.lib().gm_last_error()
    assert b"item 22 refused" in msg and b"initbp" in msg, msg                                   # the last refused item's reason
    for k, st in bad.items():
        assert got[0][k] == st and got[1](k) == got[2](k) == got[3](k) == got[4](k) == b"" and got[3].offsets[k] == got[3].offsets[k + 1], (k, got[0][k])
    good = [k for k in range(len(sel)) if k not in bad]
    check_text(got, recs, rlen, want, False, "S", only=good)
    db = np.frombuffer(got[1].buffer, dtype=np.uint8)
    for k in (9, 14, 22, 40): assert not db[int(recs[k]["ops_off"]):int(recs[k]["ops_off"]) + int(recs[k]["n_ops"])].any(), k      # nothing was written for them
    with pytest.raises(gm.GmError): gm.sw_full_batch_text(True, recs, ops, p["genome"], p["reads"][sel], rlen, initbp=initbp, clip="X")
    with pytest.raises(gm.GmError): gm.sw_full_batch_text(True, recs, ops, p["genome"], None, rlen, initbp=initbp)          # the reads are required without qralign_in


# ---- 9: the release build ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_release_build_passes_these_tests(gm):
    """the known-answer and wave-shape tests of this file once more in a child interpreter on libgmapper_hip_release.so"""
    if "release" in os.path.basename(gm.LIB_PATH): return                                       # (this IS the child)
    rel_lib = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel_lib), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "known_answers or wave_shapes", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=dict(os.environ, GM_LIB_PATH=rel_lib), cwd=oa.ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) >= 10, r.stdout[-500:]
