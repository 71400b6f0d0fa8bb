"""gm_select_pass1 / gm_select_pass2 (Session.select_pass1 / select_pass2): the two selections of a read batch as seams on arrays -- the overlap rule, the threshold and
the top-K ext-heap of pass 1 (read_pass1_per_strand, read_get_vector_hits), and the threshold, the two duplicate removals, the sort, the cuts and the mapping qualities
of pass 2 (read_pass2, read_remove_duplicate_hits, compute_unpaired_mqv).

Both rule sets are restated here in Python (restate_pass1 / restate_pass2).  Without a GPU the restatement is pinned to the REFERENCE: pass 1 on the windows of the
tests/read_windows_oracle.cpp driver (it keeps equal windows in the reference's order) with the oracle's vector filter must give oracle_api.Session.tophits row for row
in heap order (the f1 cache off in the oracle: the seam does not emulate it); pass 2, chained on those hits through the oracle's sw_vector + sw_full_ls (hit_run_full_sw's
rule), must give strand, contig, AS, MAPQ, Z0, Z1 and the order of every record of the committed reference outputs.  On the GPU the library is held to the restatement
(fixtures and hand-made shapes) and, chained from reads to text, to the reference outputs field by field."""
import ctypes as C
import gzip, math, os, re, subprocess
import numpy as np
import pytest
from tests import oracle_api as oa

GM_E_ARG, GM_E_RANGE = -2, -4
WIN_COLS = ("read", "st", "cn", "g_off", "w_len", "score_window_gen", "matches", "ax", "ay", "alen", "awidth", "reserved")
HIT_COLS = ("read", "st", "win", "cn", "gen_st", "g_off", "w_len", "score_vector", "pct_score_vector", "score_max", "matches", "score_window_gen", "ax", "ay", "alen", "awidth")
MAP_COLS = ("read", "hit", "score_full", "pct_score_full", "mqv", "flags", "posterior", "z0", "z1")
CMPL = np.array([3, 2, 1, 0, 0, 10, 9, 7, 8, 6, 5, 14, 13, 12, 11, 15], dtype=np.uint8)      # complement_base (A C G T U M R W S Y K V H D B N)
THREADS = max(1, min(8, os.cpu_count() or 1))
# fixture -> (match mode, colour space, oracle options, rows of tophits)
FIXTURES = {
    "cfg2s_100bp_2Mbp": (2, False, None, 5289),
    "stress_60bp": (2, False, None, 4898),
    "n1_noisy_70bp": (1, False, "cmw-mode=1", 4692),
    "cfg4s_50col_2Mbp": (2, True, "colour=1", None),
}


# ---- the rules, restated ---------------------------------------------------------------------------------------------------------------------------------------
def abs_or_pct(x, base):
    return -x if x < 0 else base * (x / 100.0)


def rules(match=10, match_mode=2, window_len=140.0, window_overlap=90.0, sw_vect_threshold=50.0, sw_full_threshold=50.0, num_tmp_outputs=30, num_outputs=10,
          strata=0, max_alignments=0, single_best_mapping=0, mqv_on=True, colour=False, alpha=None, beta=None):
    return dict(locals())


def rules_of(p):
    """the rules of a gm_params_t (alpha / beta as gm_session_create derives them, ref: gmapper.c:2550-2571)"""
    if p.colour_space:
        alpha = p.crossover_score / (math.log(p.pr_xover / 3) / math.log(2.0))
        pr_mm = 1.0 / (1.0 + 1.0 / 3.0 * math.pow(2.0, (float(p.match_score) - float(p.mismatch_score)) / alpha))
    else:
        pr_mm = .01
        alpha = (float(p.match_score) - float(p.mismatch_score)) / (math.log((1 - pr_mm) / (pr_mm / 3.0)) / math.log(2.0))
    beta = float(p.match_score) - 2 * alpha - alpha * math.log(1 - pr_mm) / math.log(2.0)
    return rules(match=p.match_score, match_mode=p.match_mode, window_len=p.window_len, window_overlap=p.window_overlap, sw_vect_threshold=p.sw_vect_threshold,
                 sw_full_threshold=p.sw_full_threshold, num_tmp_outputs=p.num_tmp_outputs, num_outputs=p.num_outputs, strata=p.strata, max_alignments=p.max_alignments,
                 single_best_mapping=p.single_best_mapping, mqv_on=not p.local_alignment and not p.no_mapping_qualities, colour=bool(p.colour_space), alpha=alpha, beta=beta)


def letter_alpha_beta(match=10, mismatch=-15):
    pr_mm = .01
    alpha = (float(match) - float(mismatch)) / (math.log((1 - pr_mm) / (pr_mm / 3.0)) / math.log(2.0))
    return alpha, float(match) - 2 * alpha - alpha * math.log(1 - pr_mm) / math.log(2.0)


def restate_pass1(rows, off, scores, read_len, R, clen):
    """rows: the windows as int64 columns WIN_COLS; -> (top, hits, hit_off): top = rows of 12 as tophits has them (the hit BEFORE reverse_hit, heap array order),
    hits = rows of HIT_COLS (after reverse_hit), read r's at [hit_off[r], hit_off[r + 1])"""
    n = (len(off) - 1) // 2
    W = int(abs_or_pct(R["window_len"], read_len)) & 0xFFFF
    ov = int(abs_or_pct(R["window_overlap"], W)) & 0xFFFFFFFF
    absthr = R["sw_vect_threshold"] < 0
    K = R["num_tmp_outputs"]
    top, hits, hit_off = [], [], [0]
    for r in range(n):
        heap = []                                                        # (key, window, score, pct)
        for st in range(2):
            last = None
            for i in range(int(off[2 * r + st]), int(off[2 * r + st + 1])):
                _, _, cn, g_off, w_len, _, matches = (int(x) for x in rows[i, :7])
                if matches < R["match_mode"]: continue                   # mapping.c:1275
                score = int(scores[i])
                score_max = min(read_len, w_len) * R["match"]
                thr = int(abs_or_pct(R["sw_vect_threshold"], score_max))
                if last is not None and cn == last[0] and g_off + ov <= last[1] + W: score = 0      # :1287-1293 (skipped: counts with score 0, last_good stays)
                elif score >= thr: last = (cn, g_off)                    # :1332-1335
                pct = (1000 * 100 * score) // score_max
                key = score if absthr else pct
                if score >= thr and (len(heap) < K or key > heap[0][0]): # :1391-1396
                    e = (key, i, score, pct)
                    if len(heap) < K:                                    # heap.h: insert, percolate up with a strict <
                        heap.append(e); node = len(heap)
                        while node > 1 and heap[node - 1][0] < heap[node // 2 - 1][0]:
                            heap[node - 1], heap[node // 2 - 1] = heap[node // 2 - 1], heap[node - 1]; node //= 2
                    else:                                                # replace the minimum, percolate down
                        heap[0] = e; node = 1
                        while True:
                            left, right, mn = 2 * node, 2 * node + 1, node
                            if left <= len(heap) and heap[left - 1][0] < heap[node - 1][0]: mn = left
                            if right <= len(heap) and heap[right - 1][0] < heap[mn - 1][0]: mn = right
                            if mn == node: break
                            heap[mn - 1], heap[node - 1] = heap[node - 1], heap[mn - 1]; node = mn
        for key, i, score, pct in heap:
            rd, st, cn, g_off, w_len, swg, matches, ax, ay, alen, awidth = (int(x) for x in rows[i, :11])
            top.append((rd, st, cn, g_off, w_len, score, pct, matches, ax, ay, alen, awidth))
            if st:                                                       # reverse_hit (mapping.c:254-263), anchor_reverse (anchors.h:30-34)
                g_off = int(clen[cn]) - g_off - w_len
                ax = -ax + (w_len - 1) - (alen - 1) - (awidth - 1); ay = -ay + (read_len - 1) - (alen - 1) + (awidth - 1)
            hits.append((rd, st, i, cn, st, g_off, w_len, score, pct, min(read_len, w_len) * R["match"], matches, swg, ax, ay, alen, awidth))
        hit_off.append(len(hits))
    return (np.array(top, dtype=np.int64).reshape(-1, 12), np.array(hits, dtype=np.int64).reshape(-1, 16), np.array(hit_off, dtype=np.uint64))


def qv_from_pr_corr(pr_corr):                                            # util.h:267-283
    pr_err = 1 - pr_corr
    if pr_err > .99999999: return 0
    if pr_err < 1E-25: return 250
    return int(-10.0 * math.log(pr_err) / math.log(10.0))


def restate_pass2(hits, hit_off, recs, R, post=None):
    """hits: rows of HIT_COLS; recs: per hit a dict-like with score rmapped genome_start insertions deletions status; post: per hit (posterior, status) in colour space
    -> (maps, map_off): maps = rows (read, hit, score_full, pct_score_full, mqv, posterior, z0, z1) in output order"""
    a, b = R["alpha"], R["beta"]
    thr_abs = R["sw_full_threshold"] < 0
    maps, map_off = [], [0]
    for r in range(len(hit_off) - 1):
        cand = []
        for i in range(int(hit_off[r]), int(hit_off[r + 1])):
            h = hits[i]; cn, gen_st, score_max = int(h[3]), int(h[4]), int(h[9])
            rec = recs[i]
            sf = 0 if int(rec["status"]) < 0 else int(rec["score"]); posterior = 0.0; rmapped = int(rec["rmapped"])
            if sf > 0 and R["mqv_on"]:                                   # hit_run_post_sw, mapping.c:1609-1625
                if R["colour"]:
                    if int(post[i]["status"]) < 0: sf = 0
                    else: posterior = float(post[i]["posterior"])
                else: posterior = math.pow(2.0, (float(sf) - float(rmapped) * (2.0 * a + b)) / a)
                if sf > 0: sf = max(0, int(np.rint(a * math.log(posterior) / math.log(2.0) + float(rmapped) * (2.0 * a + b))))
            pct = (1000 * 100 * sf) // score_max
            key = sf if thr_abs else pct
            if sf >= abs_or_pct(R["sw_full_threshold"], score_max):      # mapping.c:1661, as doubles
                gs = int(rec["genome_start"])
                cand.append(dict(i=i, sf=sf, pct=pct, key=key, posterior=posterior, start=(cn, gen_st, gs),
                                 end=(cn, gen_st, -gs - rmapped + int(rec["deletions"]) - int(rec["insertions"]))))
        for which in ("start", "end"):                                   # read_remove_duplicate_hits, mapping.c:1552-1600
            cand.sort(key=lambda c: c[which])                            # (stable)
            kept, k = [], 0
            while k < len(cand):
                j = k; best = k
                while j < len(cand) and cand[j][which] == cand[k][which]:
                    if cand[j]["key"] > cand[best]["key"]: best = j
                    j += 1
                kept.append(cand[best]); k = j
            cand = kept
        cand.sort(key=lambda c: -c["key"])
        cand = cand[:R["num_outputs"]]
        if R["strata"] and cand: cand = [c for k, c in enumerate(cand) if all(x["sf"] == cand[0]["sf"] for x in cand[:k + 1])]
        if R["max_alignments"] and len(cand) > R["max_alignments"]: cand = []
        out = []
        if cand and R["mqv_on"]:                                         # compute_unpaired_mqv, output.c:777-793
            z1 = 0.0
            for c in cand: z1 += c["posterior"]
            for c in cand:
                q = qv_from_pr_corr(c["posterior"] / z1)
                out.append((r, c["i"], c["sf"], c["pct"], 0 if q < 4 else q, c["posterior"], c["posterior"], z1))
            if R["single_best_mapping"]: out = [max(out, key=lambda m: m[4])]      # (max keeps the first of equals)
        else: out = [(r, c["i"], c["sf"], c["pct"], 255, 0.0, 0.0, 0.0) for c in cand]
        maps += out; map_off.append(len(maps))
    return maps, np.array(map_off, dtype=np.uint64)


# ---- the reference's side ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/read_windows_oracle.cpp, compiled as tests/test_read_windows.py compiles it"""
    so = str(tmp_path_factory.mktemp("rwo_sel") / "librwo.so")
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


def pack(codes):
    from shrimp_amd import synth
    return synth.pack_nibbles(np.asarray(codes, dtype=np.uint8))


def colours(letters):
    a = np.concatenate([[3], letters[:-1]]).astype(np.int64); b = letters.astype(np.int64)
    return np.where((a > 3) | (b > 3), 15, a ^ b).astype(np.uint8)


_u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
_ref = {}


def reference(L, name):
    """everything the CPU side knows of a fixture, computed once: the driver's windows, the oracle's vector score of each as pass 1 takes it (letter space: the forward
    window against the read or its reverse complement, mapping.c:1321-1328; colour space: the turned window against the read as given, :1297-1319), the oracle's top
    hits (f1 cache off), the strands' bitfields"""
    if name in _ref: return _ref[name]
    mode, colour, opts, _ = FIXTURES[name]
    contigs, reads, _ = oa.load_golden(name)
    cs = [np.ascontiguousarray(c, dtype=np.uint8) for c in contigs]; reads = np.ascontiguousarray(reads, dtype=np.uint8)
    u8p = C.POINTER(C.c_uint8)
    h = L.rwo_create(len(cs), (u8p * len(cs))(*[c.ctypes.data_as(u8p) for c in cs]), (C.c_uint64 * len(cs))(*[len(c) for c in cs]), int(colour), mode)
    cap = 64 * len(reads); rows = np.zeros((cap, 12), dtype=np.int64)
    w = L.rwo_windows(h, reads.shape[0], reads.shape[1], reads.ctypes.data_as(u8p), THREADS, rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
    L.rwo_destroy(h)
    assert 0 < w <= cap
    rows = rows[:w].copy()
    key = rows[:, 0] * 2 + rows[:, 1]
    off = np.searchsorted(key, np.arange(2 * len(reads) + 1)).astype(np.uint64)
    clen = np.array([len(c) for c in cs], dtype=np.int64)
    letters = [[c, CMPL[c[::-1]]] for c in cs]
    ls = [[pack(x) for x in pair] for pair in letters]
    csb = [[pack(colours(x)) for x in pair] for pair in letters] if colour else None
    rw = [pack(r[1:] if colour else r) for r in reads]; rlen = reads.shape[1] - (1 if colour else 0)
    rc = None if colour else [pack(CMPL[r[::-1]]) for r in reads]
    O = oa.load()
    scores = np.zeros(w, dtype=np.int32)
    for i in range(w):
        rd, st, cn, g_off, wl = (int(x) for x in rows[i, :5])
        go = g_off if st == 0 else int(clen[cn]) - g_off - wl
        if colour: scores[i] = O.gmo_sw_vector_cs(_u32(csb[cn][st]), go, wl, _u32(rw[rd]), rlen, _u32(ls[cn][st]), int(reads[rd, 0]))
        else: scores[i] = O.gmo_sw_vector(_u32(ls[cn][0]), g_off, wl, _u32(rc[rd] if st else rw[rd]), rlen)      # pass 1, letter space: the forward contig, strand 1 of the READ
    top = None
    if not colour:                                                       # (the oracle's stage dump reads letters)
        S = oa.Session(contigs, opts=opts); S.set(hash_filter_calls=False)
        top = S.tophits(reads, nthreads=THREADS).copy(); S.close()
    _ref[name] = dict(contigs=cs, reads=reads, rows=rows, off=off, scores=scores, top=top, clen=clen, ls=ls, rw=rw, rlen=rlen, colour=colour, mode=mode)
    return _ref[name]


def fixture_rules(name, **over):
    mode, colour = FIXTURES[name][:2]
    a, b = letter_alpha_beta()
    R = rules(match_mode=mode, colour=colour, alpha=a, beta=b)
    if colour: R.update(sw_vect_threshold=47.0, sw_full_threshold=50.0)
    R.update(over)
    return R


def sam_records(name, tag=None):
    """mapped records of a reference output: (read, strand, contig, POS, MAPQ, CIGAR, tags)"""
    f = "%s@%s.sam.gz" % (name, tag) if tag else name + ".sam.gz"
    out = []
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", f), "rt") as fh:
        for line in fh:
            if line.startswith("@"): continue
            t = line.rstrip("\n").split("\t")
            if int(t[1]) & 4: continue
            tags = {x[:2]: x[5:] for x in t[11:]}
            out.append((int(t[0][1:]), 1 if int(t[1]) & 16 else 0, int(t[2][len("contig"):]) - 1, int(t[3]), int(t[4]), t[5], tags))
    return out


def neglog(x): return int(1000.0 * -math.log(x))                        # double_to_neglog, util.h:297-301


_full = {}


def oracle_full(L, name):
    """hit_run_full_sw's rule (mapping.c:331-401) with the oracle's routines on the restatement's hits of a letter-space fixture: -> (hits, hit_off, recs)"""
    if name in _full: return _full[name]
    F = reference(L, name); R = fixture_rules(name)
    _, hits, hit_off = restate_pass1(F["rows"], F["off"], F["scores"], F["rlen"], R, F["clen"])
    O = oa.load(); out = (C.c_int * 9)(); db = C.create_string_buffer(4096); qr = C.create_string_buffer(4096)
    recs = np.zeros(len(hits), dtype=[(k, np.int64) for k in ("score", "read_start", "rmapped", "genome_start", "gmapped", "matches", "mismatches", "insertions", "deletions", "status")])
    for i, h in enumerate(hits):
        rd, _, _, cn, gen_st, g_off, w_len = (int(x) for x in h[:7]); ax, ay, alen, awidth = (int(x) for x in h[12:16])
        thresh = int(abs_or_pct(R["sw_full_threshold"], int(h[9])))
        sv = O.gmo_sw_vector(_u32(F["ls"][cn][gen_st]), g_off, w_len, _u32(F["rw"][rd]), F["rlen"])
        if sv < thresh: continue
        O.gmo_sw_full_ls(_u32(F["ls"][cn][gen_st]), g_off, w_len, _u32(F["rw"][rd]), F["rlen"], ax, ay, alen, awidth, gen_st, out, db, qr, 4096)      # revcmpl = gen_st && Tflag
        recs[i] = tuple(out) + (0,)
    _full[name] = (hits, hit_off, recs)
    return _full[name]


# ---- CPU: the restatement against the reference -------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries_and_their_record_sizes():
    """fails without the feature"""
    try: import torch                                                    # (as in the gm fixture below: where torch is installed its HIP runtime is loaded before the library's)
    except Exception: pass
    from shrimp_amd import gmapper as gm
    L = gm.lib()
    header = open(os.path.join(oa.ROOT, "include", "gmapper_hip.h")).read()
    for name in ("gm_select_pass1", "gm_select_pass2", "gm_pass1_hit_size", "gm_mapping_size"):
        assert hasattr(L, name) and name in gm.EXPORTS and re.search(r"\b%s\(" % name, header), name
    assert L.gm_pass1_hit_size() == 64 == C.sizeof(gm.Pass1Hit) == gm.PASS1_HIT_DTYPE.itemsize
    assert gm.PASS1_HIT_DTYPE.names == HIT_COLS and [gm.PASS1_HIT_DTYPE.fields[c][1] for c in HIT_COLS] == list(range(0, 64, 4))
    assert L.gm_mapping_size() == 48 == C.sizeof(gm.Mapping) == gm.MAPPING_DTYPE.itemsize
    assert gm.MAPPING_DTYPE.names == MAP_COLS and [gm.MAPPING_DTYPE.fields[c][1] for c in MAP_COLS] == [0, 4, 8, 12, 16, 20, 24, 32, 40]
    assert [L.gm_abi_sizeof(k) for k in range(6)] == [C.sizeof(gm.Params), C.sizeof(gm.PairOpts), C.sizeof(gm.MapStats), C.sizeof(gm.MergeOptions), C.sizeof(gm.SwFullRec), C.sizeof(gm.PostRec)]
    assert L.gm_abi_sizeof(6) == -1                                  # the list of gm_abi_sizeof stays 0..5: the records have their own size functions


@pytest.mark.parametrize("name", ["cfg2s_100bp_2Mbp", "stress_60bp", "n1_noisy_70bp"])
def test_restated_pass1_gives_the_top_hits_of_the_reference_in_heap_order(driver, name):
    F = reference(driver, name)
    top, hits, hit_off = restate_pass1(F["rows"], F["off"], F["scores"], F["rlen"], fixture_rules(name), F["clen"])
    want = F["top"]
    assert len(want) == FIXTURES[name][3]
    assert top.shape == want.shape, (top.shape, want.shape)
    bad = np.nonzero((top != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), top[bad[:5]], want[bad[:5]])
    assert int(hit_off[-1]) == len(hits) == len(top)
    if name == "stress_60bp": assert int(np.diff(hit_off.astype(np.int64)).max()) == 30      # reads that fill every slot of the heap


@pytest.mark.parametrize("name,tag,over,n_records", [
    ("cfg2s_100bp_2Mbp", None, {}, None),
    ("stress_60bp", None, {}, 3554),
    ("stress_60bp", "strata", dict(strata=1), None),
    ("stress_60bp", "max3_o5", dict(max_alignments=3, num_outputs=5), None),
    ("stress_60bp", "single_best", dict(single_best_mapping=1), None)])
def test_restated_pass2_gives_the_records_of_the_reference(driver, name, tag, over, n_records):
    """strand, contig, AS, MAPQ, Z0, Z1 of every record, in the reference's order"""
    hits, hit_off, recs = oracle_full(driver, name)
    maps, map_off = restate_pass2(hits, hit_off, recs, fixture_rules(name, **over))
    want = sam_records(name, tag)
    if n_records is not None: assert len(want) == n_records
    got = [(m[0], int(hits[m[1], 4]), int(hits[m[1], 3]), m[4], m[2], neglog(m[6]), neglog(m[7])) for m in maps]
    exp = [(w[0], w[1], w[2], w[4], int(w[6]["AS"]), int(w[6]["Z0"]), int(w[6]["Z1"])) for w in want]
    assert len(got) == len(exp), (len(got), len(exp))
    bad = [k for k in range(len(got)) if got[k] != exp[k]]
    assert not bad, (len(bad), [(got[k], exp[k]) for k in bad[:5]])
    if tag is None:                                                      # duplicates were there to prune: hits at or above the threshold that are not records
        R = fixture_rules(name)
        passing = sum(1 for i in range(len(hits)) if recs[i]["score"] >= abs_or_pct(R["sw_full_threshold"], int(hits[i, 9])))
        pruned_or_cut = passing - len(maps)
        assert pruned_or_cut >= {"cfg2s_100bp_2Mbp": 289, "stress_60bp": 173}[name], pruned_or_cut


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------------------------
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


def win_rows(wins):
    return np.stack([wins[c].astype(np.int64) for c in WIN_COLS], axis=1) if len(wins) else np.zeros((0, 12), dtype=np.int64)


def hit_rows(hits):
    return np.stack([hits[c].astype(np.int64) for c in HIT_COLS], axis=1) if len(hits) else np.zeros((0, 16), dtype=np.int64)


def as_wins(gm, rows):
    w = np.zeros(len(rows), dtype=gm.READ_WINDOW_DTYPE)
    for k, c in enumerate(WIN_COLS): w[c] = rows[:, k]
    return w


def as_hits(gm, rows):
    h = np.zeros(len(rows), dtype=gm.PASS1_HIT_DTYPE)
    for k, c in enumerate(HIT_COLS): h[c] = rows[:, k]
    return h


def params_of(gm, name, **fields):
    mode, colour = FIXTURES[name][:2]
    p = gm.default_params_cs() if colour else gm.default_params()
    p.match_mode = mode
    for k, v in fields.items(): setattr(p, k, v)
    return p


_open = {}


def opened(gm, name, fields=None):
    """(index, session, params, reads) of a fixture under its own match mode and the given gm_params_t fields, kept open for the module"""
    key = (name, tuple(sorted((fields or {}).items())))
    if key not in _open:
        contigs, reads, _ = oa.load_golden(name)
        p = params_of(gm, name, **(fields or {}))
        ix = gm.Index(contigs, params=p)
        s = gm.Session(ix, params=p, max_batch_reads={"n1_noisy_70bp": 4096, "stress_60bp": 8192}.get(name, 131072))
        _open[key] = (ix, s, p, np.ascontiguousarray(reads, dtype=np.uint8))
    return _open[key]


def vector_setup(gm, p):
    colour = bool(p.colour_space)
    gm.sw_vector_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score,
                       p.match_score + p.crossover_score if colour else p.mismatch_score, 1 if colour else 0, True)


def library_scores(gm, ix, p, reads, rows):
    """gm_sw_vector_batch_ix on every window as pass 1 scores it: -> (scores, the packed reads, their length)"""
    from shrimp_amd import synth
    colour = bool(p.colour_space)
    body = np.ascontiguousarray(reads[:, 1:]) if colour else reads
    rw = np.ascontiguousarray(synth.pack_reads(body)); clen = ix.contig_lengths()
    vector_setup(gm, p)
    st = rows[:, 1]; rd = rows[:, 0]; lens = np.full(len(rows), body.shape[1])
    if colour:                                                           # the hit turned onto the read's input strand, the read as given
        goff = np.where(st == 0, rows[:, 3], clen[rows[:, 2]] - rows[:, 3] - rows[:, 4])
        return ix.sw_vector_batch(rows[:, 2], st.astype(np.uint8), goff, rows[:, 4], rw[rd], lens, initbp=reads[rd, 0]), rw, body.shape[1]
    rc = np.ascontiguousarray(synth.pack_reads(np.ascontiguousarray(CMPL[body[:, ::-1]])))     # the forward window, strand 1 of the read
    both = np.where((st == 1)[:, None], rc[rd], rw[rd])
    return ix.sw_vector_batch(rows[:, 2], np.zeros(len(rows), dtype=np.uint8), rows[:, 3], rows[:, 4], both, lens), rw, body.shape[1]


def unturned(hits, read_len, clen):
    """rows of tophits from hit rows: strand-1 hits turned back (reverse_hit and anchor_reverse are their own inverses)"""
    h = hits.copy(); t = h[:, 1] == 1
    h[t, 5] = clen[h[t, 3]] - h[t, 5] - h[t, 6]
    h[t, 12] = -h[t, 12] + (h[t, 6] - 1) - (h[t, 14] - 1) - (h[t, 15] - 1)
    h[t, 13] = -h[t, 13] + (read_len - 1) - (h[t, 14] - 1) + (h[t, 15] - 1)
    return h[:, [0, 1, 3, 5, 6, 7, 8, 10, 12, 13, 14, 15]]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_pass1_on_the_driver_windows_equals_the_restatement_and_the_top_hits(gm, driver, name):
    """the driver's windows (equal windows in the reference's order), scores from gm_sw_vector_batch_ix: every column of every hit, anchors included"""
    F = reference(driver, name)
    ix, s, p, reads = opened(gm, name)
    scores, _, rlen = library_scores(gm, ix, p, reads, F["rows"])
    assert np.array_equal(scores, F["scores"])
    hits, hit_off = s.select_pass1(as_wins(gm, F["rows"]), F["off"], scores, rlen)
    top, want, want_off = restate_pass1(F["rows"], F["off"], scores, rlen, rules_of(p), F["clen"])
    got = hit_rows(hits)
    assert np.array_equal(hit_off, want_off)
    assert np.array_equal(got, want), (got[(got != want).any(axis=1)][:5], want[(got != want).any(axis=1)][:5])
    # the reference's own top hits (letter space: the oracle's, its f1 cache off; colour space, where the oracle has no such dump: the mapping pipeline's)
    top_ref = s.tophits(reads[:, 1:], initbp=reads[:, 0]) if p.colour_space else F["top"]
    assert len(top_ref) > 3000 and np.array_equal(unturned(got, rlen, F["clen"]), top_ref)


def tie_mask(rows):
    """windows that share (read, st, cn, g_off) with another window"""
    key = rows[:, :4]
    order = np.lexsort(key.T[::-1]); k = key[order]
    eq = (k[1:] == k[:-1]).all(axis=1)
    m = np.zeros(len(rows), dtype=bool); m[order[1:]] |= eq; m[order[:-1]] |= eq
    return m


_chain = {}


def library_pass1(gm, name, fields=None):
    """read_windows -> vector batch -> select_pass1 on a fixture, made once"""
    key = (name, tuple(sorted((fields or {}).items())))
    if key not in _chain:
        ix, s, p, reads = opened(gm, name, fields)
        colour = bool(p.colour_space)
        wins, off = s.read_windows(reads[:, 1:], initbp=reads[:, 0]) if colour else s.read_windows(reads)
        rows = win_rows(wins)
        scores, rw, rlen = library_scores(gm, ix, p, reads, rows)
        hits, hit_off = s.select_pass1(wins, off, scores)               # (read_len: that of the read_windows call)
        _chain[key] = dict(wins=wins, rows=rows, off=off, scores=scores, rw=rw, rlen=rlen, hits=hits, hit_off=hit_off)
    return _chain[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_pass1_on_read_windows_equals_the_restatement(gm, name):
    """windows from gm_read_windows: groups of equal (read, st, cn, g_off) come in no promised order, so hits inside such a group are compared without the anchor box"""
    ix, s, p, reads = opened(gm, name)
    c = library_pass1(gm, name)
    _, want, want_off = restate_pass1(c["rows"], c["off"], c["scores"], c["rlen"], rules_of(p), ix.contig_lengths())
    got = hit_rows(c["hits"])
    assert np.array_equal(c["hit_off"], want_off) and got.shape == want.shape
    tied = tie_mask(c["rows"])
    groups = len(np.unique(c["rows"][tied][:, :4], axis=0)) if tied.any() else 0
    assert groups == (33 if name == "stress_60bp" else 0)
    in_group = tied[want[:, 2]]
    cols = np.ones(16, dtype=bool); cols[[2, 12, 13, 14, 15]] = False   # (which of two equal windows: win and the box)
    assert np.array_equal(got[~in_group], want[~in_group])
    assert np.array_equal(got[in_group][:, cols], want[in_group][:, cols])
    assert tied[got[in_group][:, 2]].all()


# hand-made pass-1 shapes: synthetic windows and scores on the cfg2 session (100 bp: W = 140, overlap 126, threshold 50 % = 500 of 1000, K = 30)
def shape_windows(lists):
    """lists: per read-strand a list of (cn, g_off, w_len, score[, matches]) -> rows, off, scores"""
    rows, scores, off = [], [], [0]
    for rs, lst in enumerate(lists):
        for k, w in enumerate(lst):
            cn, g_off, w_len, score = w[:4]; matches = w[4] if len(w) > 4 else 2
            rows.append((rs // 2, rs & 1, cn, g_off, w_len, 300 + k, matches, 3 + k % 5, 2 + k % 3, 11 + k % 4, 1 + k % 2, 0)); scores.append(score)
        off.append(len(rows))
    return np.array(rows, dtype=np.int64).reshape(-1, 12), np.array(off, dtype=np.uint64), np.array(scores, dtype=np.int32)


def run_shape(gm, s, p, lists, read_len, clen):
    rows, off, scores = shape_windows(lists)
    hits, hit_off = s.select_pass1(as_wins(gm, rows), off, scores, read_len)
    top, want, want_off = restate_pass1(rows, off, scores, read_len, rules_of(p), clen)
    got = hit_rows(hits)
    assert np.array_equal(hit_off, want_off), (hit_off, want_off)
    assert np.array_equal(got, want), (got[(got != want).any(axis=1)][:5], want[(got != want).any(axis=1)][:5])
    return got, hit_off


def spaced(n, score_of, cn=0, start=1000, step=200, w_len=140):
    return [(cn, start + step * k, w_len, score_of(k)) for k in range(n)]


@pytest.mark.gpu
def test_pass1_hand_made_shapes(gm):
    ix, s, p, _ = opened(gm, "cfg2s_100bp_2Mbp")
    clen = ix.contig_lengths(); L = 100
    W, ov = 140, 126
    # the overlap boundary: g_off + 126 <= last + 140 exactly (skipped) and one beyond (kept); a contig change; a window below the threshold between two passing ones
    got, _ = run_shape(gm, s, p, [[(0, 5000, 140, 900), (0, 5000 + W - ov, 140, 950), (0, 5000 + W - ov + 1, 140, 800)], []], L, clen)
    assert got[:, 7].tolist() == [900, 800] or sorted(got[:, 7].tolist()) == [800, 900]
    got, _ = run_shape(gm, s, p, [[(0, 5000, 140, 900), (1, 5005, 140, 950)], []], L, clen)
    assert len(got) == 2
    got, _ = run_shape(gm, s, p, [[(0, 5000, 140, 900), (0, 5020, 140, 300), (0, 5027, 140, 990)], []], L, clen)      # last_good stays at 5000: 5027 + 126 > 5140, kept
    assert sorted(got[:, 7].tolist()) == [900, 990]
    got, _ = run_shape(gm, s, p, [[(0, 5000, 140, 300), (0, 5010, 140, 990), (0, 5014, 140, 995)], []], L, clen)      # the failing window is no last_good; 5014 is skipped by 5010
    assert got[:, 7].tolist() == [990]
    # a window clamped shorter than the read: score_max from w_len (450 passes 50 % of 800, not 50 % of 1000)
    got, _ = run_shape(gm, s, p, [[(0, 0, 80, 450), (0, 1000, 140, 450)], []], L, clen)
    assert got[:, [6, 9]].tolist() == [[80, 800]]
    # a match count below match_mode is passed over, whatever its score, and is no last_good
    run_shape(gm, s, p, [[(0, 5000, 140, 1000, 1), (0, 5010, 140, 900, 2)], []], L, clen)
    # lists of 1, 63, 64, 65, 128 and 283 windows; the passing chain crosses the 64-window step (every window overlaps the one before; every third passes)
    for n in (1, 63, 64, 65, 128, 283):
        run_shape(gm, s, p, [[(0, 2000 + 10 * k, 140, 900 - k if k % 3 == 0 else 100) for k in range(n)], [(1, 900 + 9 * k, 140, 700 + k) for k in range(n)]], L, clen)
        run_shape(gm, s, p, [[(0, 2000 + 10 * k, 140, 900 - (k % 50)) for k in range(n)], []], L, clen)
    # exactly K, K + 1 and 3 K candidates, ascending, descending and mixed keys; equal keys at the heap minimum are not admitted
    for n in (30, 31, 90):
        for score_of in (lambda k: 600 + k, lambda k: 990 - k, lambda k: 600 + (k * 37) % 97, lambda k: 700):
            run_shape(gm, s, p, [spaced(n, score_of), []], L, clen)
            run_shape(gm, s, p, [spaced(n // 2, score_of), spaced(n - n // 2, score_of, cn=1)], L, clen)
    got, _ = run_shape(gm, s, p, [spaced(30, lambda k: 700) + [(0, 9000, 140, 700)], []], L, clen)
    assert 30 not in got[:, 2].tolist() and len(got) == 30
    # candidates only on strand 1; empty reads between full ones; a strand-1 hit that ends at the end of its contig (turned g_off 0)
    end = int(clen[2]) - 140
    got, hit_off = run_shape(gm, s, p, [[], spaced(5, lambda k: 800 + k), [], [], [(2, end, 140, 900)], [(2, end, 140, 900)], [], [], spaced(40, lambda k: 650 + k), spaced(3, lambda k: 999)], L, clen)
    assert hit_off.tolist() == [0, 5, 5, 7, 7, 37]
    assert got[5, [1, 4, 5]].tolist() == [0, 0, end] and got[6, [1, 4, 5]].tolist() == [1, 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("fields", [dict(sw_vect_threshold=-650.0), dict(num_tmp_outputs=1), dict(num_tmp_outputs=64), dict(window_len=-120.0, window_overlap=-100.0)])
def test_pass1_under_other_rules(gm, fields):
    """an absolute threshold (the key is the score), K = 1 and K = 64, absolute window length and overlap"""
    ix, _, _, _ = opened(gm, "cfg2s_100bp_2Mbp")
    p = params_of(gm, "cfg2s_100bp_2Mbp", **fields)
    s = gm.Session(ix, params=p, max_batch_reads=1024)
    clen = ix.contig_lengths()
    for n in (1, 64, 65, 200):
        run_shape(gm, s, p, [[(0, 2000 + 15 * k, 80 + (k * 7) % 61, 350 + (k * 53) % 500) for k in range(n)], spaced(n, lambda k: 640 + (k * 11) % 30, cn=1)], 100, clen)
    s.close()


def fake_recs(gm, items):
    """items: per hit (score, genome_start, rmapped, insertions, deletions[, status])"""
    recs = np.zeros(len(items), dtype=gm.SW_FULL_REC_DTYPE)
    for i, it in enumerate(items):
        recs[i]["score"], recs[i]["genome_start"], recs[i]["rmapped"], recs[i]["insertions"], recs[i]["deletions"] = it[:5]
        recs[i]["status"] = it[5] if len(it) > 5 else 0
        recs[i]["gmapped"] = it[2] + it[3] - it[4]
    return recs


def fake_hits(per_read):
    """per read a list of (cn, gen_st) -> hit rows with score_max 1000, hit_off"""
    rows, off = [], [0]
    for r, lst in enumerate(per_read):
        for cn, gen_st in lst: rows.append((r, gen_st, len(rows), cn, gen_st, 100, 140, 900, 90000, 1000, 2, 300, 0, 0, 10, 1))
        off.append(len(rows))
    return np.array(rows, dtype=np.int64).reshape(-1, 16), np.array(off, dtype=np.uint64)


def check_pass2(gm, s, p, per_read, items, post=None):
    hits, hit_off = fake_hits(per_read)
    recs = fake_recs(gm, items)
    maps, map_off = s.select_pass2(as_hits(gm, hits), hit_off, recs, post)
    want, want_off = restate_pass2(hits, hit_off, recs, rules_of(p), post)
    assert np.array_equal(map_off, want_off), (map_off, want_off)
    got = [tuple(m[c].item() for c in ("read", "hit", "score_full", "pct_score_full", "mqv", "posterior", "z0", "z1")) for m in maps]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]
    assert (maps["flags"] == 0).all()
    return maps, map_off


@pytest.mark.gpu
@pytest.mark.parametrize("fields", [dict(), dict(strata=1), dict(strata=1, num_outputs=3), dict(max_alignments=3), dict(max_alignments=3, num_outputs=5), dict(single_best_mapping=1),
                                    dict(sw_full_threshold=-700.0), dict(no_mapping_qualities=1), dict(num_outputs=64)])
def test_pass2_hand_made_shapes(gm, fields):
    ix, _, _, _ = opened(gm, "cfg2s_100bp_2Mbp")
    p = params_of(gm, "cfg2s_100bp_2Mbp", **fields)
    s = gm.Session(ix, params=p, max_batch_reads=1024)
    per_read, items = [], []
    def read(hits_and_items):
        per_read.append([h for h, _ in hits_and_items]); items.extend(it for _, it in hits_and_items)
    f0, f1, r0 = (0, 0), (1, 0), (0, 1)
    read([(f0, (900, 500, 100, 0, 0)), (f0, (950, 500, 98, 0, 0)), (f0, (940, 700, 100, 0, 0))])                      # equal start, different ends: the larger key stays
    read([(f0, (900, 500, 100, 0, 0)), (f0, (950, 502, 98, 0, 0)), (f0, (700, 900, 100, 0, 0))])                      # different starts, equal end
    read([(f0, (900, 500, 100, 0, 0)), (f0, (900, 500, 100, 1, 1)), (f0, (900, 500, 100, 0, 0))])                     # a run of three equal keys: the first stays
    read([(f0, (900, 500, 100, 0, 0)), (r0, (900, 500, 100, 0, 0)), (f1, (900, 500, 100, 0, 0)), (f0, (910, 500, 100, 0, 0))])      # duplicates over both strands / contigs: never merged
    read([(f0, (400, 500 + 200 * k, 100, 0, 0)) for k in range(12)])                                                  # all below 50 %
    read([])
    read([(f0, (900, 1000 * k, 100, 0, 0)) for k in range(4)] + [(f0, (800, 9000, 100, 0, 0))])                       # strata: a tie across a cut at 3; max_alignments 3 exceeded
    read([(f0, (900, 1000 * k, 100, 0, 0)) for k in range(3)])                                                        # max_alignments hit exactly
    read([(f0, (900, 100, 100, 0, 0, GM_E_ARG)), (f0, (950, 400, 100, 0, 0)), (f1, (990, 400, 100, 0, 0, GM_E_RANGE)), (f1, (700, 800, 100, 0, 0))])   # refused records among answered ones
    read([((k % 3, k & 1), (700 + (k * 29) % 290, 100 * (k % 16), 100 - k % 3, k % 2, (k // 2) % 2)) for k in range(64)])           # 64 items, many duplicates
    read([(f0, (1000 - 5 * k, 300 * k, 100, 0, 0)) for k in range(40)])                                               # 40 distinct, descending
    read([(f0, (805 + 5 * k, 300 * k, 100, 0, 0)) for k in range(40)])                                                # ... ascending
    maps, map_off = check_pass2(gm, s, p, per_read, items)
    if not fields:
        assert np.diff(map_off.astype(np.int64)).tolist()[:9] == [2, 2, 1, 3, 0, 0, 5, 3, 2]
        assert maps["hit"][:5].tolist() == [1, 2, 4, 5, 6]
    s.close()


# ---- the chain from reads to text -----------------------------------------------------------------------------------------------------------------------------------
# reference output -> the gm_params_t fields it was written under (oracle_api.SAM_TAIL_CASES; the noisy reads here under the default match mode 2)
CHAINS = {"cfg2s_100bp_2Mbp@extra_fields": dict(extra_sam_fields=1), "n1_noisy_70bp@extra_fields_rg_unal": dict(extra_sam_fields=1, read_group=b"grp1", sam_unaligned=1, match_mode=2),
          "cfg4s_50col_2Mbp@cs_extra_rg": dict(extra_sam_fields=1, read_group=b"grp1", sam_unaligned=1), "stress_60bp": dict()}


def full_setup(gm, p):
    if p.colour_space:
        gm.sw_full_cs_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, p.crossover_score,
                            True, p.anchor_width, p.indel_taboo_len)
    else:
        gm.sw_full_ls_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, True, p.anchor_width)


def post_setup(gm, p):
    """post_sw_setup as gmapper-cs calls it (gmapper.c:2557-2572, 2959-2963): pr_xover => alpha => pr_mismatch, the gap probabilities from the scores"""
    R = rules_of(p); a, b = R["alpha"], R["beta"]
    pr_mm = 1.0 / (1.0 + 1.0 / 3.0 * math.pow(2.0, (float(p.match_score) - float(p.mismatch_score)) / a))
    gm.post_sw_setup(1400, pr_mm, p.pr_xover, math.pow(2.0, float(p.a_gap_open_score) / a), math.pow(2.0, float(p.a_gap_extend_score) / a),
                     math.pow(2.0, float(p.b_gap_open_score) / a), math.pow(2.0, (float(p.b_gap_extend_score) - b) / a))


def map_tuples(maps):
    return [tuple(m[c].item() for c in ("read", "hit", "score_full", "pct_score_full", "mqv", "posterior", "z0", "z1")) for m in maps]


@pytest.mark.gpu
@pytest.mark.parametrize("golden", sorted(CHAINS))
def test_chain_from_reads_to_the_records_of_the_reference(gm, golden):
    """gm_read_windows -> gm_sw_vector_batch_ix -> gm_select_pass1 -> gm_sw_full_ls_batch_ix (colour space: gm_sw_full_cs_batch_ix + gm_post_sw_batch_ix) ->
    gm_select_pass2 -> gm_sw_full_batch_text_ix: FLAG strand, RNAME, POS, MAPQ, CIGAR, AS, Z0, Z1 and, where the reference printed them, ZM ZR ZV ZH ZE of every mapped
    record, in the reference's order; then the mapping entry on the same session"""
    name, _, tag = golden.partition("@")
    ix, s, p, reads = opened(gm, name, CHAINS[golden])
    colour = bool(p.colour_space); extra = bool(CHAINS[golden].get("extra_sam_fields"))
    c = library_pass1(gm, name, CHAINS[golden])
    hits, hit_off = c["hits"], c["hit_off"]; rlen = c["rlen"]; n = len(hits)
    full_setup(gm, p)
    thresh = np.array([int(abs_or_pct(p.sw_full_threshold, sm)) for sm in hits["score_max"]], dtype=np.int32)
    anchors = [(int(h["ax"]), int(h["ay"]), int(h["alen"]), int(h["awidth"])) for h in hits]
    rw = c["rw"][hits["read"]]; lens = np.full(n, rlen)
    cn, gst, goff, wl = hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"]
    revcmpl = (hits["gen_st"] == 1).astype(np.uint8) if p.tiebreak_rev else None                # rh->gen_st && Tflag
    post = None; qbuf = None; ib = None
    if colour:                                                           # hit_run_full_sw, colour space (mapping.c:375-379): no second vector score
        ib = reads[hits["read"], 0]
        recs, ops, strings = ix.sw_full_cs_batch(cn, gst, goff, wl, rw, lens, ib, anchors, revcmpl=revcmpl, threshscore=thresh)
        post_setup(gm, p)
        post, qralign, _ = ix.post_sw_batch(cn, gst, recs, ops, rw, lens, ib)
        qbuf = qralign.buffer; sv = hits["score_vector"]
    else:                                                                # letter space (:386-396): the vector filter again on the turned hit, the full alignment at or above the threshold
        vector_setup(gm, p)
        sv = ix.sw_vector_batch(cn, gst, goff, wl, rw, lens)
        recs, ops, strings = ix.sw_full_ls_batch(cn, gst, goff, wl, rw, lens, anchors=anchors, revcmpl=revcmpl, threshscore=thresh, maxscore=sv)
        recs = recs.copy(); recs["score"][sv < thresh] = 0
    assert (recs["status"] == 0).all()
    maps, map_off = s.select_pass2(hits, hit_off, recs, post)
    want_maps, want_off = restate_pass2(hit_rows(hits), hit_off, recs, rules_of(p), post)
    assert np.array_equal(map_off, want_off) and map_tuples(maps) == want_maps
    flagged = sorted(set(maps["read"][(maps["flags"] & 1) != 0].tolist()))
    if flagged:                                                          # the header's recipe: the posteriors of such a read through the single seam, then the call again
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
        assert not ((maps["flags"] & 1) != 0)[np.isin(maps["read"], flagged)].any()
    k = maps["hit"]; rev = (hits["gen_st"][k] == 1).astype(np.uint8)
    # (the text call takes the records of ONE full call: all of them, the mappings picked out afterwards)
    status, _, _, cigar, edit = ix.sw_full_batch_text(cn, gst, recs, ops, rw, lens, initbp=ib, qralign=qbuf, reverse=(hits["gen_st"] == 1).astype(np.uint8),
                                                      what=("cigar", "edit"), colour_space=colour)
    assert (status == 0).all() and len(rev) == len(k)
    clen = ix.contig_lengths()
    want = sam_records(name, tag or None)
    tied = tie_mask(c["rows"])
    skip = set(c["rows"][tied][:, 0].tolist())                           # reads that own a group of equal windows (stress_60bp only)
    assert len(skip) <= (33 if name == "stress_60bp" else 0)
    text = lambda b: b.decode() if isinstance(b, bytes) else b
    got = []
    for m in maps:
        i = int(m["hit"]); h = hits[i]; r = recs[i]
        if int(m["read"]) in skip: continue
        if h["gen_st"] == 0: pos = int(r["genome_start"]) + 1
        else: pos = (int(clen[h["cn"]]) - int(r["genome_start"])) - (int(r["rmapped"]) - 1 - int(r["deletions"]) + int(r["insertions"]))      # output.c:626-634
        rec = [int(m["read"]), int(h["gen_st"]), int(h["cn"]), pos, int(m["mqv"]), text(cigar(i)), int(m["score_full"]), neglog(m["z0"]), neglog(m["z1"])]
        if extra: rec += [int(h["matches"]), int(h["score_window_gen"]), int(sv[i]), int(r["score"]), text(edit(i))]
        got.append(tuple(rec))
    exp = []
    for w in want:
        if w[0] in skip: continue
        rec = [w[0], w[1], w[2], w[3], w[4], w[5], int(w[6]["AS"]), int(w[6]["Z0"]), int(w[6]["Z1"])]
        if extra: rec += [int(w[6]["ZM"]), int(w[6]["ZR"]), int(w[6]["ZV"]), int(w[6]["ZH"]), w[6]["ZE"]]
        exp.append(tuple(rec))
    assert len(got) == len(exp) and len(exp) > 2000, (len(got), len(exp))
    bad = [i for i in range(len(got)) if got[i] != exp[i]]
    assert not bad, (len(bad), [(got[i], exp[i]) for i in bad[:5]])
    assert {g[0] for g in got} == {e[0] for e in exp}                    # the set of mapped reads
    # the mapping entry on the same session afterwards prints the reference's bytes
    contigs, _, sam = oa.load_golden(name)
    out = s.map_reads_cs(reads) if colour else s.map_reads(reads)
    assert oa.sam_header(contigs) + out == (oa.load_option_sam(name, tag) if tag else sam)


@pytest.mark.gpu
def test_pieces_refusals_and_reuse(gm):
    """a call over three pieces concatenated equals one call; every refusal stands beside a following good call; one session serves selection and mapping calls in turn"""
    name = "stress_60bp"
    ix, s, p, reads = opened(gm, name)
    c = library_pass1(gm, name)
    wins, off, scores, rlen = c["wins"], c["off"], c["scores"], c["rlen"]
    n = len(reads); cuts = [0, 1000, 1777, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi = int(off[2 * a]), int(off[2 * b])
        w = wins[lo:hi].copy(); w["read"] -= a
        h, ho = s.select_pass1(w, off[2 * a:2 * b + 1] - off[2 * a], scores[lo:hi], rlen)
        h = h.copy(); h["read"] += a; h["win"] += lo
        parts.append((h, ho))
    assert np.array_equal(np.concatenate([h for h, _ in parts]), c["hits"])
    assert np.array_equal(np.concatenate([[0]] + [ho[1:].astype(np.int64) + int(c["hit_off"][a]) for (_, ho), a in zip(parts, cuts[:-1])]), c["hit_off"].astype(np.int64))
    contigs, _, sam = oa.load_golden(name)
    assert oa.sam_header(contigs) + s.map_reads(reads) == sam
    # pass-1 refusals
    def refused(call, code, word):
        with pytest.raises(gm.GmError) as e: call()
        assert "(%d)" % code in str(e.value) and word in str(e.value), str(e.value)
    bad_off = off.copy(); bad_off[5], bad_off[6] = off[6] + 1, off[5]
    refused(lambda: s.select_pass1(wins, bad_off, scores, rlen), GM_E_ARG, "ascending")
    short = off.copy(); short[-1] -= 1
    refused(lambda: s.select_pass1(wins, short, scores, rlen), GM_E_ARG, "offsets run")
    for field, value, word in (("read", 7, "says read"), ("st", 1 - int(wins["st"][0]), "says read"), ("cn", len(contigs), "contig"), ("cn", -1, "contig"), ("w_len", 0, "w_len"),
                               ("g_off", 2 ** 31, "beyond contig")):
        w = wins.copy(); w[field][0] = value
        refused(lambda: s.select_pass1(w, off, scores, rlen), GM_E_ARG, word)
    refused(lambda: s.select_pass1(wins, off, scores, 0), GM_E_ARG, "bad arguments")
    h, ho = s.select_pass1(wins, off, scores, rlen)
    assert np.array_equal(h, c["hits"]) and np.array_equal(ho, c["hit_off"])
    p65 = params_of(gm, name, num_tmp_outputs=65)
    s65 = gm.Session(ix, params=p65, max_batch_reads=1024)
    refused(lambda: s65.select_pass1(wins, off, scores, rlen), GM_E_RANGE, "num_tmp_outputs")
    s65.close()
    e, eo = s.select_pass1(wins[:0], np.zeros(1, dtype=np.uint64), scores[:0], rlen)
    assert len(e) == 0 and e.dtype == gm.PASS1_HIT_DTYPE and eo.tolist() == [0]
    # pass-2 refusals
    hits, hit_off = fake_hits([[(0, 0)] * 3, [(1, 1)] * 2])
    recs = fake_recs(gm, [(900, 100 * k, 100, 0, 0) for k in range(5)])
    good, good_off = s.select_pass2(as_hits(gm, hits), hit_off, recs)
    assert good_off.tolist() == [0, 3, 5]
    bo = hit_off.copy(); bo[1] = 6
    refused(lambda: s.select_pass2(as_hits(gm, hits), bo, recs), GM_E_ARG, "ascending")
    for col, value, word in ((0, 1, "says read"), (3, len(contigs), "contig"), (4, 2, "strand"), (9, 0, "score_max")):
        hb = hits.copy(); hb[0, col] = value
        refused(lambda: s.select_pass2(as_hits(gm, hb), hit_off, recs), GM_E_ARG, word)
    many, many_off = fake_hits([[(0, 0)] * 65])
    refused(lambda: s.select_pass2(as_hits(gm, many), many_off, fake_recs(gm, [(900, 100 * k, 100, 0, 0) for k in range(65)])), GM_E_ARG, "65 hits")
    again, again_off = s.select_pass2(as_hits(gm, hits), hit_off, recs)
    assert np.array_equal(again, good) and np.array_equal(again_off, good_off)
    e, eo = s.select_pass2(as_hits(gm, hits[:0]), np.zeros(1, dtype=np.uint64), recs[:0])
    assert len(e) == 0 and e.dtype == gm.MAPPING_DTYPE and eo.tolist() == [0]
    assert oa.sam_header(contigs) + s.map_reads(reads) == sam
    h, ho = s.select_pass1(wins, off, scores, rlen)
    assert np.array_equal(h, c["hits"]) and np.array_equal(ho, c["hit_off"])
