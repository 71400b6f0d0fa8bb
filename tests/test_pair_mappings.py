"""gm_pair_mappings: a chunk of read pairs to mapping arrays in one call (Session.pair_mappings).

Without a GPU: the Python mirrors of gm_pair_mapping_t / gm_pair_mappings_t against a C sizeof / offsetof program; a Python restatement of readpair_pass2's selection
(py_pair_select) held to the reference by replay -- the printed pairs of a golden, fed back as candidates in another order, come out as printed and in the printed order.

With one: table() computes the fields of every SAM record from the arrays, and every record of the paired goldens must come out, field by field and in order, no
pair left out; gm_map_pairs after gm_pair_mappings on one session gives the golden's bytes and, in the other order, the arrays are the same bytes; the pair selection
kernel against the host loop gm_map_pairs runs and against py_pair_select on hand-made candidate lists (gm_debug_pair_select); the mechanics of the call."""
import ctypes as C
import gzip, math, os, re, subprocess, sys, tempfile
import numpy as np
import pytest
from tests import oracle_api as oa

GOLD = os.path.join(oa.ROOT, "tests", "golden")
PAIR_MODES = ["opp-in", "opp-out", "col-fw", "col-bw"]
PE_OPTS = {"pe_nhp": dict(half_paired=0), "pe_n3": dict(match_mode=3), "pe_n3_nhp": dict(match_mode=3, half_paired=0)}
# run id -> (fixture, golden tag or None, gm_params_t fields, gm_pair_opts_t fields, pairs from the front or None)
RUNS = {}
for _m in PAIR_MODES:
    RUNS["pairfix_" + _m] = ("pairfix_" + _m, None, {}, {}, None)
    RUNS["pair_edges_" + _m] = ("pair_edges_" + _m, None, {}, {}, None)
    for _t, _o in PE_OPTS.items(): RUNS["pair_edges_%s@%s" % (_m, _t)] = ("pair_edges_" + _m, _t, {}, _o, None)
RUNS.update({
    "stress_pairs_2x100": ("stress_pairs_2x100", None, {}, {}, None),
    "stress_pairs_2x100@no_half_paired": ("stress_pairs_2x100", "no_half_paired", {}, dict(half_paired=0), None),
    "stress_pairs_2x100@pairs_no_mapq": ("stress_pairs_2x100", "pairs_no_mapq", dict(no_mapping_qualities=1), {}, None),
    "stress_pairs_2x100@geo_w250_n3": ("stress_pairs_2x100", "geo_w250_n3", dict(window_len=250.0), dict(match_mode=3), oa.GEOMETRY_READS["stress_pairs_2x100"]),
    "pair_heap_tandem@ph_o3_strata": ("pair_heap_tandem", "ph_o3_strata", dict(strata=1, num_outputs=3), {}, None),
    "pair_heap_ties@ph_o3_strata": ("pair_heap_ties", "ph_o3_strata", dict(strata=1, num_outputs=3), {}, None),
    "split_pairs_2x60@nhp": ("split_pairs_2x60", "nhp", {}, dict(half_paired=0), None),
    "chimeric_pairs_2x150@chim_single_best": ("chimeric_pairs_2x150", "chim_single_best", dict(single_best_mapping=1), {}, None),
    "chimeric_pairs_2x150@chim_single_best_all": ("chimeric_pairs_2x150", "chim_single_best_all", dict(single_best_mapping=1, all_contigs=1), {}, None),
    "chimeric_pairs_2x150@chim_single_best_all_noimp": ("chimeric_pairs_2x150", "chim_single_best_all_noimp", dict(single_best_mapping=1, all_contigs=1, no_improper_mappings=1), {}, None),
    "cfg5s_2x150_1Mbp@cfg5_no_half_paired": ("cfg5s_2x150_1Mbp", "cfg5_no_half_paired", {}, dict(half_paired=0), None),
    "rna_ls_pairs": ("rna_ls_pairs", None, dict(sam_unaligned=1), {}, None),
    # --extra-sam-fields (with --sam-r2 and a read group, which the fields compared here do not show): ZM ZR ZV ZH and the edit string ZE of every record; opp-in turns
    # mate 2, and half of the pairs map to the reverse strand
    "cfg5s_2x150_1Mbp@pairs_r2_rg_extra": ("cfg5s_2x150_1Mbp", "pairs_r2_rg_extra", dict(sam_r2=1, read_group=b"grp1", extra_sam_fields=1), {}, None),
})
RUN_IDS = sorted(RUNS)
IN_ST = {"opp-in": (0, 1), "opp-out": (1, 0), "col-fw": (0, 0), "col-bw": (1, 1)}      # mates the pair mode reverses (ref: gmapper-defaults.h:184-191)

_FX = {}
def fixture(base):
    """contigs, contig names, the mates with their names, mode and insert bounds of a paired fixture"""
    if base in _FX: return _FX[base]
    if base == "rna_ls_pairs":
        g = oa.load_rna_case(base); (n1, m1, _), (n2, m2, _) = g["reads"]; mode, lo, hi = g["pairing"]
        d = dict(contigs=g["contigs"], contig_names=[bytes(x) for x in g["contig_names"]], m1=m1, m2=m2, names1=n1, names2=n2, mode=mode, ins=(lo, hi))
    elif base == "split_pairs_2x60":
        z = np.load(os.path.join(GOLD, base + ".npz")); lens = z["contig_len"].astype(np.int64); off = np.concatenate([[0], np.cumsum(lens)])
        contigs = np.split(np.ascontiguousarray(z["S"], dtype=np.uint8), off[1:-1])
        d = dict(contigs=contigs, contig_names=[b"contig%d" % (i + 1) for i in range(len(contigs))], m1=z["mates1"], m2=z["mates2"],
                 names1=[bytes(n) + b"/1" for n in z["names"]], names2=[bytes(n) + b"/2" for n in z["names"]], mode=str(z["mode"]), ins=tuple(int(x) for x in z["ins"]))
    else:
        g = oa.load_golden_pairs(base)
        d = {k: g[k] for k in ("contigs", "contig_names", "m1", "m2", "names1", "names2", "mode", "ins")}
    _FX[base] = d
    return d


def golden_text(base, tag):
    with gzip.open(os.path.join(GOLD, base + ("@" + tag if tag else "") + ".sam.gz"), "rb") as f: return f.read()


def qname_of(a, b):
    """QNAME of a pair: the common prefix of the mates' names, minus a trailing ':' or '/' (ref: output.c:365-378)"""
    i = 0
    while i < min(len(a), len(b)) and a[i] == b[i]: i += 1
    if i > 0 and a[i - 1:i] in (b":", b"/"): i -= 1
    return a[:i]


def golden_records(text):
    """qname -> its records in printed order; a record: (FLAG, RNAME, POS, MAPQ, CIGAR, RNEXT, PNEXT, TLEN, the AS / Z* / NM tags as printed)"""
    out = {}; order = []
    for ln in text.split(b"\n"):
        if not ln or ln.startswith(b"@"): continue
        f = ln.split(b"\t")
        tags = tuple(x for x in f[11:] if x[:2] in (b"AS", b"NM") or x[:1] == b"Z")
        if f[0] not in out: out[f[0]] = []; order.append(f[0])
        out[f[0]].append((int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[6], int(f[7]), int(f[8]), tags))
    return out, order


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# readpair_pass2's selection, restated (ref: mapping.c:2181-2314); a window: (cn, gen_st, genome_start, rmapped, deletions, insertions, score_full, score_max, sort_idx)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def pair_threshold(thr, smax):
    return int(-thr) if thr < 0 else int(smax * (thr / 100.0))


def py_pair_select(cands, W, thr=50.0, num_outputs=10, strata=0, max_alignments=0):
    def score(h): return W[0][h[0]][6] + W[1][h[1]][6]
    def key(h):
        smax = W[0][h[0]][7] + W[1][h[1]][7]
        return score(h) if thr < 0 else (1000 * 100 * score(h)) // smax
    v = []
    for a, b in cands:
        if W[0][a][6] == 0 or W[1][b][6] == 0: continue
        if W[0][a][6] + W[1][b][6] >= pair_threshold(thr, W[0][a][7] + W[1][b][7]): v.append([a, b])
    start = lambda w: (w[0], w[1], w[2])
    end = lambda w: (w[0], w[1], -w[2] - w[3] + w[4] - w[5])
    for nip in (0, 1):
        for kf in (start, end):
            v.sort(key=lambda h: kf(W[nip][h[nip]]))                      # (stable)
            i = 0
            while i < len(v):
                j = i + 1
                while j < len(v) and kf(W[nip][v[j][nip]]) == kf(W[nip][v[i][nip]]): j += 1
                mi = i
                for k in range(i + 1, j):
                    if W[nip][v[k][nip]][6] > W[nip][v[mi][nip]][6]: mi = k
                best = v[mi][nip]
                for k in range(i, j): v[k][nip] = best
                i = j
    sidx = lambda h: (W[0][h[0]][8], W[1][h[1]][8])
    v.sort(key=sidx)
    v = [h for k, h in enumerate(v) if k == 0 or sidx(v[k - 1]) != sidx(h)]
    v.sort(key=lambda h: -key(h))
    v = v[:num_outputs]
    if strata and v:
        k = 1
        while k < len(v) and score(v[k]) == score(v[0]): k += 1
        v = v[:k]
    if max_alignments and len(v) > max_alignments: v = []
    return [(a, b) for a, b in v]


def cigar_counts(cig):
    runs = [(int(n), op) for n, op in re.findall(rb"(\d+)([MIDS])", cig)]
    m = sum(n for n, op in runs if op == b"M"); i = sum(n for n, op in runs if op == b"I"); d = sum(n for n, op in runs if op == b"D")
    return m, i, d      # (a CIGAR I is a read letter against a gap: a deletion of the record; a CIGAR D its insertion)


def replay_windows(recs, contig_index, contig_len, in_st):
    """the printed proper pairs of one read pair as windows and candidates; sort_idx: the rank of (read strand, contig, forward position) among the mate's hits"""
    pairs = [(recs[k], recs[k + 1]) for k in range(0, len(recs) - 1, 2) if recs[k][0] & 2]
    W = [[], []]; where = [{}, {}]; cands = []
    for pr in pairs:
        h = []
        for m in (0, 1):
            flag, rname, pos, _, cig, _, _, _, tags = pr[m]
            gen_st = 1 if flag & 16 else 0; M, I, D = cigar_counts(cig); cn = contig_index[rname]
            rmapped = M + I
            gs = pos - 1 if not gen_st else contig_len[cn] - pos - (rmapped - 1 - I + D)
            AS = int(dict(t.split(b":i:") for t in tags)[b"AS"])
            w = (cn, gen_st, gs, rmapped, I, D, AS, 0, (gen_st ^ in_st[m], cn, pos))
            if w not in where[m]: where[m][w] = len(W[m]); W[m].append(w)
            h.append(where[m][w])
        cands.append(tuple(h))
    return W, cands


@pytest.mark.parametrize("base,tag", [("stress_pairs_2x100", None), ("pair_heap_tandem", None), ("pair_heap_ties", None), ("pair_heap_tandem", "ph_o3_strata"),
                                      ("pair_heap_ties", "ph_o3_strata")], ids=lambda x: str(x))
def test_restatement_keeps_the_printed_pairs_in_the_printed_order(base, tag):
    """replay: the proper pairs the reference printed for a read pair, offered as candidates in reverse and in an interleaved order, are all kept (the reference had
    removed every duplicate and dominated window) and come out in the printed order -- under strata and -o 3 as well.  The heap fixtures hold pairs with equal keys and
    windows with equal starts or ends of different pairs."""
    F = fixture(base); recs, order = golden_records(golden_text(base, tag))
    cidx = {n: i for i, n in enumerate(F["contig_names"])}; clen = [len(c) for c in F["contigs"]]
    L = [F["m1"].shape[1], F["m2"].shape[1]]
    kw = dict(num_outputs=3, strata=1) if tag else {}
    n_pairs = n_multi = n_ties = 0
    for q in order:
        W, cands = replay_windows(recs[q], cidx, clen, IN_ST[F["mode"]])
        if not cands: continue
        # score_max = read length x match; sort_idx: the rank of the proxy
        for m in (0, 1):
            ranks = {s: r for r, s in enumerate(sorted(set(w[8] for w in W[m])))}
            W[m] = [w[:7] + (L[m] * 10, ranks[w[8]]) for w in W[m]]
        keys = [(100000 * (W[0][a][6] + W[1][b][6])) // (W[0][a][7] + W[1][b][7]) for a, b in cands]
        n_pairs += 1; n_multi += len(cands) > 1; n_ties += len(set(keys)) < len(keys)
        for scrambled in (cands[::-1], cands[1::2] + cands[0::2]):
            assert py_pair_select(scrambled, W, **kw) == cands, (q, cands, scrambled)
    assert n_pairs > 20 and n_multi > 0
    if base.startswith("pair_heap"): assert n_ties > 0, "the heap fixtures hold pairs of equal keys"


def test_struct_mirrors_against_a_c_program():
    """sizeof and offsetof of every field of gm_pair_mapping_t and gm_pair_mappings_t from a C compiler == the ctypes mirrors (and the numpy dtype)"""
    from shrimp_amd import gmapper as G
    cc = next((c for c in ("cc", "gcc", "clang") if subprocess.run(["sh", "-c", "command -v " + c], capture_output=True).returncode == 0), None)
    assert cc, "no C compiler"
    def fields(name, S): return "".join('  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (name, f[0], name, f[0]) for f in S._fields_)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "gmapper_hip.h"\nint main(void) {\n  printf("gm_pair_mapping_t %zu\\n", sizeof(gm_pair_mapping_t));\n'
           '  printf("gm_pair_mappings_t %zu\\n", sizeof(gm_pair_mappings_t));\n' + fields("gm_pair_mapping_t", G.PairMapping) + fields("gm_pair_mappings_t", G.PairMappingsResult) +
           "  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "m.c"), "w") as f: f.write(src)
        subprocess.run([cc, "-I", os.path.join(oa.ROOT, "include"), os.path.join(d, "m.c"), "-o", os.path.join(d, "m")], check=True)
        out = subprocess.run([os.path.join(d, "m")], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    want = {"gm_pair_mapping_t": C.sizeof(G.PairMapping), "gm_pair_mappings_t": C.sizeof(G.PairMappingsResult)}
    for name, S in (("gm_pair_mapping_t", G.PairMapping), ("gm_pair_mappings_t", G.PairMappingsResult)):
        for f in S._fields_: want["%s.%s" % (name, f[0])] = getattr(S, f[0]).offset
    assert got == want
    assert got["gm_pair_mapping_t"] == 112 == G.PAIR_MAPPING_DTYPE.itemsize
    assert [G.PAIR_MAPPING_DTYPE.fields[f[0]][1] for f in G.PairMapping._fields_] == [getattr(G.PairMapping, f[0]).offset for f in G.PairMapping._fields_]


def test_the_library_exports_the_entry():
    from shrimp_amd import gmapper as G
    L = G.lib()
    for sym in ("gm_pair_mappings", "gm_pair_mappings_free", "gm_pair_mappings_size", "gm_pair_mapping_size", "gm_debug_pair_select"):
        assert hasattr(L, sym) and sym in G.EXPORTS
    assert L.gm_pair_mapping_size() == C.sizeof(G.PairMapping) and L.gm_pair_mappings_size() == C.sizeof(G.PairMappingsResult)
    assert [L.gm_abi_sizeof(k) for k in range(6)] == [C.sizeof(G.Params), C.sizeof(G.PairOpts), C.sizeof(G.MapStats), C.sizeof(G.MergeOptions), C.sizeof(G.SwFullRec), C.sizeof(G.PostRec)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
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


def neglog(v): return int(1000 * -math.log(v))      # double_to_neglog, ref: common/util.h:297-301


def table(pm, pair, names, params):
    """The SAM records of one pair from the arrays, in the order readpair_output prints them (ref: output.c:1236-1291): the paired mappings, mate 1's unpaired ones
    (each with mate 2's unmapped record), mate 2's; for a pair with nothing, the two unaligned records under sam_unaligned.  A record as golden_records parses it."""
    mqv_on = not params.local_alignment and not params.no_mapping_qualities
    ztags = mqv_on and not params.all_contigs
    def hit(m, i):
        h, r = pm.hits[m][i], pm.recs[m][i]
        pos = int(pm.positions(m, [i])[0])
        extra = ()
        if params.extra_sam_fields:      # ref: output.c:729-756
            extra = (b"ZM:i:%d" % h["matches"], b"ZR:i:%d" % h["score_window_gen"], b"ZV:i:%d" % h["score_vector"], b"ZH:i:%d" % r["score"], b"ZE:Z:" + pm.edit(m, i))
        return dict(rname=names[int(h["cn"])], rev=int(h["gen_st"]) == 1, pos=pos, gend=pos + int(r["gmapped"]) - 1, cigar=pm.cigar(m, i),
                    nm=int(r["mismatches"]) + int(r["deletions"]) + int(r["insertions"]), extra=extra)
    def record(m, me, mate, mapq, AS, z, improper):
        flag = 1 | (0 if mate else 8) | (0x20 if mate and mate["rev"] else 0) | (0x40 if m == 0 else 0x80)
        if me is None: return (flag | 4, b"*", 0, 0, b"*", mate["rname"] if mate else b"*", mate["pos"] if mate else 0, 0, ())
        proper = mate is not None and not improper
        flag |= (2 if proper else 0) | (0x10 if me["rev"] else 0)
        rnext, tlen = b"*", 0
        if mate:
            if mate["rname"] == me["rname"]:
                rnext = b"="; tlen = (mate["gend"] if mate["rev"] else mate["pos"] - 1) - (me["gend"] if me["rev"] else me["pos"] - 1)
            else: rnext = mate["rname"]
        tags = [b"AS:i:%d" % AS]
        if ztags: tags += [b"Z%d:i:%d" % (k, neglog(v)) for k, v in zip((2, 3, 4, 6) if proper else (0, 1, 4, 5), z)]
        tags.append(b"NM:i:%d" % me["nm"]); tags += me["extra"]
        return (flag, me["rname"], me["pos"], mapq, me["cigar"], rnext, mate["pos"] if mate else 0, tlen, tuple(tags))
    rows = []
    for k in range(int(pm.pmap_off[pair]), int(pm.pmap_off[pair + 1])):
        e = pm.pmaps[k]; assert int(e["pair"]) == pair
        H = [hit(m, pm.pair_hit(m, k)) for m in (0, 1)]
        for m in (0, 1): rows.append(record(m, H[m], H[1 - m], int(e["mapq"][m]), int(e["as"][m]), e["z"][m], bool(e["improper"])))
    for m in (0, 1):
        for k in range(int(pm.umap_off[m][pair]), int(pm.umap_off[m][pair + 1])):
            u = pm.umaps[m][k]; assert int(u["read"]) == pair
            me = hit(m, int(u["hit"]))
            mapped = record(m, me, None, int(u["mqv"]), int(u["score_full"]), (u["z0"], u["z1"], pm.umap_z45[m][k][0], pm.umap_z45[m][k][1]), False)
            other = record(1 - m, None, me, 0, 0, (), False)
            rows += [mapped, other] if m == 0 else [other, mapped]
    if not rows and params.sam_unaligned: rows = [record(0, None, None, 0, 0, (), False), record(1, None, None, 0, 0, (), False)]
    return rows


def open_run(gm, rid, max_batch_reads=4096):
    base, tag, pf, of, front = RUNS[rid]
    F = fixture(base); p = gm.default_params()
    for k, v in pf.items(): setattr(p, k, v)
    opts = gm.PairOpts.default(F["mode"], F["ins"][0], F["ins"][1])
    for k, v in of.items(): setattr(opts, k, v)
    n = front or len(F["m1"])
    ix = gm.Index(F["contigs"], names=F["contig_names"], params=p); s = gm.Session(ix, params=p, max_batch_reads=max_batch_reads)
    return F, p, opts, n, ix, s


def text_slices_follow_the_mappings(pm, p):
    """a hit that some mapping names has a CIGAR -- and, under extra_sam_fields, an edit string; every other hit has empty slices; without the option there are no
    edit arrays at all.  Returns the hits named, per mate."""
    mapped = [np.zeros(len(pm.hits[m]), dtype=bool) for m in (0, 1)]
    for k in range(len(pm.pmaps)):
        for m in (0, 1): mapped[m][pm.pair_hit(m, k)] = True
    for m in (0, 1):
        mapped[m][pm.umaps[m]["hit"].astype(np.int64)] = True
        assert ((np.diff(pm.cigar_off[m].astype(np.int64)) > 0) == mapped[m]).all()
        if p.extra_sam_fields:
            assert len(pm.edit_off[m]) == len(pm.hits[m]) + 1 and int(pm.edit_off[m][0]) == 0 and int(pm.edit_off[m][-1]) == len(pm.edit_buf[m])
            assert ((np.diff(pm.edit_off[m].astype(np.int64)) > 0) == mapped[m]).all()
        else:
            assert pm.edit_off[m] is None and pm.edit_buf[m] is None
            with pytest.raises(Exception): pm.edit(m, 0)
    return mapped


def check_against_golden(rid, F, p, n, pm):
    """every record of the run's golden, field by field and in order; no pair left out"""
    base, tag = RUNS[rid][:2]
    want, order = golden_records(golden_text(base, tag))
    qn = [qname_of(F["names1"][i], F["names2"][i]) for i in range(n)]
    assert len(set(qn)) == n and set(order) <= set(qn), "the fixture's pairs have distinct names and the golden knows no other"
    n_rec = 0
    for i in range(n):
        rows = table(pm, i, F["contig_names"], p)
        assert rows == want.get(qn[i], []), (rid, i, qn[i], rows, want.get(qn[i], []))
        n_rec += len(rows)
    assert n_rec == sum(len(v) for v in want.values()) and n_rec > 0
    # the layout: offsets ascend to the counts, kinds are 0 then 1 within a pair, a paired mapping names hits of its own pair, hits carry their pair
    for m in (0, 1):
        ho = pm.hit_off[m].astype(np.int64)
        assert ho[0] == 0 and ho[-1] == len(pm.hits[m]) == len(pm.recs[m]) == len(pm.hit_kind[m]) and (np.diff(ho) >= 0).all()
        assert (pm.hits[m]["read"] == np.repeat(np.arange(n), np.diff(ho))).all()
        for i in range(n): assert (np.diff(pm.hit_kind[m][ho[i]:ho[i + 1]].astype(int)) >= 0).all()
        zero = pm.recs[m]["score"] == 0
        assert (pm.recs[m]["n_ops"][zero] == 0).all() and (pm.recs[m]["rmapped"][zero] == 0).all()
        assert int(pm.umap_off[m][-1]) == len(pm.umaps[m]) and len(pm.cigar_off[m]) == len(pm.hits[m]) + 1 and int(pm.cigar_off[m][-1]) == len(pm.cigar_buf[m])
    mapped = text_slices_follow_the_mappings(pm, p)
    assert int(pm.pmap_off[-1]) == len(pm.pmaps)
    for k in range(len(pm.pmaps)):
        e = pm.pmaps[k]; i = int(e["pair"])
        for m in (0, 1):
            a = pm.pair_hit(m, k); assert int(pm.hit_off[m][i]) <= a < int(pm.hit_off[m][i + 1])
            assert int(pm.hit_kind[m][a]) == (1 if e["improper"] else 0)
    return n_rec


@pytest.mark.gpu
@pytest.mark.parametrize("rid", RUN_IDS)
def test_arrays_give_every_record_of_the_reference(gm, rid):
    F, p, opts, n, ix, s = open_run(gm, rid)
    try:
        pm = s.pair_mappings(F["m1"][:n], F["m2"][:n], opts); st = s.stats
    finally:
        s.close(); ix.close()
    n_rec = check_against_golden(rid, F, p, n, pm)
    print(rid, "pairs", n, "records", n_rec, "hits", len(pm.hits[0]), len(pm.hits[1]), "pmaps", len(pm.pmaps), "retries", st["retries"])
    assert st["reads"] == 2 * n


@pytest.mark.gpu
@pytest.mark.parametrize("base", ["pair_edges_" + m for m in PAIR_MODES] + ["stress_pairs_2x100"])
def test_edit_strings_in_every_pair_mode_equal_the_mapping_entry(gm, base):
    """extra_sam_fields in all four pair modes (each turns other mates) and with indels: every record computed from the arrays -- ZM, ZR, ZV,
    ZH and the edit string with it -- equals the record gm_map_pairs prints on the same session (which the reference's goldens of --extra-sam-fields pin elsewhere)"""
    F = fixture(base); p = gm.default_params(); p.extra_sam_fields = 1; p.sam_unaligned = 1
    opts = gm.PairOpts.default(F["mode"], F["ins"][0], F["ins"][1]); n = min(len(F["m1"]), 400)
    ix = gm.Index(F["contigs"], names=F["contig_names"], params=p); s = gm.Session(ix, params=p)
    try:
        pm = s.pair_mappings(F["m1"][:n], F["m2"][:n], opts)
        sam = s.map_pairs(F["m1"][:n], F["m2"][:n], F["names1"][:n], F["names2"][:n], opts=opts)
    finally:
        s.close(); ix.close()
    want, _ = golden_records(sam)
    n_rev = n_edit = n_gap = 0
    for i in range(n):
        rows = table(pm, i, F["contig_names"], p); w = want[qname_of(F["names1"][i], F["names2"][i])]
        assert rows == w, (base, i, rows, w)
        for r in rows:
            ze = [x for x in r[8] if x.startswith(b"ZE:Z:")]
            n_edit += len(ze); n_rev += bool(ze) and bool(r[0] & 16); n_gap += any(b"-" in x or b"(" in x for x in ze)
    assert n_edit > 100 and n_rev > 20, (n_edit, n_rev)
    if base == "stress_pairs_2x100": assert n_gap > 0
    text_slices_follow_the_mappings(pm, p)


def edit_counts(e):
    """(matched letters, substituted letters) an edit string states (ref: common/output.c:36-115): the numbers; the letters outside a '(...)' run of read letters
    against a gap, a '-' standing for a genome letter against one"""
    e = re.sub(rb"\([^)]*\)", b" ", e)
    return sum(int(x) for x in re.findall(rb"\d+", e)), len(re.findall(rb"[A-Za-wyz]", e))


@pytest.mark.gpu
def test_edit_strings_on_rna_agree_with_their_records(gm):
    """RNA reads on RNA contigs (the complement of A is U there) under extra_sam_fields: the edit string of every mapped hit states the matches and mismatches of its
    record -- the record whose NM the reference's golden pins in test_arrays_give_every_record_of_the_reference -- on both strands and for the mate opp-in turns.
    gm_map_pairs is no yardstick here: its host edit string complements a reverse-strand RNA contig with the DNA table and prints a U for every A (on this fixture
    b'ZE:Z:11UU1UU2U...' beside NM:i:0 and AS:i:500 where the arrays give b'ZE:Z:50'); no golden of the reference holds --extra-sam-fields on RNA, and the mapping
    entries are left as they are."""
    F = fixture("rna_ls_pairs"); p = gm.default_params(); p.extra_sam_fields = 1
    opts = gm.PairOpts.default(F["mode"], F["ins"][0], F["ins"][1])
    ix = gm.Index(F["contigs"], names=F["contig_names"], params=p); s = gm.Session(ix, params=p)
    try:
        pm = s.pair_mappings(F["m1"], F["m2"], opts)
    finally:
        s.close(); ix.close()
    mapped = text_slices_follow_the_mappings(pm, p)
    n = [[0, 0], [0, 0]]; n_mis = 0
    for m in (0, 1):
        for i in np.nonzero(mapped[m])[0]:
            r = pm.recs[m][i]
            assert edit_counts(pm.edit(m, i)) == (int(r["matches"]), int(r["mismatches"])), (m, i, pm.edit(m, i), r)
            n[m][int(pm.hits[m]["gen_st"][i])] += 1; n_mis += int(r["mismatches"]) > 0
    assert min(n[0] + n[1]) > 20 and n_mis > 10, (n, n_mis)
    assert any(b"U" in bytes(pm.edit_buf[m]) for m in (0, 1))      # (the fixture's reads hold U: a substituted one is printed as U)


def arrays_of(pm):
    out = [pm.pmaps, pm.pmap_off]
    for m in (0, 1): out += [pm.hits[m], pm.hit_off[m], pm.hit_kind[m], pm.recs[m], pm.umaps[m], pm.umap_off[m], pm.umap_z45[m], np.frombuffer(pm.cigar_buf[m], dtype=np.uint8), pm.cigar_off[m]]
    return [a.tobytes() for a in out]


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["stress_pairs_2x100", "pair_edges_col-fw@pe_nhp"])
def test_beside_the_mapping_entry_on_one_session(gm, rid):
    """gm_map_pairs after gm_pair_mappings on one session prints the golden byte for byte; gm_pair_mappings after gm_map_pairs gives the same bytes in every array"""
    base, tag = RUNS[rid][:2]
    want = b"".join(ln + b"\n" for ln in golden_text(base, tag).split(b"\n") if ln and not ln.startswith(b"@"))
    F, p, opts, n, ix, s = open_run(gm, rid)
    try:
        a = s.pair_mappings(F["m1"], F["m2"], opts)
        sam = s.map_pairs(F["m1"], F["m2"], F["names1"], F["names2"], opts=opts)
        b = s.pair_mappings(F["m1"], F["m2"], opts)
    finally:
        s.close(); ix.close()
    assert sam == want
    assert arrays_of(a) == arrays_of(b)
    check_against_golden(rid, F, p, n, b)


# ---- the pair selection kernel against the host loop and the restatement ---------------------------------------------------------------------------------
def hand_made_cases(rng, thr, smax=1000):
    """[(windows of mate 1, windows of mate 2, candidates)]; thr: the integer threshold at score_max 2 x smax"""
    def win(cn=0, st=0, gs=100, rm=100, d=0, i=0, sf=900, sidx=0): return [cn, st, gs, rm, d, i, sf, smax, sidx]
    def fin(W): return [[w[:8] + [k] for k, w in enumerate(ws)] for ws in W]
    cases = []
    for n in (0, 1, 2, 63, 64):                                             # 0, 1, 2, 63 and 64 candidates of 8 x 8 windows
        W = [[win(cn=int(rng.integers(0, 2)), st=int(rng.integers(0, 2)), gs=int(rng.integers(0, 6)) * 50, rm=100 - int(rng.integers(0, 3)), sf=int(rng.integers(5, 11)) * 100)
              for _ in range(8)] for _ in (0, 1)]
        allp = [(a, b) for a in range(8) for b in range(8)]; rng.shuffle(allp)
        cases.append((fin(W), [tuple(x) for x in allp[:n]]))
    W = [[win(gs=100 * k, sf=800) for k in range(6)] for _ in (0, 1)]       # all keys equal
    cases.append((fin(W), [(a, (a * 5 + 1) % 6) for a in range(6)] + [(a, a) for a in range(6)]))
    W = [[win(gs=500, rm=100 - k, sf=700 + 10 * (k % 3)) for k in range(5)], [win(gs=1000 + 7 * k, sf=900) for k in range(5)]]      # equal starts, other ends
    cases.append((fin(W), [(k, k) for k in range(5)]))
    W = [[win(gs=500, sf=700), win(gs=500, rm=99, sf=800), win(gs=501, rm=99, sf=750)], [win(gs=900, sf=900), win(gs=950, sf=600)]]      # a rewrite makes two candidates one
    cases.append((fin(W), [(0, 0), (1, 0), (2, 0), (0, 1)]))
    for dlt in (-1, 0, 1):                                                  # sums at thr - 1, thr, thr + 1
        W = [[win(sf=thr // 2 + dlt)], [win(sf=thr - thr // 2)]]
        cases.append((fin(W), [(0, 0)]))
    W = [[win(gs=100 * k, sf=s) for k, s in enumerate((900, 900, 900, 850, 800))], [win(gs=100 * k, sf=900) for k in range(5)]]      # a tie at the cut, and beyond it
    cases.append((fin(W), [(k, k) for k in range(5)]))
    for n in (3, 4):                                                        # max_alignments (3) exactly reached, exceeded
        W = [[win(gs=100 * k, sf=900 - k) for k in range(n)], [win(gs=100 * k, sf=900) for k in range(n)]]
        cases.append((fin(W), [(k, k) for k in range(n)]))
    for _ in range(150):                                                    # small value ranges: ties of every kind
        nw = [int(rng.integers(1, 7)), int(rng.integers(1, 7))]
        W = [[win(cn=int(rng.integers(0, 2)), st=int(rng.integers(0, 2)), gs=int(rng.integers(0, 3)) * 10, rm=100 - int(rng.integers(0, 2)), d=int(rng.integers(0, 2)),
                  i=int(rng.integers(0, 2)), sf=int(rng.choice([0, thr // 2 - 1, thr // 2, thr // 2 + 1, 900, 1000]))) for _ in range(nw[m])] for m in (0, 1)]
        W = fin(W)
        for m in (0, 1):
            perm = rng.permutation(nw[m])
            for k, w in enumerate(W[m]): w[8] = int(perm[k])
        allp = [(a, b) for a in range(nw[0]) for b in range(nw[1])]; rng.shuffle(allp)
        cases.append((W, [tuple(x) for x in allp[:int(rng.integers(0, len(allp) + 1))]]))
    return cases


SELECT_SETS = {"default": {}, "absolute": dict(sw_full_threshold=-1000.0), "o1": dict(num_outputs=1), "o3_strata": dict(num_outputs=3, strata=1),
               "max3": dict(max_alignments=3), "o3_strata_max2_abs": dict(num_outputs=3, strata=1, max_alignments=2, sw_full_threshold=-1500.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(SELECT_SETS))
def test_pair_selection_kernel_equals_the_host_loop(gm, which):
    """k_pair_sel_items + k_sel_pair_pass2 == pair_pass2 (the loop gm_map_pairs runs) == py_pair_select on hand-made candidate lists: 0, 1, 2, 63 and 64 candidates,
    all keys equal, equal starts with other ends, a rewrite that makes two candidates one, sums at thr - 1 / thr / thr + 1, a tie at the cut, max_alignments reached and
    exceeded, and 150 drawn lists with ties of every kind -- under a percentage and an absolute threshold, -o 1, --strata, --max-alignments"""
    rng = np.random.default_rng(7)
    p = gm.default_params()
    for k, v in SELECT_SETS[which].items(): setattr(p, k, v)
    thr = pair_threshold(p.sw_full_threshold, 2000)
    cases = hand_made_cases(rng, thr)
    contigs = [rng.integers(0, 4, 3000).astype(np.uint8) for _ in range(2)]
    n = len(cases)
    cnt = [np.array([len(c[0][m]) for c in cases], dtype=np.uint32) for m in (0, 1)]
    wins = [np.array([w for c in cases for w in c[0][m]], dtype=np.int32).reshape(-1, 9) for m in (0, 1)]
    plist = np.zeros((n, 64), dtype=np.uint32); pcnt = np.zeros(n, dtype=np.uint32)
    for k, (W, cands) in enumerate(cases):
        pcnt[k] = len(cands)
        for j, (a, b) in enumerate(cands): plist[k, j] = (a << 8) | b
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    try:
        dev, host = s.debug_pair_select(1, cnt[0], wins[0], cnt[1], wins[1], plist, pcnt)
    finally:
        s.close(); ix.close()
    kw = dict(thr=p.sw_full_threshold, num_outputs=p.num_outputs, strata=p.strata, max_alignments=p.max_alignments)
    n_kept = n_rewritten = 0
    for k, (W, cands) in enumerate(cases):
        want = py_pair_select(cands, W, **kw)
        assert host[k] == want, (which, k, W, cands, host[k], want)
        assert dev[k] == want, (which, k, W, cands, dev[k], want)
        n_kept += len(want); n_rewritten += any(h not in cands for h in py_pair_select(cands, W, thr=p.sw_full_threshold, num_outputs=64))
    assert n_kept > 50 and n_rewritten > 5, (n_kept, n_rewritten)      # (rewritten: before the cuts, a dominance pass put a window into a pair that no candidate had)


# ---- mechanics ----------------------------------------------------------------------------------------------------------------------------------------------------
class env_set:
    def __init__(self, **kv): self.kv = kv
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}; os.environ.update(self.kv)
    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def child_pytest(select, env, expect):
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=dict(os.environ, **env), cwd=oa.ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) == expect, p.stdout[-500:]


SMALL = ["pair_edges_opp-in", "pair_edges_col-bw@pe_nhp", "pair_edges_opp-out@pe_n3"]


@pytest.mark.gpu
@pytest.mark.parametrize("rid", SMALL)
def test_sub_batches_of_64(gm, rid):
    """several sub-batches: offsets and hit indices are the call's, under the pipeline order of the environment (GM_OVERLAP, see the child runs below)"""
    F, p, opts, n, ix, s = open_run(gm, rid, max_batch_reads=64)
    try:
        pm = s.pair_mappings(F["m1"], F["m2"], opts)
    finally:
        s.close(); ix.close()
    assert n > 3 * 64
    check_against_golden(rid, F, p, n, pm)


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", ["0", "1"])
def test_sub_batches_under_both_pipeline_orders(overlap):
    child_pytest("test_sub_batches_of_64", dict(GM_OVERLAP=overlap), len(SMALL))


@pytest.mark.gpu
def test_release_build(gm):
    """the library without the tuning knobs: the golden cases of the small fixtures and the kernel cases in a child interpreter"""
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    child_pytest("test_sub_batches_of_64 or test_pair_selection_kernel_equals_the_host_loop or (test_arrays_give_every_record_of_the_reference and (pair_heap or stress_pairs_2x100))",
                 dict(GM_LIB_PATH=rel), len(SMALL) + len(SELECT_SETS) + 6)


@pytest.mark.gpu
def test_a_capacity_grows_in_mid_call(gm):
    """A window row overflows, the sub-batch is redone from its front with larger rows, and the arrays are the reference's.  stress_pairs_2x100 does that on its own (a
    read-strand with more windows than the 64 a row starts with).  The pairs inside the tandem repeat stay below 64, so their rows start at 8 there (GM_HCAP, a knob of
    the tuning library; not under GM_LIB_PATH)."""
    runs = [("stress_pairs_2x100", {})]
    if not os.environ.get("GM_LIB_PATH"): runs.append(("pair_heap_tandem@ph_o3_strata", dict(GM_HCAP="8")))
    for rid, env in runs:
        with env_set(**env):
            F, p, opts, n, ix, s = open_run(gm, rid)
            try:
                pm = s.pair_mappings(F["m1"], F["m2"], opts); st = s.stats
            finally:
                s.close(); ix.close()
        assert st["retries"] >= 1, (rid, st)
        check_against_golden(rid, F, p, n, pm)


@pytest.mark.gpu
def test_no_pairs_and_pairs_that_do_not_map(gm):
    F, p, opts, n, ix, s = open_run(gm, "pair_edges_opp-in")
    rng = np.random.default_rng(3)
    try:
        e = s.pair_mappings(np.zeros((0, 40), dtype=np.uint8), np.zeros((0, 60), dtype=np.uint8), opts)
        r = s.pair_mappings(rng.integers(0, 4, (70, 40)).astype(np.uint8), rng.integers(0, 4, (70, 60)).astype(np.uint8), opts)
        pm = s.pair_mappings(F["m1"], F["m2"], opts)
    finally:
        s.close(); ix.close()
    assert e.n_pairs == 0 and len(e.pmaps) == 0 and list(e.pmap_off) == [0] and all(list(e.hit_off[m]) == [0] and len(e.hits[m]) == 0 for m in (0, 1))
    assert len(r.pmaps) == 0 and len(r.umaps[0]) == 0 and len(r.umaps[1]) == 0 and list(r.pmap_off) == [0] * 71 and len(r.cigar_buf[0]) == 0
    check_against_golden("pair_edges_opp-in", F, p, n, pm)


def cigar_from_ops(ops, read_start, rmapped, read_len, rev):
    runs = []
    if read_start: runs.append((read_start, "S"))
    for o in bytes(ops).decode():
        c = {"M": "M", "I": "D", "D": "I"}[o]
        if runs and runs[-1][1] == c: runs[-1] = (runs[-1][0] + 1, c)
        else: runs.append((1, c))
    tail = read_len - read_start - rmapped
    if tail: runs.append((tail, "S"))
    if rev: runs = runs[::-1]
    return "".join("%d%s" % r for r in runs).encode()


@pytest.mark.gpu
def test_want_ops_on_and_off(gm):
    """the operations come down only on request; the records point into them either way, and the CIGAR of every mapped hit is the one its operations spell"""
    F, p, opts, n, ix, s = open_run(gm, "stress_pairs_2x100")
    try:
        a = s.pair_mappings(F["m1"][:300], F["m2"][:300], opts, want_ops=True)
        b = s.pair_mappings(F["m1"][:300], F["m2"][:300], opts)
    finally:
        s.close(); ix.close()
    assert arrays_of(a) == arrays_of(b) and b.ops == [None, None]
    n_indel = 0
    for m in (0, 1):
        r = a.recs[m]; L = (F["m1"], F["m2"])[m].shape[1]
        assert len(a.ops[m]) == int(r["n_ops"].sum()) and (r["ops_off"] == np.concatenate([[0], np.cumsum(r["n_ops"])[:-1]])).all()
        for i in range(len(r)):
            cig = a.cigar(m, i)
            if not cig: continue
            ops = a.ops[m][int(r["ops_off"][i]):int(r["ops_off"][i]) + int(r["n_ops"][i])]
            assert cig == cigar_from_ops(ops, int(r["read_start"][i]), int(r["rmapped"][i]), L, int(a.hits[m]["gen_st"][i]) == 1), (m, i)
            n_indel += (b"I" in cig) or (b"D" in cig)
    assert n_indel > 0


@pytest.mark.gpu
def test_every_refusal_leaves_the_session_usable(gm):
    """every refusal, then a good call on the SAME session: gm_pair_mappings itself where the session's parameters admit one; where they are what was refused, the mapping
    entry -- against a fresh session of the same parameters, or (colour space) against the reference's golden.  A window beyond pass 2's LDS admits no mapping call at
    all: there gm_map_pairs must give the same refusal, made by the same function."""
    G = gm; F = fixture("pair_edges_opp-in"); E_ARG, E_RANGE = -2, -4
    def pairs_text(s, X, p):
        opts = G.PairOpts.default(X["mode"], *X["ins"])
        return (s.map_pairs_cs if p.colour_space else s.map_pairs)(X["m1"], X["m2"], X["names1"], X["names2"], opts=opts)
    def refused(params, opts_fields, m1, m2, code, word, then="pair_mappings"):
        cs = params.pop("cs", False)
        X = fixture("pair_edges_cs_opp-in") if cs else F      # (the colour-space fixture's own contigs and mates for the call that follows)
        p = G.default_params_cs() if cs else G.default_params()
        for k, v in params.items(): setattr(p, k, v)
        opts = G.PairOpts.default(F["mode"], *F["ins"])
        for k, v in opts_fields.items(): setattr(opts, k, v)
        ip = G.default_params_cs() if cs else G.default_params()      # (the index under the defaults: the session's parameters are what is refused)
        ix = G.Index(X["contigs"], names=X["contig_names"], params=ip); s = G.Session(ix, params=p)
        try:
            with pytest.raises(G.GmError) as e: s.pair_mappings(m1, m2, opts)
            assert word in str(e.value) and "(%d)" % code in str(e.value), str(e.value)
            if then == "pair_mappings":
                pm = s.pair_mappings(F["m1"], F["m2"], G.PairOpts.default(F["mode"], *F["ins"]))
                check_against_golden("pair_edges_opp-in", F, p, len(F["m1"]), pm)
            elif then == "golden":
                got = pairs_text(s, X, p)
                want = b"".join(ln + b"\n" for ln in golden_text("pair_edges_cs_opp-in", None).split(b"\n") if ln and not ln.startswith(b"@"))
                assert got == want
            elif then == "fresh":
                got = pairs_text(s, X, p)
                s2 = G.Session(ix, params=p)
                try: want = pairs_text(s2, X, p)
                finally: s2.close()
                assert got == want and got.count(b"\n") > 300
            else:
                with pytest.raises(G.GmError) as e2: pairs_text(s, X, p)
                assert word in str(e2.value) and "(%d)" % code in str(e2.value), str(e2.value)
        finally:
            s.close(); ix.close()
    refused(dict(cs=True, sam_unaligned=1), {}, F["m1"], F["m2"], E_ARG, "colour-space", then="golden")
    refused(dict(output_format=1), {}, F["m1"], F["m2"], E_ARG, "output_format", then="fresh")
    refused(dict(output_format=2), {}, F["m1"], F["m2"], E_ARG, "output_format", then="fresh")
    refused({}, dict(match_mode=2), F["m1"], F["m2"], E_ARG, "match_mode")
    refused({}, dict(match_mode=7), F["m1"], F["m2"], E_ARG, "match_mode")
    refused({}, dict(pair_mode=9), F["m1"], F["m2"], E_ARG, "pair_mode")
    refused(dict(num_tmp_outputs=65), {}, F["m1"], F["m2"], E_RANGE, "num_tmp_outputs", then="fresh")
    refused({}, {}, np.zeros((2, 1001), dtype=np.uint8), F["m2"][:2], E_RANGE, "read length")
    refused({}, {}, F["m1"][:2], np.zeros((2, 1001), dtype=np.uint8), E_RANGE, "read length")
    refused(dict(window_len=-3400.0), {}, F["m1"], F["m2"], E_RANGE, "window length 3400", then="the same refusal")
