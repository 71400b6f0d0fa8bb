"""Reads of 128 to 1 000 bases and colours: the lengths at which the kernels of the mapping path change shape -- the stripes of the vector filter (128 / 129), the carry rows
of pass 1 in LDS and the end of the bucket lookup kernel (183 / 184), the three colour-space pass-2 kernels (204 / 205 and LONG_CS_G4_LAST / + 1), K2's register sort and
k_prune's bins on reads with thousands of lists, pairs with mates of several hundred bases and of different lengths.  The fixtures are the reference's output on one
repeat-rich genome (tools/make_golden.py --long-only; tests/oracle_api.py LONG_INPUTS, LONG_CASES).

Without a GPU: the oracle gives every golden byte for byte, every fixture holds what LONG_MIN asks for, the oracle with its vector filter cut to 128 rows or its anchor
lists cut to 1 024 entries misses the goldens that are there for it, and the size functions that pick the pass-2 kernel are held to the C header.  With one: map_reads /
map_reads_cs / map_pairs give the goldens' bytes, header included, through the kernels the tables name, under the forced variants, in sub-batches and on a session that
changes length; the seams agree with their chains; what cannot run is refused before anything is uploaded."""
import os, re, subprocess, sys
import numpy as np
import pytest
from tests import oracle_api as oa

GOLD = os.path.join(oa.ROOT, "tests", "golden")
TAGS = sorted(oa.LONG_CASES)
GM_E_RANGE = -4


def _first_diff(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y: return i, x[:300], y[:300]
    return min(len(la), len(lb)), len(la), len(lb)


def kind_of(tag): return oa.LONG_INPUTS[tag.split(":")[0]]["kind"]
def is_cs(tag): return kind_of(tag).startswith("cs")
def is_pairs(tag): return kind_of(tag).endswith("pairs")


_in = {}
def inputs(name):
    if name not in _in: _in[name] = oa.load_long_input(name)
    return _in[name]


def oracle_sam(tag, more_opts=""):
    """the oracle's SAM text of a case, header included; more_opts: options behind the case's own"""
    name, _, opts, _, _ = oa.LONG_CASES[tag]; g = inputs(name)
    opts = ";".join(x for x in ("colour=1" if is_cs(tag) else "", opts, more_opts) if x)
    o = oa.Session(g["contigs"], g["contig_names"], opts=opts)
    try:
        o.set(True, True)
        if is_pairs(tag):
            o.set_pairing(g["mode"], *g["ins"])
            body = o.map_pairs_sam(g["m1"], g["m2"], g["names1"], g["names2"], nthreads=4)
        elif "quals" in g: body = o.map_sam_q(g["reads"], g["quals"], g["qual_delta"], nthreads=4)
        else: body = o.map_sam(g["reads"], nthreads=4)
    finally: o.close()
    return oa.sam_header(g["contigs"], g["contig_names"]) + body


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# (reads with a mapped record, reads with more than one, records, records on the reverse strand, records with an I or a D[, proper pairs, half-paired or unpaired records]):
# as the generator printed them
COUNTS = {
    "ls_128:default": (200, 77, 812, 425, 524),
    "ls_129:default": (200, 88, 907, 405, 516),
    "ls_129:local": (200, 88, 907, 405, 497),
    "ls_129:extra": (200, 88, 907, 405, 516),
    "ls_183:default": (200, 98, 958, 525, 736),
    "ls_184:default": (200, 91, 928, 525, 720),
    "ls_184:n1": (200, 91, 928, 525, 720),
    "ls_256:default": (200, 88, 878, 483, 739),
    "ls_257:default": (200, 81, 852, 447, 754),
    "ls_257:w16H": (200, 81, 851, 447, 753),
    "ls_257:extra": (200, 81, 852, 447, 754),
    "ls_385:default": (100, 44, 467, 238, 463),
    "ls_400:default": (100, 47, 468, 224, 445),
    "ls_400:local": (100, 47, 471, 224, 433),
    "ls_400:n1": (100, 47, 468, 224, 445),
    "ls_400:o5_strata": (100, 2, 108, 49, 99),
    "ls_700:default": (59, 28, 285, 180, 275),
    "ls_700:extra": (59, 28, 285, 180, 275),
    "ls_1000:default": (40, 13, 132, 75, 132),
    "ls_1000:local": (40, 15, 149, 77, 149),
    "ls_1000:w16H": (40, 13, 132, 75, 132),
    "ls_1000:w110": (40, 13, 132, 75, 132),
    "cs_129:default": (200, 88, 881, 509, 874),
    "cs_129:local": (200, 88, 888, 513, 855),
    "cs_204:default": (200, 87, 907, 408, 898),
    "cs_204:unit": (200, 87, 911, 409, 897),
    "cs_205:default": (200, 76, 799, 380, 792),
    "cs_205:unit": (200, 79, 821, 397, 807),
    "cs_400:default": (100, 38, 389, 175, 389),
    "cs_400:local": (100, 41, 414, 193, 405),
    "cs_400:ungapped": (98, 33, 324, 143, 265),
    "cs_556:default": (100, 39, 388, 176, 388),
    "cs_557:default": (100, 43, 433, 204, 432),
    "cs_1000:default": (30, 7, 74, 31, 74),
    "ls_400q:fq": (100, 39, 397, 255, 393),
    "cs_200q:csfq": (199, 92, 917, 444, 914),
    "cs_555:local": (60, 22, 229, 93, 226),
    "pairs_2x250_opp-in:default": (200, 108, 1013, 488, 879, 97, 309),
    "pairs_2x250_opp-in:nhp": (194, 66, 704, 352, 602, 97, 0),
    "pairs_2x250_opp-in:n3": (200, 150, 1355, 664, 1213, 97, 575),
    "pairs_400_100_col-fw:default": (199, 148, 1455, 697, 1227, 98, 561),
    "pairs_400_100_col-fw:nhp": (196, 90, 882, 398, 708, 98, 0),
    "pairs_400_100_col-bw:default": (200, 149, 1429, 739, 1168, 99, 655),
    "pairs_400_100_col-bw:nhp": (182, 80, 744, 360, 582, 91, 0),
    "pairs_2x250_opp-out:default": (200, 109, 1013, 517, 917, 97, 503),
    "pairs_2x250_opp-out:nhp": (194, 46, 510, 255, 452, 97, 0),
    "pairs_2x700_opp-in:default": (80, 51, 387, 186, 387, 39, 195),
    "pairs_2x700_opp-in:nhp": (78, 14, 192, 96, 192, 39, 0),
    "cs_pairs_2x150_opp-in:default": (200, 100, 895, 437, 661, 98, 325),
    "cs_pairs_2x150_opp-in:nhp": (196, 52, 570, 285, 380, 98, 0),
}


def test_the_tables_name_every_fixture_and_the_computed_limits():
    assert len(TAGS) == 50 and sorted(COUNTS) == TAGS
    # the two sides of the four-window / one-window limit of colour-space pass 2 and the last length colour-space --local is admitted at, from gm_pass2_cs_lds and
    # GM_SWF_LDS_LIMIT at windows of 140 % (the same figures from the C header: test_size_functions_equal_the_header)
    assert (oa.LONG_CS_G4_LAST, oa.LONG_CS_G4_LAST + 1, oa.LONG_CS_LOCAL_LAST) == (556, 557, 555)
    for L in (129, 204, 205, 400, 555, 556, 557, 1000): assert "cs_%d" % L in oa.LONG_INPUTS
    for L in (128, 129, 183, 184, 256, 257, 385, 400, 700, 1000): assert "ls_%d" % L in oa.LONG_INPUTS
    files = sorted(f for f in os.listdir(GOLD) if f.startswith("long_"))
    assert files == sorted([oa.long_file(t) for t in TAGS] + ["long_%s.npz" % n for n in oa.LONG_INPUTS] + ["long_genome.npz"])
    for f in files: assert os.path.getsize(os.path.join(GOLD, f)) <= 200_000, f
    contigs, rep = oa.load_long_genome()
    assert 140_000 <= sum(len(c) for c in contigs) <= 160_000 and len(contigs) == 2 and 20_000 <= rep[1] - rep[0] <= 30_000
    assert int((contigs[0] == 15).sum()) == 200 and int((contigs[1] > 3).sum()) == 0


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_holds_what_it_is_there_for(tag):
    """LONG_MIN on the committed files: 90 % of the reads mapped, 10 % with more than one record, 30 % of the records on the reverse strand, half with an indel; pairs:
    60 % properly paired and, with half-paired mappings allowed, 5 % of the records half-paired or unpaired (LONG_NO_INDELS / LONG_NO_MULTI: what -U and --strata rule out)"""
    inp = oa.LONG_INPUTS[tag.split(":")[0]]; body = oa.load_long_sam(tag)
    c = oa.long_counts(body, inp["n"], is_pairs(tag))
    got = (c["mapped"], c["multi"], c["records"], c["reverse"], c["indel"]) + ((c["proper"], c["loose"]) if is_pairs(tag) else ())
    print(tag, got)
    assert oa.long_conditions(tag, c) == [] and got == COUNTS[tag]
    g = inputs(tag.split(":")[0])
    assert body.startswith(oa.sam_header(g["contigs"], g["contig_names"])) and b"@PG" not in body
    if is_pairs(tag): assert g["m1"].shape == (inp["n"], inp["len"][0] + is_cs(tag)) and g["m2"].shape == (inp["n"], inp["len"][1] + is_cs(tag))
    else: assert g["reads"].shape == (inp["n"], inp["len"] + is_cs(tag))
    unmapped = sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@") and int(l.split(b"\t")[1]) & 4)
    if not is_pairs(tag): assert unmapped == c["reads"] - c["mapped"]      # --sam-unaligned: no read is left out of a golden (a half-paired record brings its mate's unmapped one)
    names = {l.split(b"\t")[0] for l in body.split(b"\n") if l and not l.startswith(b"@")}
    assert len(names) == inp["n"]


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_equals_the_reference_on_the_long_goldens(oracle_lib, tag):
    got, want = oracle_sam(tag), oa.load_long_sam(tag)
    assert got == want, _first_diff(got, want)


# ---- negative controls -------------------------------------------------------------------------------------------------------------------------------------------
# every default golden of unpaired reads above 128 bases or colours -- but at 129 the one with --extra-sam-fields: a filter that loses the 129th position alone moves a
# window's score by one match at the most, which no record of the two default goldens at 129 shows; the ZV field (the vector filter's score) does
ROWS_TAGS = [t for t in TAGS if t.endswith(":default") and not is_pairs(t) and oa.LONG_INPUTS[t.split(":")[0]]["len"] > 129] + ["ls_129:extra"]


@pytest.mark.parametrize("tag", ROWS_TAGS)
def test_oracle_with_the_vector_filter_cut_to_128_rows_misses_the_golden(oracle_lib, tag):
    """what a vector filter that stopped after its first stripe of 128 read positions would print: a window's score ends at 1 280, below the threshold of half the read's
    score from 257 bases on, and below the scores pass 1 orders the windows by from 129"""
    got, want = oracle_sam(tag, "test-vector-rows=128"), oa.load_long_sam(tag)
    assert got != want and oa.sam_distance(want, got) >= 5, oa.sam_distance(want, got)


def test_the_cut_to_128_rows_changes_nothing_at_128_bases_and_no_record_of_the_default_goldens_at_129(oracle_lib):
    for tag in ("ls_128:default", "ls_129:default", "cs_129:default"):
        assert oracle_sam(tag, "test-vector-rows=128") == oa.load_long_sam(tag), tag


CAP_TAGS = ["ls_400:default", "ls_700:default", "ls_1000:default", "cs_1000:default", "ls_400:n1", "pairs_2x700_opp-in:default"]


def test_oracle_with_the_anchor_lists_cut_misses_goldens_at_512_entries_and_none_at_1024(oracle_lib):
    """an anchor list cut behind its first 1 024 entries a read-strand reproduces every golden: on this genome no list is that long, at any length up to 1 000 bases -- the
    9-mer tandem gives a read some 300 diagonals, the repeat family nine.  Cut behind 512 entries the 1 000-base golden is missed (10 records), behind 256 the -n 1 golden
    at 400 bases too: lists of more than 512 entries exist and decide records, lists of more than 1 024 are not covered by these fixtures."""
    for t in CAP_TAGS: assert oracle_sam(t, "test-anchor-cap=1024") == oa.load_long_sam(t), t
    assert oa.sam_distance(oa.load_long_sam("ls_1000:default"), oracle_sam("ls_1000:default", "test-anchor-cap=512")) == 10
    assert oa.sam_distance(oa.load_long_sam("ls_400:n1"), oracle_sam("ls_400:n1", "test-anchor-cap=256")) == 20


# ---- the size functions --------------------------------------------------------------------------------------------------------------------------------------------
SIZE_LENGTHS = [60, 100, 128, 129, 183, 184, 204, 205, 256, 257, 385, 400, 555, 556, 557, 592, 593, 700, 1000]


def test_size_functions_equal_the_header(tmp_path):
    """gm_pass2_g4_lds, gm_pass2_cs_lds and gm_pass2_max_window as tests/oracle_api.py restates them == shrimp_amd/csrc/gm_pass2_sizes.h through tests/host/pass2_sizes_main.cpp,
    at the lengths of the fixtures; and the kernel each colour-space length must get"""
    exe = str(tmp_path / "pass2_sizes_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(oa.ROOT, "shrimp_amd", "csrc"), "-o", exe, os.path.join(oa.ROOT, "tests", "host", "pass2_sizes_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    p = subprocess.run([exe] + [str(L) for L in SIZE_LENGTHS], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().split("\n")
    assert lines[0] == "limit %d" % oa.GM_SWF_LDS_LIMIT and len(lines) == 1 + len(SIZE_LENGTHS)
    for L, line in zip(SIZE_LENGTHS, lines[1:]):
        W = oa.default_window(L)
        want = "%d %d g4 %d %d cs %d %d %d max %d %d %d" % (L, W, oa.gm_pass2_g4_lds(4, L, W), oa.gm_pass2_g4_lds(8, L, W), oa.gm_pass2_cs_lds(1, L, W), oa.gm_pass2_cs_lds(4, L, W),
                                                          oa.gm_pass2_cs_lds(8, L, W), oa.gm_pass2_max_window(0, 0, L), oa.gm_pass2_max_window(1, 0, L), oa.gm_pass2_max_window(1, 1, L))
        assert line == want, (line, want)
    assert [oa.pass2_kernel(True, L) for L in (100, 129, 204, 205, 400, 556, 557, 1000)] == ["k_pass2_cs_g4<8,int16_t>"] + ["k_pass2_cs_g4<16,int>"] * 5 + ["k_pass2_cs"] * 2
    # (at the default scores a move changes the score by 60 at the most and `reach` passes 16 000 at 112 colours: the 64 KB of the eight-window kernel decide only under
    # smaller scores -- at unit scores between 204 and 205 colours)
    assert [oa.pass2_kernel(True, L, big=3) for L in (129, 204, 205)] == ["k_pass2_cs_g4<8,int16_t>"] * 2 + ["k_pass2_cs_g4<16,int>"]
    assert oa.gm_pass2_max_window(1, 1, 60) == 829 and oa.gm_pass2_max_window(1, 0, 60) == 3335 and oa.gm_pass2_max_window(0, 0, 100) == 3140      # (the limits tests/test_window_geometry.py names)


# ---- the windows driver ------------------------------------------------------------------------------------------------------------------------------------------
import ctypes as C
from tests import test_read_windows as trw

driver = trw.driver                                                      # (the fixture: tests/read_windows_oracle.cpp, compiled once for this module)
_drv = {}


def driver_rows(L, name):
    """(rows, off) of the windows driver on a letter-space input under the default options, computed once"""
    if name not in _drv:
        g = inputs(name); cs = [np.ascontiguousarray(c, dtype=np.uint8) for c in g["contigs"]]; reads = np.ascontiguousarray(g["reads"], dtype=np.uint8); u8p = C.POINTER(C.c_uint8)
        h = L.rwo_create(len(cs), (u8p * len(cs))(*[c.ctypes.data_as(u8p) for c in cs]), (C.c_uint64 * len(cs))(*[len(c) for c in cs]), 0, 2)
        cap = 256 * len(reads)
        for _ in range(2):
            rows = np.zeros((cap, 12), dtype=np.int64)
            w = L.rwo_windows(h, reads.shape[0], reads.shape[1], reads.ctypes.data_as(u8p), trw.THREADS, rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
            if w <= cap: break
            cap = int(w)
        L.rwo_destroy(h)
        assert 0 < w <= cap
        _drv[name] = (rows[:w].copy(), trw.offsets(rows[:w], len(reads)))
    return _drv[name]


@pytest.mark.parametrize("name", ["ls_129", "ls_257", "ls_700"])
def test_driver_windows_carry_zm_zr_zv_of_the_extra_field_goldens(driver, oracle_lib, name):
    """every mapped record of the --extra-sam-fields goldens has a driver window of its read and strand that covers the alignment and carries its ZM and ZR; the oracle's
    vector score at the header's address of one such window is its ZV"""
    g = inputs(name); contigs, reads = g["contigs"], g["reads"]
    rows, off = driver_rows(driver, name)
    assert trw.in_list_order(rows)
    recs = trw.records("long_%s@extra" % name)
    assert len(recs) == COUNTS[name + ":extra"][2]
    cands = trw.candidates(rows, off, recs)
    clen = np.array([len(c) for c in contigs], dtype=np.int64)
    ls = {c: [trw.pack(x) for x in (contigs[c], trw.CMPL[contigs[c][::-1]])] for c in (0, 1)}
    rw = [trw.pack(r) for r in reads]; rlen = reads.shape[1]
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def scores_of(idx, rd):
        st, goff = trw.header_address(rows[idx], clen)
        return np.array([oracle_lib.gmo_sw_vector(u32(ls[int(rows[i, 2])][st[k]]), int(goff[k]), int(rows[i, 4]), u32(rw[r]), rlen) for k, (i, r) in enumerate(zip(idx, rd))], dtype=np.int64)
    trw.some_candidate_gives_zv(recs, cands, scores_of)


# What gm_last_lookup_kernel() must name for the unpaired inputs: (colour space, set, length) -> kernel, recorded from k1_plan (gm_lookup_plan.h) through the query mode of
# tests/host/lookup_plan_main.cpp on the 148 323 bases of the long genome; test_the_lookup_table_is_the_plans keeps it there.  Every other unpaired case: k_lookup_v3.
LOOKUP_KERNEL = {"ls_128": "k_lookup_bkt", "ls_129": "k_lookup_bkt", "ls_183": "k_lookup_bkt", "cs_129": "k_lookup_bkt"}
DEFAULT_SEEDS = ["11110111101111", "1111011100100001111", "1111000011001101111"]


def lookup_kernel(tag):
    name, st = tag.split(":")
    return "k_lookup" if st == "n1" else LOOKUP_KERNEL.get(name, "k_lookup_v3")      # (-n 1, no region counts: the slab sweep)


def test_the_lookup_table_is_the_plans(tmp_path):
    exe = str(tmp_path / "lookup_plan_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(oa.ROOT, "shrimp_amd", "csrc"), "-o", exe, os.path.join(oa.ROOT, "tests", "host", "lookup_plan_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    total = sum(len(c) for c in oa.load_long_genome()[0]); seen = set()
    for tag in TAGS:
        if is_pairs(tag): continue
        name, st = tag.split(":"); inp = oa.LONG_INPUTS[name]; seeds = oa.LONG_CASES[tag][4] or DEFAULT_SEEDS
        p = subprocess.run([exe, "query", str(total), str(int(is_cs(tag))), str(int(st == "w16H")), str(inp["len"]), str(inp["n"]), "8" if st == "n1" else "0", "-", ",".join(seeds)],
                           capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout.split(" | ")[0] == lookup_kernel(tag), (tag, p.stdout)
        seen.add(p.stdout.split(" | ")[0])
    assert seen == {"k_lookup_bkt", "k_lookup_v3", "k_lookup"}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
from tests.test_pair_edges import env_set                               # environment variables for the length of a block


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
    for ix in _index.values(): ix.close()
    _index.clear()


_index = {}
def index_of(gm, tag):
    """the index of a case: one a space and seed set, on the one genome"""
    seeds = oa.LONG_CASES[tag][4]; key = (is_cs(tag), tuple(seeds or ()))
    if key not in _index:
        contigs = oa.load_long_genome()[0]; p = gm.default_params_cs() if is_cs(tag) else gm.default_params()
        if seeds: p.hash_seeds = 1
        _index[key] = gm.Index(contigs, names=[b"contig1", b"contig2"], seeds=seeds, params=p)
    return _index[key]


def params_of(gm, tag, **more):
    """(gm_params_t, gm_pair_opts_t fields) of a case"""
    fields = oa.LONG_CASES[tag][3]
    p = gm.default_params_cs() if is_cs(tag) else gm.default_params()
    for k, v in dict(fields, **more).items():
        if not k.startswith("pair_"): setattr(p, k, v)
    p.sam_unaligned = 1
    return p, {k[5:]: v for k, v in fields.items() if k.startswith("pair_")}


def map_on(gm, s, tag, n=None, pick=None):
    """the SAM text of a case on the session s (its first n reads or pairs; pick: these reads or pairs of it, under their own names), header included"""
    g = inputs(tag.split(":")[0]); _, pair_fields = params_of(gm, tag)
    if pick is not None:
        if is_pairs(tag): g = dict(g, m1=g["m1"][pick], m2=g["m2"][pick], names1=[g["names1"][i] for i in pick], names2=[g["names2"][i] for i in pick])
        else: g = dict(g, reads=g["reads"][pick], names=[b"r%d" % i for i in pick])
    if is_pairs(tag):
        opts = gm.PairOpts.default(g["mode"], g["ins"][0], g["ins"][1])
        for k, v in pair_fields.items(): setattr(opts, k, v)
        body = (s.map_pairs_cs if is_cs(tag) else s.map_pairs)(g["m1"][:n], g["m2"][:n], g["names1"][:n], g["names2"][:n], opts=opts)
    elif "quals" in g: body = (s.map_reads_cs_fastq if is_cs(tag) else s.map_reads_fastq)(g["reads"][:n], g["quals"][:n], g["qual_delta"])
    else: body = (s.map_reads_cs if is_cs(tag) else s.map_reads)(g["reads"][:n], names=g.get("names"))
    return index_of(gm, tag).sam_header() + body


def map_case(gm, tag, max_batch_reads=None, pick=None):
    """a case through map_reads / map_reads_cs / map_pairs on a fresh session no larger than its reads: (SAM text, stats, lookup kernel, pass-2 kernel)"""
    p, _ = params_of(gm, tag); n = oa.LONG_INPUTS[tag.split(":")[0]]["n"]
    s = gm.Session(index_of(gm, tag), params=p, max_batch_reads=max_batch_reads or max(64, n))
    try:
        got = map_on(gm, s, tag, pick=pick)
        return got, dict(s.stats, sub_batches=s.lookup_timing()[2]), gm.lib().gm_last_lookup_kernel().decode(), gm.lib().gm_last_pass2_kernel().decode()
    finally: s.close()


def pass2_kernel(tag):
    """what gm_last_pass2_kernel() must name after a case: the last pass 2 of a call is that of its last mate or read length"""
    inp = oa.LONG_INPUTS[tag.split(":")[0]]; L = inp["len"][1] if is_pairs(tag) else inp["len"]
    return oa.pass2_kernel(is_cs(tag), L, local="local" in tag, big=3 if tag.endswith(":unit") else None)


# the cases the front's prune kernel has no LDS for (pass2_front_prune_lds: 3 932 lists a read-strand under the weight-16 -H set at 1 000 bases give a survivor capacity of
# 16 384 and a table of 256 KB): refused before anything is uploaded, held to the oracle alone -- open against the reference
REFUSED_TAGS = ["ls_1000:w16H"]
RELEASE_TAGS = ["ls_129:default", "ls_257:default", "ls_1000:default", "cs_557:default", "cs_555:local", "pairs_400_100_col-bw:nhp"]
MAP_TAGS = RELEASE_TAGS if os.environ.get("GM_LONG_RELEASE_CASES") else [t for t in TAGS if t not in REFUSED_TAGS]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", MAP_TAGS)
def test_map_equals_the_reference_golden(gm, tag):
    """map_reads, map_reads_cs and map_pairs == the reference's SAM text, header included, byte for byte; through the lookup kernel the plan names (unpaired cases) and the
    pass-2 kernel the size functions name"""
    got, st, k1, p2 = map_case(gm, tag); want = oa.load_long_sam(tag)
    print(tag, k1, p2)
    assert got == want, (_first_diff(got, want), st)
    assert p2 == pass2_kernel(tag), (p2, pass2_kernel(tag))
    if not is_pairs(tag) and not os.environ.get("GM_LONG_RELEASE_CASES"): assert k1 == lookup_kernel(tag), (k1, lookup_kernel(tag))


@pytest.mark.gpu
def test_release_build_reproduces_six_long_goldens():
    """`make release` (the build bench.py measures): six cases in a child interpreter with GM_LIB_PATH on libgmapper_hip_release.so"""
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    env = dict(os.environ, GM_LIB_PATH=rel, GM_LONG_RELEASE_CASES="1")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "test_map_equals_the_reference_golden", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=env, cwd=oa.ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) == len(RELEASE_TAGS), p.stdout[-500:]


# ---- variants ------------------------------------------------------------------------------------------------------------------------------------------------------
VARIANT_TAGS = ["ls_257:default", "ls_400:default", "ls_1000:default", "cs_400:default"]
# knobs of the tuning build -> the lookup kernel they must lead to on these cases (None: the plan's own), as the plan's query mode names it for each of them: the slab
# sweep and v3 run where they are forced; v4 needs more than one slab, the plan declines it on this index and names v3.  (A forced v5: the test behind this one.)  (GM_OVERLAP=0 changes nothing in a call of one sub-batch: test_three_sub_batches_under_both_pipeline_orders has it.)
VARIANTS = {
    "heavy_tier": (dict(GM_SCAP="256", GM_SCAP2="64"), None),
    "no_prune": (dict(GM_NO_PRUNE="1"), None),
    "slabs_of_2^17": (dict(GM_SLAB_BITS="17"), None),
    "sweep_forced": (dict(GM_K1_V2="1"), "k_lookup"),
    "v3_forced": (dict(GM_K1_V3="1"), "k_lookup_v3"),
    "v4_forced_and_declined": (dict(GM_K1_V4="1"), "k_lookup_v3"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("tag", VARIANT_TAGS)
def test_variants_give_the_same_bytes(gm, tag, variant):
    env, kern = VARIANTS[variant]; want = oa.load_long_sam(tag)
    with env_set(**env):
        if "GM_SLAB_BITS" in env:                                        # (the slabs are the index's: one of its own for the block)
            contigs = oa.load_long_genome()[0]
            ix = gm.Index(contigs, names=[b"contig1", b"contig2"], params=gm.default_params_cs() if is_cs(tag) else gm.default_params())
            p, _ = params_of(gm, tag); s = gm.Session(ix, params=p, max_batch_reads=256)
            try:
                assert ix.n_slabs == 2
                g = inputs(tag.split(":")[0]); got = ix.sam_header() + (s.map_reads_cs if is_cs(tag) else s.map_reads)(g["reads"]); st = dict(s.stats)
            finally: s.close(); ix.close()
            k1 = None
        else: got, st, k1, _ = map_case(gm, tag)
    assert got == want, (_first_diff(got, want), st)
    if kern: assert k1 == kern, (k1, kern)


@pytest.mark.gpu
def test_a_forced_v5_lookup_at_257_bases_gives_the_same_bytes(gm):
    """GM_K1_V5=1 at 732 lists a read-strand: k_lookup_v5 in its full shape, one round (the plan admits it at 1 161 and 2 961 lists too: not run here)"""
    with env_set(GM_K1_V5="1"):
        got, st, k1, _ = map_case(gm, "ls_257:default")
    assert got == oa.load_long_sam("ls_257:default"), (_first_diff(got, oa.load_long_sam("ls_257:default")), st)
    assert k1 == "k_lookup_v5"


@pytest.mark.gpu
@pytest.mark.parametrize("env", [dict(GM_P2_G4="0"), dict(GM_P2_G="16")], ids=["one_window", "four_windows"])
@pytest.mark.parametrize("tag", ["cs_400:default", "cs_204:unit", "ls_400:default"])
def test_the_other_pass_2_kernels_give_the_same_bytes(gm, tag, env):
    """GM_P2_G4=0: k_pass2_cs / k_pass2, one window a wave, where four or eight would run; GM_P2_G=16: four windows with int rows where the eight-window kernel would run"""
    with env_set(**env):
        got, st, _, p2 = map_case(gm, tag)
    assert got == oa.load_long_sam(tag), (_first_diff(got, oa.load_long_sam(tag)), st)
    if "GM_P2_G4" in env: assert p2 == ("k_pass2_cs" if is_cs(tag) else "k_pass2")
    else: assert p2 == ("k_pass2_cs_g4<16,int>" if is_cs(tag) else "k_pass2_g4<16,int>")


def records_by_name(sam):
    """QNAME -> its records, in their order, of a SAM text (header lines dropped)"""
    d = {}
    for l in sam.split(b"\n"):
        if l and not l.startswith(b"@"): d.setdefault(l.split(b"\t", 1)[0], []).append(l + b"\n")
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", ["0", "1"])
@pytest.mark.parametrize("tag", VARIANT_TAGS + ["pairs_2x250_opp-in:default"])
def test_three_sub_batches_under_both_pipeline_orders(gm, tag, overlap):
    """192 reads or pairs -- the input's own, taken again from the front where it has fewer -- on a session of 64 (the smallest sub-batch a session makes): three sub-batches,
    counted by the lookup launches of the call (unpaired: one a sub-batch), with the fronts of the next one queued ahead (GM_OVERLAP=1) and in strict order (0);
    every read's records are the golden's"""
    n = oa.LONG_INPUTS[tag.split(":")[0]]["n"]; pick = [i % n for i in range(192)]
    with env_set(GM_OVERLAP=overlap):
        got, st, _, _ = map_case(gm, tag, max_batch_reads=64, pick=pick)
    # (paired mode: two lookups a sub-batch and those of the half-paired rescue behind them -- at least six; that the pairs go in three sub-batches follows from the
    # session's size alone there: a sub-batch holds at most max_batch_reads and at least 64)
    assert (st["sub_batches"] >= 6) if is_pairs(tag) else (st["sub_batches"] == 3), st
    want = records_by_name(oa.load_long_sam(tag)); g = inputs(tag.split(":")[0])
    names = [g["names1"][i][:-2] for i in pick] if is_pairs(tag) else [b"r%d" % i for i in pick]
    body = b"".join(l + b"\n" for l in got.split(b"\n") if l and not l.startswith(b"@"))
    assert body == b"".join(b"".join(want[nm]) for nm in names), st


@pytest.mark.gpu
def test_one_session_follows_the_read_length_up_and_down(gm):
    """a session maps the 128-base input (the shortest on this genome: the 100-base goldens have genomes of their own), then the 1 000-base one, then the short one again:
    each byte-equal"""
    p, _ = params_of(gm, "ls_128:default"); s = gm.Session(index_of(gm, "ls_128:default"), params=p, max_batch_reads=256)
    try:
        for tag in ("ls_128:default", "ls_1000:default", "ls_128:default"):
            got = map_on(gm, s, tag); want = oa.load_long_sam(tag)
            assert got == want, (tag, _first_diff(got, want))
    finally: s.close()


@pytest.mark.gpu
def test_one_colour_space_session_follows_the_read_length_through_two_pass_2_kernels(gm):
    p, _ = params_of(gm, "cs_129:default"); s = gm.Session(index_of(gm, "cs_129:default"), params=p, max_batch_reads=256)
    try:
        for tag, k in (("cs_129:default", "k_pass2_cs_g4<16,int>"), ("cs_1000:default", "k_pass2_cs"), ("cs_129:default", "k_pass2_cs_g4<16,int>")):
            got = map_on(gm, s, tag); want = oa.load_long_sam(tag)
            assert got == want, (tag, _first_diff(got, want))
            assert gm.lib().gm_last_pass2_kernel().decode() == k
    finally: s.close()


# ---- the seams -------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ls_257", "ls_400", "ls_1000"])
def test_read_windows_equal_the_driver_and_score_windows_the_oracle(gm, driver, oracle_lib, name):
    """Session.read_windows row by row against the windows driver (groups of equal (read, st, cn, g_off) as multisets, no row dropped), and Session.score_windows on those
    windows against the oracle's sw_vector at the same addresses"""
    from tests.test_many_contigs import oracle_scores
    tag = name + ":default"; g = inputs(name); reads = np.ascontiguousarray(g["reads"], dtype=np.uint8)
    want, want_off = driver_rows(driver, name)
    p, _ = params_of(gm, tag); s = gm.Session(index_of(gm, tag), params=p, max_batch_reads=256)
    try:
        wins, off = s.read_windows(reads)
        rows = trw.as_rows(wins)
        assert np.array_equal(off, want_off), np.nonzero(off != want_off)[0][:10]
        a, b = trw.canon(rows), trw.canon(want)
        assert a.shape == b.shape and np.array_equal(a, b), (a[(a != b).any(axis=1)][:5], b[(a != b).any(axis=1)][:5])
        scores, _ = s.score_windows(reads, wins, off)
    finally: s.close()
    ws = oracle_scores(rows, g["contigs"], reads, False, False, p)
    bad = np.nonzero(scores != ws)[0]
    assert len(bad) == 0, (len(bad), rows[bad[:5]], scores[bad[:5]], ws[bad[:5]])
    assert int(ws.max()) > 10 * 128 and len(rows) > len(reads)              # (scores beyond the first stripe of 128 rows)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ls_257", "ls_400", "ls_1000"])
def test_read_hits_equal_the_three_calls(gm, name):
    """Session.read_hits == read_windows -> score_windows -> select_pass1 on the same session"""
    from tests import test_pass1_seam as tps
    tag = name + ":default"; reads = np.ascontiguousarray(inputs(name)["reads"], dtype=np.uint8)
    p, _ = params_of(gm, tag); s = gm.Session(index_of(gm, tag), params=p, max_batch_reads=256)
    try:
        chain = tps.chain_of(s, p, reads, cache=True)
        hits, hit_off, wins, off, scores = s.read_hits(reads, want_windows=True)
        tps.same_up_to_equal_windows((wins, off, scores, hits, hit_off), chain)
        assert len(set(hits["read"].tolist())) >= 0.9 * len(reads)
    finally: s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["ls_257:default", "ls_400:default", "ls_1000:default"])
def test_read_mappings_equal_the_chain_of_seams_and_the_reference(gm, tag):
    """Session.read_mappings == its own hits through sw_vector_batch -> sw_full_ls_batch -> select_pass2 -> the text entry (the chain of tests/test_read_mappings.py), array
    by array; through sam_records the reference's records, read by read, no read left out; and the bytes map_reads gives on the same session"""
    from tests import test_read_mappings as trm
    g = inputs(tag.split(":")[0]); reads = np.ascontiguousarray(g["reads"], dtype=np.uint8)
    p, _ = params_of(gm, tag); ix = index_of(gm, tag); s = gm.Session(ix, params=p, max_batch_reads=256)
    try:
        R = s.read_mappings(reads, want_ops=True)
        c = trm.chain_of(gm, ix, s, p, reads, R)
        n_run = trm.assert_equals_chain(gm, p, R, c)
        assert len(R.hits) > len(reads) and len(R.maps) > len(reads) and n_run > len(reads) // 2
        got, off = s.sam_records(reads, R)
        mapped = s.map_reads(reads)
    finally: s.close()
    body = b"".join(l + b"\n" for l in oa.load_long_sam(tag).split(b"\n") if l and not l.startswith(b"@"))
    want = trm.by_read(body, len(reads))
    bad = [r for r in range(len(reads)) if got[int(off[r]):int(off[r + 1])] != want[r]]
    assert not bad, (len(bad), [(got[int(off[r]):int(off[r + 1])], want[r]) for r in bad[:2]])
    assert bytes(got[:int(off[len(reads)])]) == mapped == body


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["cs_400:default", "cs_557:default"])
def test_read_mappings_cs_equal_the_chain_of_seams_and_the_reference(gm, oracle_lib, tag):
    """colour space: Session.read_mappings_cs == its hits through sw_full_cs_batch -> post_sw_batch -> select_pass2 -> the text entry (tests/test_read_mappings_cs.py), and
    through sam_records the reference's records -- k_post_sw_cs on columns of several hundred colours -- and map_reads_cs's bytes on the same session"""
    from tests import test_read_mappings_cs as trc
    g = inputs(tag.split(":")[0]); n = len(g["reads"])
    F = dict(contigs=g["contigs"], cnames=None, reads=np.ascontiguousarray(g["reads"], dtype=np.uint8), names=None, quals=None, qual_delta=33)
    p, _ = params_of(gm, tag); ix = index_of(gm, tag); s = gm.Session(ix, params=p, max_batch_reads=256)
    try:
        R = s.read_mappings_cs(F["reads"], want_ops=True)
        c = trc.chain_of(gm, ix, s, p, F, R)
        trc.assert_equals_chain(gm, p, R, c)
        assert len(R.hits) > n and len(R.maps) > n
        mine = trc.sam_of(s, F, R)
        skip = trc.tied(s, F)
        mapped = s.map_reads_cs(F["reads"])
    finally: s.close()
    body = b"".join(l + b"\n" for l in oa.load_long_sam(tag).split(b"\n") if l and not l.startswith(b"@"))
    want = trc.by_read(body, None, n)
    bad = [r for r in range(n) if r not in skip and mine[r] != want[r]]
    assert not bad and len(skip) <= n // 10, (len(bad), len(skip), [(mine[r], want[r]) for r in bad[:2]])
    assert mapped == body


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["pairs_2x250_opp-in:default", "pairs_400_100_col-fw:default", "pairs_400_100_col-bw:nhp"])
def test_pair_mappings_give_every_record_of_the_reference(gm, tag):
    """Session.pair_mappings through the record builder of tests/test_pair_mappings.py == the reference's records, field by field and in order, no pair left out"""
    from tests import test_pair_mappings as tpm
    name = tag.split(":")[0]; g = inputs(name); n = len(g["m1"]); base = "long_" + name; rid = base + "@" + tag.split(":")[1]
    p, pair_fields = params_of(gm, tag)
    tpm._FX[base] = {k: g[k] for k in ("contigs", "contig_names", "m1", "m2", "names1", "names2", "mode", "ins")}
    tpm.RUNS[rid] = (base, tag.split(":")[1], {}, pair_fields, None)
    opts = gm.PairOpts.default(g["mode"], g["ins"][0], g["ins"][1])
    for k, v in pair_fields.items(): setattr(opts, k, v)
    s = gm.Session(index_of(gm, tag), params=p, max_batch_reads=128)
    try:
        pm = s.pair_mappings(g["m1"], g["m2"], opts); st = s.stats
    finally: s.close()
    try: n_rec = tpm.check_against_golden(rid, tpm._FX[base], p, n, pm)
    finally: del tpm.RUNS[rid]
    assert n_rec > 2 * n and st["reads"] == 2 * n


# ---- refusals, each with a good call behind it -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lengths_beyond_the_admitted_ones_are_refused_before_anything_is_uploaded(gm):
    """colour-space --local one colour past LONG_CS_LOCAL_LAST, reads one past longest_read_len in both spaces, and the weight-16 -H set at 1 000 bases (the front's prune
    kernel, REFUSED_TAGS): GM_E_RANGE with the figure named, and the session maps a golden afterwards (check_read_len runs in the call's argument check, before the
    call touches the device).  The longest
    admitted colour-space --local length itself maps its golden (test_map_equals_the_reference_golden, cs_555:local)."""
    L = oa.LONG_CS_LOCAL_LAST
    p, _ = params_of(gm, "cs_555:local"); s = gm.Session(index_of(gm, "cs_555:local"), params=p, max_batch_reads=64)
    try:
        with pytest.raises(gm.GmError) as e: s.map_reads_cs(np.zeros((4, L + 2), dtype=np.uint8))
        assert "(%d)" % GM_E_RANGE in str(e.value) and "reads of %d" % (L + 1) in str(e.value) and "columns" in str(e.value), str(e.value)
        with pytest.raises(gm.GmError) as e: s.map_reads_cs(np.zeros((4, 1002), dtype=np.uint8))
        assert "(%d)" % GM_E_RANGE in str(e.value) and "read length 1001" in str(e.value), str(e.value)
        got = map_on(gm, s, "cs_555:local")
    finally: s.close()
    assert got == oa.load_long_sam("cs_555:local")
    tag = REFUSED_TAGS[0]; p, _ = params_of(gm, tag); s = gm.Session(index_of(gm, tag), params=p, max_batch_reads=64)
    try:
        with pytest.raises(gm.GmError) as e: map_on(gm, s, tag)
        assert "(%d)" % GM_E_RANGE in str(e.value) and "reads of 1000" in str(e.value) and "prune kernel needs 262144 bytes" in str(e.value) and "163840" in str(e.value), str(e.value)
        with pytest.raises(gm.GmError) as e: s.map_reads(np.zeros((4, 1001), dtype=np.uint8))
        assert "(%d)" % GM_E_RANGE in str(e.value) and "read length 1001" in str(e.value), str(e.value)
        got = map_on(gm, s, "ls_257:w16H")                               # the same session and index at 257 bases
    finally: s.close()
    assert got == oa.load_long_sam("ls_257:w16H")
