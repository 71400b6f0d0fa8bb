"""The seed lookup under other seed sets than the ones the suite has run (tests/oracle_api.py SEED_SETS; fixtures: tools/make_golden.py --seeds-only).

  ref_w10 ref_w11 ref_w16H ref_w18H   the non-default rows of the reference's own seed table; the two -H sets have spans of 26 to 30: four words under the hashed key
  span32 span32H span32_14 span31_25H the span limit, alone, hashed, beside a short seed (one max_seed_span for both), and 31 + 25
  one sixteen w13 w14 contiguous      one seed, GM_MAX_SEEDS seeds (784 lists a read-strand at 60 colours, 1 424 at 100 bases), the weight limit

Each set runs through the reference on four committed inputs (SEED_RUNS): stress_100bp_unal, n1_noisy_70bp's first 1 500 reads under -n 1 and by default, and
stress_cs_60col_unal's first 600 reads; w14 on the two default-mode letter-space ones.  The goldens are the records only, written with --sam-unaligned and
--extra-sam-fields -- except on stress_100bp_unal, where the reference does not return from --extra-sam-fields (an N in the edit string of a record on the negative
strand: reverse_alignment_edit_string knows A C G T only), so that input is stored without them.  ZM, the seed matches of a window, is the field that notices a
seed's lists missing; the n1_noisy and colour-space goldens carry it.

Without a GPU: the oracle gives every golden byte for byte, the windows driver carries ZM / ZR / ZV of every record, and the fixtures can fail: the oracle with any
one seed left out (a single seed: with one mask bit cleared) differs from a golden.  With one: the library gives the same bytes on both builds, its windows are the
driver's under every lookup variant with the kernel the plan names, and seed sets beyond a limit are refused by name."""
import ctypes as C
import gzip, os, re, shutil, subprocess, sys
import numpy as np
import pytest
from tests import oracle_api as oa
from tests import test_read_windows as trw
from tests.test_pair_edges import env_set

GOLD = os.path.join(oa.ROOT, "tests", "golden")
CASES = [(name, run) for name in oa.SEED_SETS for run in oa.seed_runs(name)]
case_id = lambda c: c[0] + (c[1] or "_stress")
RELEASE_SETS = ("ref_w16H", "span32_14", "span32H", "sixteen", "one")
WINDOW_SETS = [n for n in oa.SEED_SETS if n != "w14"]

_in = {}
def inputs(run):
    """(contigs, reads) of a run of SEED_RUNS, loaded once"""
    base, n, cs, n1 = oa.SEED_RUNS[run]
    if base not in _in:
        contigs, reads, _ = oa.load_golden(base)
        _in[base] = ([np.ascontiguousarray(c, dtype=np.uint8) for c in contigs], np.ascontiguousarray(reads, dtype=np.uint8))
    contigs, reads = _in[base]
    return contigs, np.ascontiguousarray(reads[:n] if n else reads)


def golden_name(name, run):
    base, n, cs, n1 = oa.SEED_RUNS[run]
    return "%s@seeds_%s%s" % (base, name, "_n1" if n1 else "")


def has_extra(run): return run not in oa.SEED_RUNS_NO_EXTRA


def _first_diff(a, b):
    la, lb = a.split(b"\n"), b.split(b"\n")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y: return i, x[:400], y[:400]
    return min(len(la), len(lb)), len(la), len(lb)


def oracle_sam(seeds, hashed, run):
    base, n, cs, n1 = oa.SEED_RUNS[run]
    contigs, reads = inputs(run)
    o = oa.Session(contigs, opts=oa.seed_oracle_opts(seeds, hashed, cs, n1) + (";extra-sam-fields=1" if has_extra(run) else ""))
    o.set(hash_filter_calls=True, sam_unaligned=True)
    got = o.map_sam(reads, nthreads=trw.THREADS); o.close()
    return got


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_equals_the_reference_under_the_seed_set(oracle_lib, case):
    """byte for byte, ZM / ZR / ZV / ZH / ZE included where the golden has them"""
    name, run = case; seeds, hashed = oa.SEED_SETS[name]
    want = oa.load_seed_sam(name, run)
    assert not want.startswith(b"@") and (b"\tZM:i:" in want) == has_extra(run)
    got = oracle_sam(seeds, hashed, run)
    assert got == want, _first_diff(got, want)


def test_every_new_fixture_is_no_larger_than_the_largest_before_it():
    n = 0
    for dirpath, _, files in os.walk(GOLD):
        for f in files:
            if "@seeds_" in f or os.path.basename(dirpath) in oa.SEED_INDEX_CASES:
                n += 1; assert os.path.getsize(os.path.join(dirpath, f)) <= 734_000, f
    assert n == len(CASES) + sum(3 + len(s) for s, _ in oa.SEED_INDEX_CASES.values())


driver = trw.driver
_drv = {}
def run_driver(L, seeds, hashed, cs, mode, contigs, reads):
    """the driver's rows (tests/read_windows_oracle.cpp rwo_create_opts) for a seed set on a genome and reads"""
    u8p = C.POINTER(C.c_uint8)
    L.rwo_create_opts.argtypes = [C.c_int, C.POINTER(u8p), C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p)]; L.rwo_create_opts.restype = C.c_void_p
    h = L.rwo_create_opts(len(contigs), (u8p * len(contigs))(*[c.ctypes.data_as(u8p) for c in contigs]), (C.c_uint64 * len(contigs))(*[len(c) for c in contigs]),
                          int(cs), mode, int(hashed), len(seeds), (C.c_char_p * len(seeds))(*[s.encode() for s in seeds]))
    cap = 64 * len(reads)
    for _ in range(2):                                               # (the call says how many rows there are: a second one when the first array was too small)
        rows = np.zeros((cap, 12), dtype=np.int64)
        w = L.rwo_windows(h, reads.shape[0], reads.shape[1], reads.ctypes.data_as(u8p), trw.THREADS, rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
        if w <= cap: break
        cap = int(w)
    L.rwo_destroy(h)
    assert 0 < w <= cap, w
    return rows[:w].copy()


def driver_rows(L, seeds, hashed, run):
    """(rows, off) of the driver under a seed set on a run's reads, computed once"""
    key = (tuple(seeds), hashed, run)
    if key not in _drv:
        base, n, cs, n1 = oa.SEED_RUNS[run]
        contigs, reads = inputs(run)
        rows = run_driver(L, seeds, hashed, cs, 1 if n1 else 2, contigs, reads)
        _drv[key] = (rows, trw.offsets(rows, len(reads)))
    return _drv[key]


def set_rows(L, name, run): return driver_rows(L, *oa.SEED_SETS[name], run)


@pytest.mark.parametrize("case", [c for c in CASES if has_extra(c[1])], ids=case_id)
def test_driver_windows_carry_the_records_and_give_zv(driver, oracle_lib, case):
    """every mapped record of the golden has a driver window of its read and strand that covers the alignment and carries its ZM and ZR; the oracle's vector score at
    the header's address of one such window is its ZV (trw.candidates / trw.some_candidate_gives_zv)"""
    name, run = case; cs = oa.SEED_RUNS[run][2]
    contigs, reads = inputs(run)
    rows, off = set_rows(driver, name, run)
    assert trw.in_list_order(rows)
    recs = trw.records(golden_name(name, run))
    assert len(recs) >= 500
    cands = trw.candidates(rows, off, recs)
    clen = np.array([len(c) for c in contigs], dtype=np.int64)
    used = sorted(set(r[2] for r in recs))
    letters = {c: [contigs[c], trw.CMPL[contigs[c][::-1]]] for c in used}
    ls = {c: [trw.pack(x) for x in letters[c]] for c in used}
    csw = {c: [trw.pack(trw.colours(x)) for x in letters[c]] for c in used} if cs else None
    rw = [trw.pack(r[1:] if cs else r) for r in reads]; rlen = reads.shape[1] - (1 if cs else 0)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))

    def scores_of(idx, rd):
        st, goff = trw.header_address(rows[idx], clen)
        out = np.zeros(len(idx), dtype=np.int64)
        for k, (i, r) in enumerate(zip(idx, rd)):
            cn, wl = int(rows[i, 2]), int(rows[i, 4])
            if cs: out[k] = oracle_lib.gmo_sw_vector_cs(u32(csw[cn][st[k]]), int(goff[k]), wl, u32(rw[r]), rlen, u32(ls[cn][st[k]]), int(reads[r, 0]))
            else: out[k] = oracle_lib.gmo_sw_vector(u32(ls[cn][st[k]]), int(goff[k]), wl, u32(rw[r]), rlen)
        return out
    trw.some_candidate_gives_zv(recs, cands, scores_of)


def lesser_sets(name):
    """the sets the fixtures must tell from `name`: every seed left out in turn; a single seed: its second 1 cleared"""
    seeds, hashed = oa.SEED_SETS[name]
    if len(seeds) > 1: return [("without seed %d" % i, seeds[:i] + seeds[i + 1:]) for i in range(len(seeds))]
    s = seeds[0]; k = s.index("1", 1)
    return [("bit %d cleared" % k, [s[:k] + "0" + s[k + 1:]])]


@pytest.mark.parametrize("name", sorted(oa.SEED_SETS))
def test_the_fixtures_notice_a_missing_seed(oracle_lib, name):
    """A condition on the FIXTURES, checked with the oracle: were a seed's lists missing (or one position of a single seed not compared), some record of some golden of
    the set would differ.  The inputs are tried in the order -n 1, default mode on the same reads, colour space, stress_100bp_unal; the first that differs settles it."""
    hashed = oa.SEED_SETS[name][1]
    order = [r for r in ("_n1", "_def", "_cs", "") if r in oa.seed_runs(name)]
    for what, seeds in lesser_sets(name):
        for run in order:
            if oracle_sam(seeds, hashed, run) != oa.load_seed_sam(name, run): break
        else: pytest.fail("%s %s: no golden differs -- the inputs are too easy for this set" % (name, what))


def index_fixture(name):
    d = os.path.join(GOLD, name); z = np.load(os.path.join(d, "inputs.npz"))
    contigs = [np.ascontiguousarray(z["contig%d" % i], dtype=np.uint8) for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    with gzip.open(os.path.join(d, "from_index.sam.gz"), "rb") as f: sam = f.read()
    return d, contigs, [bytes(x) for x in z["contig_names"]], z["reads"], str(z["seeds"]).split(","), sam


@pytest.mark.parametrize("name", sorted(oa.SEED_INDEX_CASES))
def test_oracle_index_reproduces_the_reference_index_run(oracle_lib, name):
    """the reference's -L run from its own -S files of a genome with contigs of 31, 32 and 33 bases and single Ns at both ends of a span-32 k-mer"""
    d, contigs, names, reads, seeds, sam = index_fixture(name)
    assert seeds == oa.SEED_INDEX_CASES[name][0] and [len(c) for c in contigs[2:]] == [31, 32, 33]
    assert contigs[0][1] == 15 and contigs[0][-2] == 15 and contigs[1][0] == 15 and contigs[1][-1] == 15
    o = oa.Session(contigs, contig_names=names, opts=oa.seed_oracle_opts(seeds, oa.SEED_INDEX_CASES[name][1]))
    got = oa.sam_header(contigs, names) + o.map_sam(reads, nthreads=2); o.close()
    assert got == sam, _first_diff(got, sam)
    assert sam.count(b"\n") - len(contigs) - 1 >= 300


# ---- which kernel the plan names -------------------------------------------------------------------------------------------------------------------------------
# the lookup variants of the tuning build (tests/test_gpu_parity.py KERNEL_VARIANTS reads the same knobs); the index is rebuilt under each: GM_SLAB_BITS and
# GM_NO_BUCKETS are read when it is made
VARIANTS = [{}, {"GM_NO_BUCKETS": "1"}, {"GM_SLAB_BITS": "18"}, {"GM_SLAB_BITS": "18", "GM_K1_V4": "1"}, {"GM_SLAB_BITS": "18", "GM_K1_V5": "1"},
            {"GM_SLAB_BITS": "18", "GM_K1_V5": "1", "GM_K5_ROUNDS": "3"}, {"GM_SLAB_BITS": "18", "GM_K1_V5": "1", "GM_K5_HALF": "1", "GM_K5_ROUNDS": "2"},
            {"GM_SLAB_BITS": "18", "GM_K1_V2": "1"}, {"GM_SCAP": "256", "GM_SCAP2": "64"}]
N1_VARIANTS = [{}, {"GM_SLAB_BITS": "18"}]
env_id = lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default"
# What gm_last_lookup_kernel() must name: run -> per variant (the kernel of most sets, {set: another}).  Recorded from k1_plan (gm_lookup_plan.h) through the query
# mode of tests/host/lookup_plan_main.cpp and read against the header; test_the_kernel_table_is_the_plans keeps it there.  Where a variant declines:
#   sixteen     NL = 1 424 at 100 bases, 784 at 60 colours: no bucket kernel (NL > 512), no half-size shape; a forced v4 does not fit its LDS at 1 424 lists; forced
#               rounds decline with NL > 1 024 threads at 100 bases and at 60 colours because the lists leave seen[] only 2^14 words -- all of them fall to v3
#   ref_w*      four seeds, 356 lists at 100 bases: the half-size shape does not fit its 80 KB (24 B a list + the tables), the full shape runs the two rounds
_SIX3 = {"sixteen": "k_lookup_v3"}
KERNEL_TABLE = {
    "": [("k_lookup_bkt", _SIX3), ("k_lookup_v3", {}), ("k_lookup_v3", {}), ("k_lookup_v4", _SIX3), ("k_lookup_v5", {}), ("k_lookup_v5_rounds", _SIX3),
         ("k_lookup_v5_half", dict(_SIX3, ref_w10="k_lookup_v5_rounds", ref_w11="k_lookup_v5_rounds", ref_w16H="k_lookup_v5_rounds", ref_w18H="k_lookup_v5_rounds")),
         ("k_lookup", {}), ("k_lookup_bkt", _SIX3)],
    "_cs": [("k_lookup_bkt", _SIX3), ("k_lookup_v3", {}), ("k_lookup_v3", {}), ("k_lookup_v4", {}), ("k_lookup_v5", {}), ("k_lookup_v5_rounds", _SIX3),
            ("k_lookup_v5_half", _SIX3), ("k_lookup", {}), ("k_lookup_bkt", _SIX3)],
    "_n1": [("k_lookup", {}), ("k_lookup", {})],             # -n 1: the sweep kernel is the only one that mode has
}


def table_kernel(name, run, env):
    most, other = KERNEL_TABLE[run][(N1_VARIANTS if run == "_n1" else VARIANTS).index(env)]
    return other.get(name, most)


def test_the_kernel_table_is_the_plans(tmp_path):
    """every (set, input, variant) of KERNEL_TABLE against k1_plan on that shape: the genome's length, the read length, the set's spans and weights, -H, the knobs"""
    exe = str(tmp_path / "lookup_plan_main")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(oa.ROOT, "shrimp_amd", "csrc"), "-o", exe, os.path.join(oa.ROOT, "tests", "host", "lookup_plan_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = set()
    for run in KERNEL_TABLE:
        base, n, cs, n1 = oa.SEED_RUNS[run]; contigs, reads = inputs(run)
        for env in (N1_VARIANTS if n1 else VARIANTS):
            for name in WINDOW_SETS:
                seeds, hashed = oa.SEED_SETS[name]
                p = subprocess.run([exe, "query", str(sum(len(c) for c in contigs)), str(int(cs)), str(int(hashed)), str(reads.shape[1] - int(cs)), str(len(reads)), "8" if n1 else "0",
                                    ";".join("%s=%s" % kv for kv in env.items()) or "-", ",".join(seeds)], capture_output=True, text=True)
                assert p.returncode == 0 and p.stdout.split(" | ")[0] == table_kernel(name, run, env), (name, run, env, p.stdout)
                seen.add(p.stdout.split(" | ")[0])
    assert seen == {"k_lookup", "k_lookup_bkt", "k_lookup_v3", "k_lookup_v4", "k_lookup_v5", "k_lookup_v5_rounds", "k_lookup_v5_half"}      # every family is reached


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


def params_of(gm, name, run, sam=False):
    base, n, cs, n1 = oa.SEED_RUNS[run]
    p = gm.default_params_cs() if cs else gm.default_params()
    p.hash_seeds = int(oa.SEED_SETS[name][1]); p.match_mode = 1 if n1 else 2
    if sam: p.sam_unaligned = 1; p.extra_sam_fields = int(has_extra(run))
    return p


_open = {}
def opened(gm, name, run):
    """(index, session, params) of a set on a run's genome; one at a time stays open (the buckets of a weight-14 seed alone are 17 GB of HBM)"""
    if (name, run) not in _open:
        close_all()
        p = params_of(gm, name, run, sam=True)
        ix = gm.Index(inputs(run)[0], seeds=oa.SEED_SETS[name][0], params=p)
        _open[(name, run)] = (ix, gm.Session(ix, params=p, max_batch_reads=4096), p)
    return _open[(name, run)]


def close_all():
    for ix, s, _ in _open.values(): s.close(); ix.close()
    _open.clear()


@pytest.fixture(scope="module", autouse=True)
def close_the_sessions_of_this_module():
    yield
    close_all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_sam_matches_reference_golden(gm, case):
    """map_reads / map_reads_cs under the seed set == the reference's records byte for byte, extra fields included; the header is the index's own.  (w14: 4^14 lists)"""
    name, run = case; cs = oa.SEED_RUNS[run][2]
    contigs, reads = inputs(run); want = oa.load_seed_sam(name, run)
    ix, s, _ = opened(gm, name, run)
    got = (s.map_reads_cs if cs else s.map_reads)(reads)
    assert ix.sam_header() == oa.sam_header(contigs)
    assert got == want, (_first_diff(got, want), s.stats)


@pytest.mark.gpu
def test_release_build_reproduces_the_seed_set_goldens():
    """`make release` (no tuning knobs compiled in; the build bench.py measures): the golden test of five sets in a child interpreter with GM_LIB_PATH on
    libgmapper_hip_release.so"""
    rel = os.path.join(oa.ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    assert os.path.exists(rel), "make -C shrimp_amd/csrc release (or __graft_entry__.build()) has not run"
    close_all()
    sel = "test_sam_matches_reference_golden and (" + " or ".join(RELEASE_SETS) + ")"
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       capture_output=True, text=True, env=dict(os.environ, GM_LIB_PATH=rel), cwd=oa.ROOT, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    m = re.search(r"(\d+) passed", p.stdout)
    assert m and int(m.group(1)) == sum(1 for n, _ in CASES if n in RELEASE_SETS), p.stdout[-500:]


def library_rows(gm, name, run, env, reads=None):
    base, n, cs, n1 = oa.SEED_RUNS[run]
    contigs, own = inputs(run); reads = own if reads is None else reads
    with env_set(**env):
        p = params_of(gm, name, run)
        ix = gm.Index(contigs, seeds=oa.SEED_SETS[name][0], params=p); s = gm.Session(ix, params=p, max_batch_reads=4096)
        try:
            wins, off = s.read_windows(np.ascontiguousarray(reads[:, 1:]), initbp=np.ascontiguousarray(reads[:, 0])) if cs else s.read_windows(reads)
            kern = gm.lib().gm_last_lookup_kernel().decode()
        finally: s.close(); ix.close()
    return trw.as_rows(wins), off, kern


def windows_equal_the_driver(gm, driver, name, run, env):
    reads = inputs(run)[1]; want, want_off = set_rows(driver, name, run)
    rows, off, kern = library_rows(gm, name, run, env)
    print("%s %s [%s]: %s, %d windows" % (name, run or "stress", env_id(env), kern, len(rows)))
    assert kern == table_kernel(name, run, env), (kern, table_kernel(name, run, env))
    assert np.array_equal(off, trw.offsets(rows, len(reads))) and trw.in_list_order(rows) and (rows[:, 11] == 0).all()
    assert np.array_equal(off, want_off), np.nonzero(off != want_off)[0][:10]
    a, b = trw.canon(rows), trw.canon(want)
    assert np.array_equal(a, b), (a[(a != b).any(axis=1)][:5], b[(a != b).any(axis=1)][:5])


@pytest.mark.gpu
@pytest.mark.parametrize("env", VARIANTS, ids=env_id)
@pytest.mark.parametrize("run", ["", "_cs"], ids=["stress", "cs"])
@pytest.mark.parametrize("name", WINDOW_SETS)
def test_read_windows_equal_the_driver_under_each_lookup_variant(gm, driver, name, run, env):
    """Session.read_windows == the driver row by row (tie groups through canon): cn, g_off, w_len, the match count, the window score and the anchor box of every
    window; gm_last_lookup_kernel() is the kernel KERNEL_TABLE names, also where a variant declines"""
    windows_equal_the_driver(gm, driver, name, run, env)


@pytest.mark.gpu
@pytest.mark.parametrize("env", N1_VARIANTS, ids=env_id)
@pytest.mark.parametrize("name", WINDOW_SETS)
def test_read_windows_equal_the_driver_without_region_counts(gm, driver, name, env):
    """-n 1: every list entry is an anchor"""
    windows_equal_the_driver(gm, driver, name, "_n1", env)


def anchor_heavy_reads():
    """200 exact and 200 lightly mutated 100-base reads of stress_100bp_unal's genome by a fixed rule: read i starts at 1 000 + 149 i of contig 1 + i % 2 (the two long
    i.i.d. contigs; codes above 3 become N as in the fixture's own reads), every second one reverse-complemented; the mutated ones change bases 17, 50 and 83"""
    contigs, _ = inputs("")
    reads = np.zeros((400, 100), dtype=np.uint8)
    for i in range(400):
        c = contigs[1 if i % 2 else 3]; p = 1000 + 149 * (i // 2)
        r = np.where(c[p:p + 100] > 3, 15, c[p:p + 100]).astype(np.uint8)
        if i >= 200:
            for k in (17, 50, 83): r[k] = (r[k] + 1 + i % 3) & 3 if r[k] < 4 else r[k]
        if i % 4 >= 2: r = trw.CMPL[r[::-1]]
        reads[i] = r
    return reads


@pytest.mark.gpu
def test_more_than_1024_anchors_on_a_read_strand(gm, driver, oracle_lib):
    """sixteen seeds on exact 100-base reads: more seed matches in one window than K2's register sort holds keys (1 024).  read_windows against the driver, tophits
    against the oracle"""
    reads = anchor_heavy_reads(); seeds, hashed = oa.SEED_SETS["sixteen"]; contigs, _ = inputs("")
    want = run_driver(driver, seeds, hashed, False, 2, contigs, reads)
    assert int(want[:, 6].max()) > 1024, int(want[:, 6].max())          # what the test is for
    rows, off, kern = library_rows(gm, "sixteen", "", {}, reads=reads)
    assert kern == "k_lookup_v3" and np.array_equal(off, trw.offsets(want, 400))
    a, b = trw.canon(rows), trw.canon(want)
    assert np.array_equal(a, b), (a[(a != b).any(axis=1)][:5], b[(a != b).any(axis=1)][:5])
    ix, s, _ = opened(gm, "sixteen", "")
    got = s.tophits(reads)
    o = oa.Session(contigs, opts=oa.seed_oracle_opts(seeds, hashed)); top = o.tophits(reads); o.close()
    assert got.shape == top.shape and (got == top).all(), (got.shape, top.shape)
    assert len(top) >= 400


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ref_w16H", "sixteen", "span32_14"])
def test_scores_and_hits_under_the_seed_set(gm, oracle_lib, name):
    """Session.score_windows on the session's own windows == the oracle's vector scores at the same addresses; Session.read_hits == the three separate calls"""
    from tests.test_many_contigs import oracle_scores
    from tests import test_pass1_seam as tps
    contigs, reads = inputs(""); reads = np.ascontiguousarray(reads[:600])
    ix, s, p = opened(gm, name, "")
    wins, off = s.read_windows(reads); rows = trw.as_rows(wins)
    assert len(rows) >= 600
    scores, _ = s.score_windows(reads, wins, off)
    want = oracle_scores(rows, contigs, reads, False, False, p)
    bad = np.nonzero(scores != want)[0]
    assert len(bad) == 0, (len(bad), rows[bad[:5]], scores[bad[:5]], want[bad[:5]])
    chain = tps.chain_of(s, p, reads, cache=True)
    hits, hit_off, wins2, off2, scores2 = s.read_hits(reads, want_windows=True)
    tps.same_up_to_equal_windows((wins2, off2, scores2, hits, hit_off), chain)
    assert len(set(hits["read"].tolist())) >= 500


# ---- limits ----------------------------------------------------------------------------------------------------------------------------------------------------
_S17 = ["1" * 11 + "0" * k + "1" for k in range(17)]
# what, seeds, the words the message must hold: the seed (an empty one: its number) and the limit
LIMITS = [("span 33", ["1" * 6 + "0" * 21 + "1" * 6], ["1" * 6 + "0" * 21 + "1" * 6, "span 33", "limit is 32"]),
          ("weight 15 without -H", ["1" * 15], ["1" * 15, "weight 15", "limit is 14"]),
          ("17 seeds", _S17, [_S17[16], "more than 16 seeds"]),
          ("an empty seed", ["11110111101111", ""], ["seed 1", "empty"]),
          ("another character", ["1111011x101111"], ["1111011x101111", "character 7"])]


def small_genome():
    contigs, _ = inputs("")
    return [contigs[2], np.ascontiguousarray(contigs[1][:5000])]


@pytest.mark.gpu
@pytest.mark.parametrize("what,seeds,words", LIMITS, ids=[l[0] for l in LIMITS])
def test_seed_sets_beyond_a_limit_are_refused_by_name(gm, what, seeds, words):
    """GM_E_ARG with the seed and the limit in the message; the same call with a valid set succeeds afterwards"""
    with pytest.raises(gm.GmError) as e: gm.Index(small_genome(), seeds=seeds)
    msg = str(e.value)
    assert "(%d)" % trw.GM_E_ARG in msg and all(w in msg for w in words), msg
    ix = gm.Index(small_genome(), seeds=["11110111101111"]); assert len(ix.contigs()) == 2; ix.close()


@pytest.mark.gpu
def test_a_weight_15_seed_is_accepted_with_hashed_seeds(gm):
    p = gm.default_params(); p.hash_seeds = 1
    ix = gm.Index(small_genome(), seeds=["1" * 15], params=p); assert len(ix.contigs()) == 2; ix.close()


def _patch_seed_file(path, span=None, weight=None, mask=None):
    """a saved .seed.N file with its seed header changed: mode, Hflag (2 x uint32), mask (uint64), span, weight (2 x int32), then the lists"""
    with gzip.open(path, "rb") as f: data = bytearray(f.read())
    if mask is not None: data[8:16] = np.array([mask], dtype=np.uint64).tobytes()
    if span is not None: data[16:20] = np.array([span], dtype=np.int32).tobytes()
    if weight is not None: data[20:24] = np.array([weight], dtype=np.int32).tobytes()
    with gzip.open(path, "wb") as f: f.write(bytes(data))


@pytest.mark.gpu
def test_index_files_beyond_a_limit_are_refused_by_name(gm, tmp_path):
    """gm_index_load: a seed file whose span is 33, one whose mask has 15 ones without -H, and a seventeenth seed file; the untouched files load afterwards"""
    ix = gm.Index(small_genome(), seeds=["11110111", "1101011011"]); ix.save(str(tmp_path / "ok")); ix.close()
    def variant(tag, change):
        for f in os.listdir(tmp_path):
            if f.startswith("ok."): shutil.copy(str(tmp_path / f), str(tmp_path / (tag + f[2:])))
        change(str(tmp_path / tag)); return str(tmp_path / tag)
    cases = [(variant("span", lambda p: _patch_seed_file(p + ".seed.1", span=33)), ["seed.1", "span 33", "limit is 32"]),
             (variant("weight", lambda p: _patch_seed_file(p + ".seed.0", span=15, weight=15, mask=(1 << 15) - 1)), ["seed.0", "1" * 15, "weight 15", "limit is 14"]),
             (variant("many", lambda p: shutil.copy(p + ".seed.0", p + ".seed.16")), ["seed.16", "more than 16 seeds"])]
    for prefix, words in cases:
        with pytest.raises(gm.GmError) as e: gm.Index.load(prefix)
        msg = str(e.value)
        assert "(%d)" % trw.GM_E_ARG in msg and all(w in msg for w in words), msg
    ld = gm.Index.load(str(tmp_path / "ok")); assert len(ld.contigs()) == 2; ld.close()


# ---- the index fixtures ------------------------------------------------------------------------------------------------------------------------------------------
def unhashed_lists(contigs, seed):
    """numpy restatement of the unhashed key (kmer_to_mapidx_orig, ref: gmapper.h:349-368): {key: global positions} of every k-mer whose whole span is free of code 15
    (the reference resets on N, also under a 0 of the mask; any other code goes in by its low two bits); two bits a 1 of the mask, the LAST position highest"""
    span = len(seed); ones = [i for i, c in enumerate(seed) if c == "1"]; out = {}; off = 0
    for c in contigs:
        for p in range(len(c) - span + 1):
            w = c[p:p + span]
            if (w == 15).any(): continue
            key = 0
            for i in reversed(ones): key = (key << 2) | (int(w[i]) & 3)
            out.setdefault(key, []).append(off + p)
        off += len(c)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(oa.SEED_INDEX_CASES))
def test_index_files_are_the_reference_files_and_map_the_same(gm, name, tmp_path):
    """saved here == the reference's -S files (decompressed) byte for byte, from Index(contigs) and from Index.from_fasta; the reference's files load and map to its
    -L SAM; idxfix_s32: get_list against the numpy key at the short contigs and around each N"""
    d, contigs, names, reads, seeds, sam = index_fixture(name)
    p = gm.default_params(); p.hash_seeds = int(oa.SEED_INDEX_CASES[name][1])
    fa = str(tmp_path / "g.fa")
    T = np.frombuffer(b"ACGTUMRWSYKVHDBN", dtype=np.uint8)
    with open(fa, "wb") as f:
        for nm, c in zip(names, contigs): f.write(b">" + nm + b"\n" + T[c].tobytes() + b"\n")
    for tag, make in (("built", lambda: gm.Index(contigs, names=names, seeds=seeds, params=p)), ("fasta", lambda: gm.Index.from_fasta(fa, seeds=seeds, params=p))):
        ix = make(); ix.save(str(tmp_path / tag)); ix.close()
        for k in range(len(seeds) + 1):
            suffix = ".genome" if k == len(seeds) else ".seed.%d" % k
            with gzip.open(os.path.join(d, "idx" + suffix), "rb") as f: want = f.read()
            with gzip.open(str(tmp_path / (tag + suffix)), "rb") as f: got = f.read()
            assert got == want, (tag, suffix, len(got), len(want))
    ix = gm.Index.load(os.path.join(d, "idx"), params=p); s = gm.Session(ix, params=p, max_batch_reads=1024)
    try:
        got = oa.sam_header(contigs, names) + s.map_reads(reads)
        assert got == sam, _first_diff(got, sam)
        if name == "idxfix_s32":
            want = unhashed_lists(contigs, seeds[0]); off = [int(x) for x in np.concatenate([[0], np.cumsum([len(c) for c in contigs])])]
            at = {int(q): k for k, v in want.items() for q in v}
            assert not any(off[2] <= q < off[3] for q in at) and [q for q in at if off[3] <= q < off[4]] == [off[3]] and sorted(q for q in at if q >= off[4]) == [off[4], off[4] + 1]
            for n in (1, off[1] - 2, off[1], off[2] - 1):                                           # the four single Ns, global
                assert not any(q in at for q in range(max(0, n - 31), n + 1))                       # no k-mer over an N, under a 1 or under a 0
            near = (2, off[1] - 34, off[1] + 1, off[2] - 33)                                        # ... and the first one clear of it is there
            assert all(q in at for q in near)
            for k in sorted({at[q] for q in near + (off[3], off[4], off[4] + 1)}): assert ix.get_list(0, k).tolist() == want[k], k
            assert sum(len(ix.get_list(0, k)) for k in range(4 ** 8)) == len(at)
    finally: s.close(); ix.close()
