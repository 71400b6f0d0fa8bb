#!/usr/bin/env python3
"""Time post_sw on the reference's known-answer records: the single seam called once per record against one gm_post_sw_batch call.

    python tools/post_sw_batch_timing.py [--single-lib LIB.so] [--batch-lib NEW.so] [--runs 3] [--out profiles/r07a_post_sw_batch_timing.json]
                                         [--error-out profiles/r07a_post_sw_batch_error.json]

  (a) post_sw in a loop over the 1 222 records of tests/golden/sw_kat_post.txt.gz made without quality values (host code; --single-lib may be a library built
      from an older commit, default: the tree's release build)
  (b) one gm_post_sw_batch call over the same records (--batch-lib, default: the tree's release build), and one over the fixture repeated to about 100 000 items,
      the size the entry is meant for: one thread an item leaves most of the device idle at 1 222
Each timing is a child process of its own (one library a process), legs alternate a, b, a, b, ...; a child warms up first, then takes a host clock around calls that
end in a device synchronise (the batch call is repeated until the window holds at least half a second).  Both legs check their counts against the fixture.
--error-out: the largest relative difference of the device's posteriors from the reference's over the fixture and the share the host routine answered, per QV mode.

    python tools/post_sw_batch_timing.py --leg batch --lib NEW.so --repeat 82 --loops 5     # the child form, also what a kernel trace is taken of
"""
import argparse, ctypes as C, gzip, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

CS_SETUP = (1400, 1000, -33, -7, -33, -3, 10, -24, -20, True, 8, 0)
POST_MAX_LEN = 2400


def fixture(useq):
    """(post_sw_setup's six doubles, the "S" records the P records of this QV mode index, those P records)"""
    from tests.test_sw_full_batch import items_cs
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sw_kat_post.txt.gz"), "rt") as f: rows = [l.split() for l in f if l.strip()]
    K = [float.fromhex(x) for x in [t for t in rows if t[0] == "K"][0][1:]]
    P = [t for t in rows if t[0] == "P" and int(t[2]) == useq]
    S = items_cs("sw_kat_cs.txt.gz", "S")
    return K, [S[int(t[1])] for t in P], P


def leg_single(lib_path):
    from shrimp_amd import gmapper as gm
    L = C.CDLL(lib_path); u32p = C.POINTER(C.c_uint32)
    L.post_sw_setup.argtypes = [C.c_int] + [C.c_double] * 6 + [C.c_bool, C.c_bool, C.c_int, C.c_int, C.c_bool]
    L.post_sw.argtypes = [u32p, C.c_int, C.c_char_p, C.POINTER(gm.SwFullResults)]; L.post_sw.restype = None
    L.gm_free.argtypes = [C.c_void_p]
    K, items, P = fixture(0)
    L.post_sw_setup(POST_MAX_LEN, *K, False, True, 0, 33, True)
    prep = [(np.ascontiguousarray(it["r"]), it["db"].encode(), it["qr"].encode()) for it in items]
    def one(it, r, db, qr):
        d = C.create_string_buffer(db); q = C.create_string_buffer(qr)
        s = gm.SwFullResults(); s.read_start = it["want"][1]; s.dbalign = C.addressof(d); s.qralign = C.addressof(q)
        L.post_sw(r.ctypes.data_as(u32p), it["initbp"], None, C.byref(s)); L.gm_free(s.qual)
        return [s.matches, s.mismatches, s.crossovers]
    for it, (r, db, qr) in list(zip(items, prep))[:100]: one(it, r, db, qr)       # warm-up
    t0 = time.perf_counter()
    counts = [one(it, r, db, qr) for it, (r, db, qr) in zip(items, prep)]
    dt = time.perf_counter() - t0
    assert counts == [[int(x) for x in t[5:8]] for t in P], "single seam: counts differ from the fixture"
    return dict(leg="single", records=len(items), seconds=dt, calls=len(items), lib=os.path.basename(lib_path))


def _batch_inputs(gm, useq, repeat):
    from tests.test_sw_full_batch import pack, run_cs
    K, items, P = fixture(useq)
    gm.sw_full_cs_setup(*CS_SETUP)
    gm.post_sw_setup(POST_MAX_LEN, *K, use_read_qvs=bool(useq), use_sanger_qvs=True, qual_vector_offset=0, qual_delta=33)
    recs, ops, _, _ = run_cs(gm, items); p = pack(items)
    quals = [t[3].encode() for t in P] if useq else None
    if repeat > 1:                                                                 # the fixture `repeat` times over: every copy with its own operations, read and QVs
        n = len(recs); recs = np.tile(recs, repeat); ops = np.tile(ops, repeat)
        recs["ops_off"] += np.repeat(np.arange(repeat, dtype=np.uint64) * np.uint64(ops.size // repeat), n)
        p = dict(p, reads=np.tile(p["reads"], (repeat, 1)), rlen=np.tile(p["rlen"], repeat), initbp=np.tile(p["initbp"], repeat))
        if quals: quals = quals * repeat
    return P, recs, ops, p, quals


def leg_batch(lib_path, loops, repeat):
    os.environ["GM_LIB_PATH"] = lib_path
    from shrimp_amd import gmapper as gm
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    P, recs, ops, p, quals = _batch_inputs(gm, 0, repeat)
    call = lambda: gm.post_sw_batch(recs, ops, p["genome"], p["reads"], p["rlen"], p["initbp"], quals=quals)
    post, _, _ = call(); call()                                                    # warm-up, and the check
    want = [[int(x) for x in t[5:8]] for t in P] * repeat
    assert [[int(r["matches"]), int(r["mismatches"]), int(r["crossovers"])] for r in post] == want, "batch call: counts differ from the fixture"
    n, t0 = 0, time.perf_counter()
    while True:                                                                    # (the call returns after its device synchronise, the copies back and the host's share)
        call(); n += 1
        dt = time.perf_counter() - t0
        if (loops and n >= loops) or (not loops and dt >= 0.5): break
    return dict(leg="batch", records=len(recs), seconds=dt / n, calls=n, window_seconds=dt, by_host=int(post["by_host"].sum()), plan=gm.post_sw_batch_last_plan(),
                lib=os.path.basename(lib_path))


def leg_error(lib_path):
    os.environ["GM_LIB_PATH"] = lib_path
    from shrimp_amd import gmapper as gm
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    out = {}
    for useq in (0, 1):
        P, recs, ops, p, quals = _batch_inputs(gm, useq, 1)
        post, _, _ = gm.post_sw_batch(recs, ops, p["genome"], p["reads"], p["rlen"], p["initbp"], quals=quals)
        ref = np.array([float.fromhex(t[4]) for t in P]); dev = post["by_host"] == 0
        d = np.abs(post["posterior"] - ref) / ref
        assert (post["posterior"][~dev] == ref[~dev]).all()
        out["with_qvs" if useq else "without_qvs"] = dict(records=len(P), by_host=int((~dev).sum()), by_host_share=float((~dev).mean()),
                                                          largest_relative_difference=float(d[dev].max()), bound=1e-9)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    rel = os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so")
    ap.add_argument("--leg", choices=["single", "batch", "error"]); ap.add_argument("--lib", default=rel)
    ap.add_argument("--loops", type=int, default=0); ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--single-lib", default=rel); ap.add_argument("--batch-lib", default=rel)
    ap.add_argument("--runs", type=int, default=3); ap.add_argument("--large-repeat", type=int, default=82); ap.add_argument("--out"); ap.add_argument("--error-out")
    a = ap.parse_args()
    if a.leg:
        lib = os.path.abspath(a.lib)
        r = leg_single(lib) if a.leg == "single" else leg_batch(lib, a.loops, a.repeat) if a.leg == "batch" else leg_error(lib)
        print("RESULT " + json.dumps(r)); return
    def child(*args):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), *args], capture_output=True, text=True, cwd=ROOT, timeout=600)
        if p.returncode != 0: raise SystemExit("%s failed (%d): %s" % (args, p.returncode, (p.stdout + p.stderr)[-2000:]))
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    runs = []
    for k in range(a.runs):
        for args in (("--leg", "single", "--lib", a.single_lib), ("--leg", "batch", "--lib", a.batch_lib), ("--leg", "batch", "--lib", a.batch_lib, "--repeat", str(a.large_repeat))):
            r = child(*args); r["run"] = k; runs.append(r); print(json.dumps(r), flush=True)
    n1 = runs[0]["records"]
    s = [r["seconds"] for r in runs if r["leg"] == "single"]; b = [r["seconds"] for r in runs if r["leg"] == "batch" and r["records"] == n1]
    big = [r for r in runs if r["leg"] == "batch" and r["records"] != n1]
    out = dict(what="post_sw in a loop (a) against one gm_post_sw_batch call (b), seconds for all records of the set; host clock around synchronising calls; no ratio is required",
               runs=runs, fixture=dict(records=n1, single_over_batch_per_run=[x / y for x, y in zip(s, b)]),
               large=dict(records=big[0]["records"] if big else 0, seconds_per_run=[r["seconds"] for r in big],
                          single_loop_scaled_over_batch_per_run=[x * (r["records"] / n1) / r["seconds"] for x, r in zip(s, big)]))
    print(json.dumps(out["fixture"])); print(json.dumps(out["large"]))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")
    if a.error_out:
        e = child("--leg", "error", "--lib", a.batch_lib); print(json.dumps(e))
        with open(a.error_out, "w") as f: json.dump(dict(what="gm_post_sw_batch against the reference's posteriors (tests/golden/sw_kat_post.txt.gz): items the kernel answered "
                                                              "(by_host = 0); items the host routine answered carry the reference's bits", **e), f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
