#!/usr/bin/env python3
"""Time the full-alignment seams on the reference's known-answer records: the single seam called once per record against one batch call.

    python tools/sw_full_batch_timing.py --single-lib OLD.so [--batch-lib NEW.so] [--runs 3] [--out profiles/r06a_sw_full_batch_timing.json]

  (a) sw_full_ls / sw_full_cs in a loop over the records, with the library given by --single-lib (e.g. one built from the parent commit)
  (b) one gm_sw_full_ls_batch / gm_sw_full_cs_batch call over the same records, with --batch-lib (default: the tree's release build)
for the 2 990 letter-space "F" records of tests/golden/sw_kat.txt.gz and the 1 400 colour-space "S" records of sw_kat_cs.txt.gz.  Each timing is a child process
of its own (one library a process), legs alternate a, b, a, b, ...; a child warms up first (code objects, allocator), then takes a host clock around calls that
end in a device synchronise; the batch call is repeated until the window holds at least half a second.  Both legs check their scores against the fixture.

    python tools/sw_full_batch_timing.py --leg batch --space ls --lib NEW.so --loops 20     # the child form, also what a kernel trace is taken of
"""
import argparse, ctypes as C, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


LS_SETUP = (1400, 1000, -33, -7, -33, -3, 10, -15, True, 8)                 # gmapper's default scores, the sizes the known answers were made with
CS_SETUP = (1400, 1000, -33, -7, -33, -3, 10, -24, -20, True, 8, 0)


def records(space):
    """the fixture's records as dicts: genome words, goff, glen, read words, rlen, anchor box, revcmpl, threshold, primer letter, expected score"""
    from tests import oracle_api as oa          # (the fixture readers; bench.py takes its CPU baseline from the same module)
    if space == "ls":
        return [dict(g=r[9], goff=r[1], glen=r[2], r=r[10], rlen=r[3], anchor=tuple(r[4:8]), rv=r[8], thresh=0, initbp=0, score=r[11][0]) for r in oa.load_kat() if r[0] == "F"]
    out = []
    for rec in oa.load_kat_cs("sw_kat_cs.txt.gz"):
        if rec[0] != "S": continue
        (goff, glen, rlen, initbp, ax, ay, alen, aw, rv, thresh), gls, rd, want = rec[1:5]
        out.append(dict(g=gls, goff=goff, glen=glen, r=rd, rlen=rlen, anchor=(ax, ay, alen, aw), rv=rv, thresh=thresh, initbp=initbp, score=want[0]))
    return out


def pack(items):
    """the records' genome bitfields laid end to end (each on a word boundary), the reads padded to one width"""
    base, bases = 0, []
    for it in items: bases.append(base * 8); base += len(it["g"])
    reads = np.zeros((len(items), max(len(it["r"]) for it in items)), dtype=np.uint32)
    for i, it in enumerate(items): reads[i, :len(it["r"])] = it["r"]
    col = lambda k: np.array([it[k] for it in items], dtype=np.int64)
    return dict(genome=np.concatenate([it["g"] for it in items]), g_off=np.array(bases, dtype=np.int64) + col("goff"), glen=col("glen"), rlen=col("rlen"), reads=reads,
                anchors=np.array([it["anchor"] for it in items], dtype=np.int64), rv=col("rv"), thresh=col("thresh"), initbp=col("initbp"))


def leg_single(space, lib_path):
    """the single seam through ctypes on the given library (it may be older than this tree's Python wrapper: only the single seams' symbols are touched)"""
    from shrimp_amd import gmapper as gm
    L = C.CDLL(lib_path); u32p = C.POINTER(C.c_uint32)
    L.sw_full_ls_setup.argtypes = [C.c_int] * 8 + [C.c_bool, C.c_int]
    L.sw_full_ls.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.POINTER(gm.SwFullResults), C.c_bool, C.POINTER(gm.Anchor), C.c_int, C.c_int]; L.sw_full_ls.restype = None
    L.sw_full_cs_setup.argtypes = [C.c_int] * 9 + [C.c_bool, C.c_int, C.c_int]
    L.sw_full_cs.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.POINTER(gm.SwFullResults), C.c_bool, C.c_bool, C.POINTER(gm.Anchor), C.c_int, C.c_int, C.c_void_p]
    L.sw_full_cs.restype = None
    L.gm_free.argtypes = [C.c_void_p]
    if L.gm_device_count() < 1: raise SystemExit("no HIP device")
    items = records(space)
    prep = [(np.ascontiguousarray(it["g"]), np.ascontiguousarray(it["r"]), gm.Anchor(*it["anchor"], 1, 0, 0)) for it in items]
    if space == "ls": L.sw_full_ls_setup(*LS_SETUP)
    else: L.sw_full_cs_setup(*CS_SETUP)
    def one(it, g, r, a):
        s = gm.SwFullResults()
        if space == "ls":
            L.sw_full_ls(g.ctypes.data_as(u32p), it["goff"], it["glen"], r.ctypes.data_as(u32p), it["rlen"], 0, 0, C.byref(s), bool(it["rv"]), C.byref(a), 1, 0)
        else:
            L.sw_full_cs(g.ctypes.data_as(u32p), it["goff"], it["glen"], r.ctypes.data_as(u32p), it["rlen"], it["initbp"], it["thresh"], C.byref(s), bool(it["rv"]), False,
                         C.byref(a), 1, 0, None)
        L.gm_free(s.dbalign); L.gm_free(s.qralign)
        return s.score
    for it, (g, r, a) in list(zip(items, prep))[:100]: one(it, g, r, a)            # warm-up
    t0 = time.perf_counter()
    scores = [one(it, g, r, a) for it, (g, r, a) in zip(items, prep)]              # (every call ends in its own device synchronise)
    dt = time.perf_counter() - t0
    assert scores == [it["score"] for it in items], "single seam: scores differ from the fixture"
    return dict(leg="single", space=space, records=len(items), seconds=dt, calls=len(items), lib=os.path.basename(lib_path))


def leg_batch(space, lib_path, loops):
    os.environ["GM_LIB_PATH"] = lib_path
    from shrimp_amd import gmapper as gm
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    items = records(space); p = pack(items)
    if space == "ls":
        gm.sw_full_ls_setup(*LS_SETUP)
        call = lambda: gm.sw_full_ls_batch(p["genome"], p["g_off"], p["glen"], p["reads"], p["rlen"], p["anchors"], p["rv"], p["thresh"])
    else:
        gm.sw_full_cs_setup(*CS_SETUP)
        call = lambda: gm.sw_full_cs_batch(p["genome"], p["g_off"], p["glen"], p["reads"], p["rlen"], p["initbp"], p["anchors"], p["rv"], p["thresh"])
    recs, _, _ = call(); call()                                                   # warm-up, and the check
    assert [int(s) for s in recs["score"]] == [it["score"] for it in items], "batch call: scores differ from the fixture"
    n, t0 = 0, time.perf_counter()
    while True:                                                                   # (the call returns after its device synchronise and the copies back)
        call(); n += 1
        dt = time.perf_counter() - t0
        if (loops and n >= loops) or (not loops and dt >= 0.5): break
    return dict(leg="batch", space=space, records=len(items), seconds=dt / n, calls=n, window_seconds=dt, lib=os.path.basename(lib_path))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=["single", "batch"]); ap.add_argument("--space", choices=["ls", "cs"], default="ls"); ap.add_argument("--lib")
    ap.add_argument("--loops", type=int, default=0)
    ap.add_argument("--single-lib"); ap.add_argument("--batch-lib", default=os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    ap.add_argument("--runs", type=int, default=3); ap.add_argument("--out")
    a = ap.parse_args()
    if a.leg:
        r = leg_single(a.space, os.path.abspath(a.lib)) if a.leg == "single" else leg_batch(a.space, os.path.abspath(a.lib), a.loops)
        print("RESULT " + json.dumps(r)); return
    if not a.single_lib: ap.error("--single-lib is required")
    runs = []
    for space in ("ls", "cs"):
        for k in range(a.runs):
            for leg, lib in (("single", a.single_lib), ("batch", a.batch_lib)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--space", space, "--lib", lib], capture_output=True, text=True, cwd=ROOT, timeout=600)
                if p.returncode != 0: raise SystemExit("leg %s/%s failed (%d): %s" % (leg, space, p.returncode, (p.stdout + p.stderr)[-2000:]))
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]); r["run"] = k
                runs.append(r); print(json.dumps(r), flush=True)
    out = dict(what="single seam in a loop (a) against one batch call (b), seconds for all records of the set; host clock around synchronising calls", runs=runs, ratio={})
    for space in ("ls", "cs"):
        s = [r["seconds"] for r in runs if r["space"] == space and r["leg"] == "single"]; b = [r["seconds"] for r in runs if r["space"] == space and r["leg"] == "batch"]
        out["ratio"][space] = dict(per_run=[x / y for x, y in zip(s, b)], batch_faster_in_every_run=all(y < x for x, y in zip(s, b)))
    print(json.dumps(out["ratio"]))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
