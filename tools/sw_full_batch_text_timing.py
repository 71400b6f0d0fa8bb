#!/usr/bin/env python3
"""Time the text of a chunk's alignments: gm_sw_full_batch_strings once per item on the host against one gm_sw_full_batch_text call.

    python tools/sw_full_batch_text_timing.py [--runs 3] [--items 100000] [--out profiles/r09a_sw_full_batch_text_timing.json]

The records are the reference's known answers (tests/golden/sw_kat*.txt.gz) through their batch SW call, repeated to --items: the 2 990 letter-space records
(ls), the same on an Index of their genomes (ls_ix) and the 1 400 colour-space records (cs).
  (a) loop:  gm_sw_full_batch_strings and two gm_free calls per item, driven through ctypes with every pointer prepared beforehand.  ls_ix: the one
             gm_index_get_windows call a caller without a host genome needs, and the copy of the records with genome_start moved onto the windows, are inside the
             clock.  The cost of 3 x items empty ctypes calls is measured beside it (call_overhead_seconds): a C caller would not pay that part.
  (b) batch: one gm_sw_full_batch_text call with what = GM_TEXT_ALIGN -- the same strings as (a) -- and, reported on its own because (a) has neither, one with what = 7
             (strings, CIGAR, edit string).
Each timing is a child process of its own on the release library, legs alternate a, b, a, b, ...; a child warms up first, then takes a host clock around calls that
end in a device synchronise, repeated until the window holds half a second (the loop: once).  A child prints a digest of every item's two strings; the legs' digests
must be equal.  Every child runs under its own time limit and the first one that fails ends the run.

    python tools/sw_full_batch_text_timing.py --leg batch --set ls      # the child form, also what a kernel trace is taken of
"""
import argparse, ctypes as C, hashlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
CHILD_LIMIT = 300
SETS = ("ls", "ls_ix", "cs")


def inputs(gm, which, n_items):
    """the set's records through its batch SW call, tiled to n_items (the copies share their operations, as the entries allow)"""
    from tests.test_sw_full_batch import LS_SETUP, CS_SETUP, items_F, items_cs, pack, run_ls, run_cs
    d = dict(colour=which == "cs", ix=None)
    if which == "cs":
        items = items_cs("sw_kat_cs.txt.gz", "S"); gm.sw_full_cs_setup(*CS_SETUP)
        recs, ops, _, _ = run_cs(gm, items); p = pack(items)
        d.update(genome=p["genome"], reads=p["reads"], rlen=p["rlen"].astype(np.int32), initbp=p["initbp"].astype(np.uint8))
    elif which == "ls":
        items = items_F(); gm.sw_full_ls_setup(*LS_SETUP)
        recs, ops, _, _ = run_ls(gm, items); p = pack(items)
        d.update(genome=p["genome"], reads=p["reads"], rlen=p["rlen"].astype(np.int32), initbp=None)
    else:
        from tests import test_seam_batch_ix as tx
        items = items_F(); gm.sw_full_ls_setup(*LS_SETUP)
        contigs, cn, base = tx.lay_out([it["g"] for it in items])
        ix = gm.Index(contigs, seeds=["1111111111"]); a = tx.arrays(items)
        st = np.zeros(len(items), dtype=np.uint8)
        recs, ops, _ = ix.sw_full_ls_batch(cn, st, base + a["goff"], a["glen"], a["reads"], a["rlen"], a["anchors"], a["rv"], a["thresh"], a["maxscore"])
        d.update(ix=ix, cn=cn, st=st, g_off=base + a["goff"], glen=a["glen"].astype(np.int32), reads=a["reads"], rlen=a["rlen"].astype(np.int32), initbp=None)
    order = np.resize(np.arange(len(recs)), n_items)
    d.update(recs=np.ascontiguousarray(recs[order]), ops=ops, reads=np.ascontiguousarray(d["reads"][order]), rlen=d["rlen"][order], initbp=None if d["initbp"] is None else d["initbp"][order])
    if d["ix"] is not None:
        for k in ("cn", "st", "g_off", "glen"): d[k] = np.ascontiguousarray(d[k][order])
    return d


def digest(strings):
    h = hashlib.sha1()
    for db, qr in strings: h.update(db); h.update(b"|"); h.update(qr); h.update(b"\n")
    return h.hexdigest()


def leg_loop(gm, d):
    L = gm.lib(); u32p = C.POINTER(C.c_uint32); n = len(d["recs"])
    ops = d["ops"]; rsz = d["recs"].dtype.itemsize; rw = d["reads"].shape[1]
    rptr = [C.cast(d["reads"].ctypes.data + i * rw * 4, u32p) for i in range(n)]
    def once():
        t0 = time.perf_counter()
        if d["ix"] is not None:                                                       # the windows, and the records moved onto them
            words = d["ix"].get_windows(d["cn"], d["st"], d["g_off"], d["glen"]); recs = d["recs"].copy(); recs["genome_start"] -= d["g_off"]
            gstride = words.shape[1] * 4; glen = words.shape[1] * 8; gbase = words.ctypes.data
        else:
            recs = d["recs"]; g = d["genome"]; gstride = 0; glen = g.size * 8; gbase = g.ctypes.data; gptr = C.cast(gbase, u32p)
        rbase, opp = recs.ctypes.data, ops.ctypes.data
        db, qr = C.c_void_p(), C.c_void_p(); pdb, pqr = C.byref(db), C.byref(qr)
        fn, free, at = L.gm_sw_full_batch_strings, L.gm_free, C.string_at
        colour = 1 if d["colour"] else 0; rl = d["rlen"].tolist(); ib = [0] * n if d["initbp"] is None else d["initbp"].tolist()
        out = []
        for i in range(n):
            rc = fn(colour, rbase + i * rsz, opp, ops.size, C.cast(gbase + i * gstride, u32p) if gstride else gptr, glen, rptr[i], rl[i], ib[i], 0, pdb, pqr)
            if rc: raise SystemExit("gm_sw_full_batch_strings failed on item %d" % i)
            out.append((at(db.value) if db.value else b"", at(qr.value) if qr.value else b""))
            free(db); free(qr)
        return time.perf_counter() - t0, out
    once()                                                                            # warm-up
    dt, strings = once()
    f = L.gm_abi_sizeof
    t0 = time.perf_counter()
    for i in range(3 * n): f(6)
    return dict(seconds=dt, call_overhead_seconds=time.perf_counter() - t0, digest=digest(strings))


def leg_batch(gm, d):
    n = len(d["recs"])
    def call(what):
        if d["ix"] is not None: return d["ix"].sw_full_batch_text(d["cn"], d["st"], d["recs"], d["ops"], d["reads"], d["rlen"], what=what)
        return gm.sw_full_batch_text(d["colour"], d["recs"], d["ops"], d["genome"], d["reads"], d["rlen"], initbp=d["initbp"], what=what)
    out = {}
    for name, what in (("align", ("align",)), ("all", ("align", "cigar", "edit"))):
        got = call(what); call(what)                                                  # warm-up, and the strings the legs are compared by
        if (got[0] != 0).any(): raise SystemExit("an item was refused")
        k, t0 = 0, time.perf_counter()
        while True:
            call(what); k += 1
            dt = time.perf_counter() - t0
            if dt >= 0.5 and k >= 3: break
        out["seconds_" + name] = dt / k; out["calls_" + name] = k
        if name == "align": out["digest"] = digest((got[1](i), got[2](i)) for i in range(n))
        else: out["cigar_bytes"] = len(got[3].buffer); out["edit_bytes"] = len(got[4].buffer)
    return out


def child(leg, which, n_items):
    os.environ.setdefault("GM_LIB_PATH", os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    from shrimp_amd import gmapper as gm
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    d = inputs(gm, which, n_items)
    r = leg_loop(gm, d) if leg == "loop" else leg_batch(gm, d)
    print("RESULT " + json.dumps(dict(leg=leg, set=which, items=n_items, **r)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=["loop", "batch"]); ap.add_argument("--set", choices=SETS, default="ls")
    ap.add_argument("--items", type=int, default=100_000); ap.add_argument("--runs", type=int, default=3); ap.add_argument("--sets", nargs="+", default=list(SETS)); ap.add_argument("--out")
    a = ap.parse_args()
    if a.leg: child(a.leg, a.set, a.items); return
    runs = []
    for which in a.sets:
        for k in range(a.runs):
            for leg in ("loop", "batch"):
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--leg", leg, "--set", which, "--items", str(a.items)],
                                   capture_output=True, text=True, cwd=ROOT)
                if p.returncode != 0: raise SystemExit("leg %s of %s failed (%d): %s" % (leg, which, p.returncode, (p.stdout + p.stderr)[-2000:]))
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                r["run"] = k; runs.append(r); print(json.dumps(r), flush=True)
    out = dict(what="seconds for the strings of %d alignments: gm_sw_full_batch_strings per item (loop) against one gm_sw_full_batch_text call (batch; seconds_all: with CIGAR and "
                    "edit string); host clock around synchronising calls, release library" % a.items, runs=runs, summary={})
    for which in a.sets:
        lo = [r for r in runs if r["set"] == which and r["leg"] == "loop"]; ba = [r for r in runs if r["set"] == which and r["leg"] == "batch"]
        if len({r["digest"] for r in lo + ba}) != 1: raise SystemExit("%s: the legs' strings differ" % which)
        out["summary"][which] = dict(loop_seconds=[r["seconds"] for r in lo], loop_call_overhead_seconds=[r["call_overhead_seconds"] for r in lo],
                                     batch_align_seconds=[r["seconds_align"] for r in ba], batch_all_seconds=[r["seconds_all"] for r in ba],
                                     loop_over_batch_align_per_run=[x["seconds"] / y["seconds_align"] for x, y in zip(lo, ba)],
                                     loop_less_call_overhead_over_batch_align_per_run=[(x["seconds"] - x["call_overhead_seconds"]) / y["seconds_align"] for x, y in zip(lo, ba)])
    print(json.dumps(out["summary"], indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
