#!/usr/bin/env python3
"""Time gm_read_windows on a genome of real size against what a seam caller pays for the same windows today: the front of the read loop on the CPU.

    python tools/read_windows_timing.py [--genomes cfg2 cfg3] [--runs 3] [--driver-genomes cfg2] [--out profiles/r10a_read_windows_timing.json]

131 072 reads of 100 bases (bench.py's generator) on bench.py's cfg2 genome (4 x 25 Mbp), optionally cfg3 (3 Gbp):
  lib     one gm_read_windows call, host clock around the C call (it ends in a device synchronise), repeated until the window holds half a second; then gm_map_reads
          on the same session and reads, whose ms_lookup + ms_anchors is the front alone: the difference is the export and the copies
  driver  tests/read_windows_oracle.cpp (the CPU restatement's read loop up to read_get_hit_list, compiled into a temporary directory) on the same reads, 16 threads
Each timing is a child process of its own on the release library, legs alternate lib, driver, lib, ...; a child warms up first.  A child prints the number of windows
and a digest of its rows (groups of equal (read, st, cn, g_off) ordered by the whole record); the legs' digests must be equal.  Every child runs under its own time
limit and the first one that fails ends the run.  Under `rocprofv3 --kernel-trace --stats -- python tools/read_windows_timing.py --leg lib --one cfg2` the export
kernels' own time (k_win_scan, k_win_scatter) is in the trace summary.

    python tools/read_windows_timing.py --leg lib --one cfg2      # the child form
"""
import argparse, ctypes as C, hashlib, json, os, re, subprocess, sys, tempfile, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
N_READS, RLEN, THREADS = 131072, 100, 16
GENOMES = {"cfg2": 2, "cfg3": 3}       # bench.py's genome seeds
CHILD_LIMIT = 540                      # seconds: the 3 Gbp child generates the genome and builds its index before it times anything
COLS = ("read", "st", "cn", "g_off", "w_len", "score_window_gen", "matches", "ax", "ay", "alen", "awidth", "reserved")


def workload(gname):
    from shrimp_amd import synth
    contigs = synth.make_genome(synth.contig_lengths(gname, 1.0), GENOMES[gname])
    reads, _ = synth.make_reads(contigs, N_READS, RLEN, 20261019)
    return contigs, np.ascontiguousarray(reads, dtype=np.uint8)


def digest(rows):
    return hashlib.sha1(np.ascontiguousarray(rows[np.lexsort(rows.T[::-1])]).tobytes()).hexdigest()


def child_lib(gname):
    os.environ.setdefault("GM_LIB_PATH", os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    from shrimp_amd import gmapper as gm, synth
    L = gm.lib()
    if L.gm_device_count() < 1: raise SystemExit("no HIP device")
    contigs, reads = workload(gname)
    t0 = time.perf_counter(); ix = gm.Index(contigs); build_s = time.perf_counter() - t0
    s = gm.Session(ix)
    wins, off = s.read_windows(reads); st_rw = dict(s.stats)                                 # warm-up, and the rows the legs are compared by
    s.map_reads(reads)
    packed = np.ascontiguousarray(synth.pack_reads(reads), dtype=np.uint32); offs = np.zeros(2 * N_READS + 1, dtype=np.uint64)
    out = C.c_void_p(); nw = C.c_uint64(); st = gm.MapStats(); front = []

    def call():
        rc = L.gm_read_windows(s.h, N_READS, RLEN, packed.ctypes.data_as(C.POINTER(C.c_uint32)), None, C.byref(out), C.byref(nw), offs.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st))
        if rc: raise SystemExit("gm_read_windows: %d" % rc)
    n, t0 = 0, time.perf_counter()
    while True:
        call(); t1 = time.perf_counter()
        L.gm_free(out); front.append(st.ms_lookup + st.ms_anchors); n += 1
        t0 += time.perf_counter() - t1                                                       # (the release of the buffer is not part of the call)
        dt = time.perf_counter() - t0
        if dt >= 0.5 and n >= 3: break
    maps = []
    for _ in range(3):
        s.map_reads(reads); maps.append(s.stats["ms_lookup"] + s.stats["ms_anchors"])
    rows = np.stack([wins[c].astype(np.int64) for c in COLS], axis=1)
    print("RESULT " + json.dumps(dict(leg="lib", genome=gname, seconds=dt / n, calls=n, windows=int(len(wins)), retries=int(st_rw["retries"]),
                                      read_windows_front_ms=front, map_reads_front_ms=maps, index_build_seconds=build_s, bytes_out=int(wins.nbytes + off.nbytes),
                                      kernel=L.gm_last_lookup_kernel().decode(), digest=digest(rows))))


def child_driver(gname):
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1).split()
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "librwo.so")
        subprocess.run(["g++", *flags, "-shared", "-fPIC", "-I", os.path.join(ROOT, "oracle"), "-o", so, os.path.join(ROOT, "tests", "read_windows_oracle.cpp")], check=True)
        L = C.CDLL(so)
        u8p = C.POINTER(C.c_uint8)
        L.rwo_create.argtypes = [C.c_int, C.POINTER(u8p), C.POINTER(C.c_uint64), C.c_int, C.c_int]; L.rwo_create.restype = C.c_void_p
        L.rwo_windows.argtypes = [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int, C.POINTER(C.c_longlong), C.c_long]; L.rwo_windows.restype = C.c_long
        L.rwo_destroy.argtypes = [C.c_void_p]
        contigs, reads = workload(gname)
        cs = [np.ascontiguousarray(c, dtype=np.uint8) for c in contigs]
        os.environ["OMP_NUM_THREADS"] = str(THREADS)
        t0 = time.perf_counter()
        h = L.rwo_create(len(cs), (u8p * len(cs))(*[c.ctypes.data_as(u8p) for c in cs]), (C.c_uint64 * len(cs))(*[len(c) for c in cs]), 0, 2)
        build_s = time.perf_counter() - t0
        cap = 16 * N_READS; rows = np.zeros((cap, 12), dtype=np.int64)
        run = lambda n: L.rwo_windows(h, n, RLEN, reads.ctypes.data_as(u8p), THREADS, rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
        run(4096)                                                                            # warm-up: the threads' region maps
        t0 = time.perf_counter(); w = run(N_READS); dt = time.perf_counter() - t0
        L.rwo_destroy(h)
        if not 0 < w <= cap: raise SystemExit("driver: %d rows" % w)
        print("RESULT " + json.dumps(dict(leg="driver", genome=gname, seconds=dt, calls=1, windows=int(w), threads=THREADS, index_build_seconds=build_s, digest=digest(rows[:w]))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=["lib", "driver"]); ap.add_argument("--one", choices=sorted(GENOMES))
    ap.add_argument("--genomes", nargs="+", default=["cfg2"], choices=sorted(GENOMES)); ap.add_argument("--driver-genomes", nargs="*", default=["cfg2"], choices=sorted(GENOMES))
    ap.add_argument("--runs", type=int, default=3); ap.add_argument("--out")
    a = ap.parse_args()
    if a.leg: (child_lib if a.leg == "lib" else child_driver)(a.one); return
    runs = []
    for g in a.genomes:
        for k in range(a.runs):
            for leg in ("lib", "driver"):
                if leg == "driver" and g not in a.driver_genomes: continue
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--leg", leg, "--one", g], capture_output=True, text=True, cwd=ROOT)
                if p.returncode != 0: raise SystemExit("leg %s on %s failed (%d): %s" % (leg, g, p.returncode, (p.stdout + p.stderr)[-2000:]))
                r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
                r["run"] = k; runs.append(r); print(json.dumps(r), flush=True)
    out = dict(what="%d reads of %d bases; lib: seconds a gm_read_windows call (host clock around the synchronising C call, release library) and the front's device time "
                    "(ms_lookup + ms_anchors) inside it and inside gm_map_reads on the same reads; driver: seconds of tests/read_windows_oracle.cpp on %d host threads"
                    % (N_READS, RLEN, THREADS), runs=runs, summary={})
    for g in a.genomes:
        lib = [r for r in runs if r["genome"] == g and r["leg"] == "lib"]; drv = [r for r in runs if r["genome"] == g and r["leg"] == "driver"]
        if len({(r["digest"], r["windows"]) for r in lib + drv}) != 1: raise SystemExit("%s: the legs' windows differ" % g)
        e = dict(windows=lib[0]["windows"], read_windows_ms=[1e3 * r["seconds"] for r in lib],
                 map_reads_front_ms=[min(r["map_reads_front_ms"]) for r in lib], read_windows_front_ms=[min(r["read_windows_front_ms"]) for r in lib],
                 export_and_copy_ms=[1e3 * r["seconds"] - min(r["map_reads_front_ms"]) for r in lib], reads_per_second=[N_READS / r["seconds"] for r in lib])
        if drv: e.update(driver_seconds=[r["seconds"] for r in drv], driver_reads_per_second=[N_READS / r["seconds"] for r in drv],
                         ratio_per_run=[d["seconds"] / l["seconds"] for d, l in zip(drv, lib)])
        out["summary"][g] = e
    print(json.dumps(out["summary"], indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
