#!/usr/bin/env python3
"""Genome file -> resident bitfield: gm_index_build_fasta (A) against gm_index_build on the same genome already packed in memory (B), on one MI355X.

    python tools/fasta_build_timing.py --bases 3000000000 --out profiles/NAME.json [--parent-lib PATH/libgmapper_hip.so] [--gzip]

A = seconds of gm_index_build_fasta up to the point where gm_index_build_device starts (gm_index_build_timing), and of the whole call; the genome is written by
synth.write_fasta_genome (70-column lines) and read once before the timed runs, so the page cache is warm.  B = gm_index_build
(whole call: index_prepare's host re-pack + blocking upload, then the device build; no parsing at all, which flatters B).  With --parent-lib, B runs against that library (one built from the parent
commit).  gm_index_build has no timer, so B is the whole call only; its device build runs the same kernels as A's (their time is in the kernel trace).  One untimed run of each, then three of each, alternating; every run is a child process of its own.
Under `rocprofv3 --kernel-trace --stats -- python tools/fasta_build_timing.py --one A ...` the kernels' own time is in the trace summary."""
import argparse, ctypes as C, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def lengths(bases):
    n = max(1, bases // 150_000_000)
    return [bases // n] * n


def one(kind, fasta, bases):
    from shrimp_amd import gmapper as gm, synth
    L = gm.lib() if kind == "A" else C.CDLL(gm.LIB_PATH)          # (B may run against a library of the parent commit, which lacks the new symbols)
    if kind == "A":
        t0 = time.perf_counter(); ix = gm.Index.from_fasta([fasta]); wall = time.perf_counter() - t0
    else:
        contigs = synth.make_genome(lengths(bases), 7)
        packed = [np.ascontiguousarray(gm.pack_codes(c)) for c in contigs]
        n = len(contigs); u32p = C.POINTER(C.c_uint32)
        ptrs = (u32p * n)(*[p.ctypes.data_as(u32p) for p in packed]); lens = (C.c_uint32 * n)(*[len(c) for c in contigs])
        del contigs
        h = C.c_void_p(); par = gm.Params(); L.gm_params_default(C.byref(par)); L.gm_last_error.restype = C.c_char_p
        t0 = time.perf_counter(); rc = L.gm_index_build(C.byref(h), 0, n, ptrs, lens, None, 0, None, C.byref(par)); wall = time.perf_counter() - t0
        assert rc == 0, L.gm_last_error()
    res = {"kind": kind, "call_s": wall}
    if kind == "A":
        a, b = C.c_double(), C.c_double(); L.gm_index_build_timing(ix.h, C.byref(a), C.byref(b)); res["to_bitfield_s"] = a.value
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=3_000_000_000); ap.add_argument("--out"); ap.add_argument("--parent-lib"); ap.add_argument("--gzip", action="store_true")
    ap.add_argument("--fasta", default="/tmp/gm_timing_genome.fa"); ap.add_argument("--one", choices=["A", "B"]); ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    if not os.path.exists(a.fasta):
        from shrimp_amd import synth
        synth.write_fasta_genome(a.fasta, synth.make_genome(lengths(a.bases), 7))
    if a.one:
        return one(a.one, a.fasta, a.bases)
    with open(a.fasta, "rb") as f:                      # warm the page cache
        while f.read(1 << 26): pass
    def child(kind, fasta=a.fasta):
        env = dict(os.environ)
        if kind == "B" and a.parent_lib: env["GM_LIB_PATH"] = a.parent_lib
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, "--fasta", fasta, "--bases", str(a.bases)], capture_output=True, text=True, env=env, timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    child("A"); child("B")
    runs = []
    for _ in range(a.runs):
        runs += [child("A"), child("B")]
    A = [r for r in runs if r["kind"] == "A"]; B = [r for r in runs if r["kind"] == "B"]
    out = {"bases": a.bases, "fasta_bytes": os.path.getsize(a.fasta), "parent_lib": bool(a.parent_lib), "A": A, "B": B,
           "A_to_bitfield_s": sorted(r["to_bitfield_s"] for r in A), "A_device_build_s": sorted(r["call_s"] - r["to_bitfield_s"] for r in A),
           "A_call_s": sorted(r["call_s"] for r in A), "B_call_s": sorted(r["call_s"] for r in B)}
    if a.gzip:
        gz = a.fasta + ".gz"
        if not os.path.exists(gz): subprocess.run("gzip -1 -c %s > %s" % (a.fasta, gz), shell=True, check=True)
        out["A_gzip"] = [child("A", gz) for _ in range(2)][1:]
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
