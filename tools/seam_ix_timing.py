#!/usr/bin/env python3
"""Time the batch seams on a genome of real size: the host-bitfield entries (which upload the genome with every call) against their index-resident forms.

    python tools/seam_ix_timing.py [--mbp 2 512] [--runs 3] [--out profiles/r08a_seam_ix_timing.json]

100 000 windows of 140 positions against 100-base reads on a synthetic genome (shrimp_amd/synth.py, two contigs), strand 0 only -- the host-bitfield entries cannot
express the other:
  (a) gm_sw_vector_batch / gm_sw_full_ls_batch on the host bitfield of the whole genome
  (b) gm_sw_vector_batch_ix / gm_sw_full_ls_batch_ix on an Index built from it (one seed: the seams use none)
Each timing is a child process of its own on the release library, legs alternate a, b, a, b, ...; a child warms up first, then takes a host clock around calls that
end in a device synchronise, repeated until the window holds half a second.  A child prints a digest of its scores; the two legs' digests must be equal.  Every
child runs under its own time limit and the first one that fails ends the run.

    python tools/seam_ix_timing.py --leg ix --one-mbp 512      # the child form
"""
import argparse, hashlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
N_WINDOWS, GLEN, RLEN = 100_000, 140, 100
LS_SETUP = (1400, 1000, -33, -7, -33, -3, 10, -15, True, 8)
CHILD_LIMIT = 420                      # seconds: the 512 Mbp child generates, packs and (leg b) indexes the genome before it times anything


def workload(mbp):
    from shrimp_amd import synth
    half = mbp * 1_000_000 // 2 // 8 * 8                         # (a multiple of 8: the contigs' bitfields laid end to end are the one forward bitfield the entries take)
    contigs = synth.make_genome([half, half], seed=81)
    rng = np.random.default_rng(82)
    cn = rng.integers(0, 2, size=N_WINDOWS).astype(np.int32); off = rng.integers(0, half - GLEN, size=N_WINDOWS).astype(np.int64)
    idx = off[:, None] + 20 + np.arange(RLEN)[None, :]
    reads = np.where(cn[:, None] == 0, contigs[0][idx], contigs[1][idx])
    reads = np.where(rng.random(reads.shape) < 0.05, rng.integers(0, 4, size=reads.shape), reads).astype(np.uint8)
    return contigs, half, cn, off, synth.pack_reads(reads)


def child(leg, mbp):
    os.environ.setdefault("GM_LIB_PATH", os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    from shrimp_amd import gmapper as gm, synth
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    contigs, half, cn, off, rw = workload(mbp)
    glen = np.full(N_WINDOWS, GLEN, dtype=np.int32); rlen = np.full(N_WINDOWS, RLEN, dtype=np.int32)
    anchors = np.tile(np.array([20, 0, RLEN, 1], dtype=np.int64), (N_WINDOWS, 1)); zeros = np.zeros(N_WINDOWS, dtype=np.int64)
    gm.sw_vector_setup(1400, 1000, -33, -7, -33, -3, 10, -15, 0, True); gm.sw_full_ls_setup(*LS_SETUP)
    build_s = 0.0
    if leg == "host":
        genome = np.concatenate([synth.pack_nibbles(c) for c in contigs]); g_off = cn.astype(np.int64) * half + off
        calls = dict(vector=lambda: gm.sw_vector_batch(genome, g_off, glen, rw, rlen),
                     full_ls=lambda: gm.sw_full_ls_batch(genome, g_off, glen, rw, rlen, anchors, zeros, zeros)[0]["score"])
        moved = int(genome.nbytes)
    else:
        t0 = time.perf_counter(); ix = gm.Index(contigs, seeds=["1111111111"]); build_s = time.perf_counter() - t0
        st = np.zeros(N_WINDOWS, dtype=np.uint8)
        calls = dict(vector=lambda: ix.sw_vector_batch(cn, st, off, glen, rw, rlen),
                     full_ls=lambda: ix.sw_full_ls_batch(cn, st, off, glen, rw, rlen, anchors, zeros, zeros)[0]["score"])
        moved = 0
    out = []
    for entry, call in calls.items():
        scores = np.asarray(call(), dtype=np.int32); call()                                 # warm-up, and the scores the legs are compared by
        n, t0 = 0, time.perf_counter()
        while True:
            call(); n += 1
            dt = time.perf_counter() - t0
            if dt >= 0.5 and n >= 3: break
        out.append(dict(leg=leg, mbp=mbp, entry=entry, seconds=dt / n, calls=n, genome_bytes_per_call=moved, index_build_seconds=build_s,
                        digest=hashlib.sha1(scores.tobytes()).hexdigest(), mean_score=float(scores.mean())))
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--leg", choices=["host", "ix"]); ap.add_argument("--one-mbp", type=int)
    ap.add_argument("--mbp", type=int, nargs="+", default=[2, 512]); ap.add_argument("--runs", type=int, default=3); ap.add_argument("--out")
    a = ap.parse_args()
    if a.leg: child(a.leg, a.one_mbp); return
    runs = []
    for mbp in a.mbp:
        for k in range(a.runs):
            for leg in ("host", "ix"):
                p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--leg", leg, "--one-mbp", str(mbp)],
                                   capture_output=True, text=True, cwd=ROOT)
                if p.returncode != 0: raise SystemExit("leg %s at %d Mbp failed (%d): %s" % (leg, mbp, p.returncode, (p.stdout + p.stderr)[-2000:]))
                for r in json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]):
                    r["run"] = k; runs.append(r); print(json.dumps(r), flush=True)
    out = dict(what="seconds a call of %d windows of %d positions against %d-base reads; host clock around synchronising calls, release library" % (N_WINDOWS, GLEN, RLEN),
               runs=runs, summary={})
    for mbp in a.mbp:
        for entry in ("vector", "full_ls"):
            sel = lambda leg: [r for r in runs if r["mbp"] == mbp and r["entry"] == entry and r["leg"] == leg]
            h, x = sel("host"), sel("ix")
            if len({r["digest"] for r in h + x}) != 1: raise SystemExit("%s at %d Mbp: the legs' scores differ" % (entry, mbp))
            out["summary"]["%s@%dMbp" % (entry, mbp)] = dict(host_seconds=[r["seconds"] for r in h], ix_seconds=[r["seconds"] for r in x],
                                                              ratio_per_run=[p["seconds"] / q["seconds"] for p, q in zip(h, x)],
                                                              host_genome_bytes_per_call=h[0]["genome_bytes_per_call"], ix_genome_bytes_per_call=0)
    print(json.dumps(out["summary"], indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
