#!/usr/bin/env python3
"""Time a chunk of read pairs to mapping arrays (gm_pair_mappings) beside the mapping entry on the same session and pairs (gm_map_pairs).

    python tools/pair_mappings_timing.py [--runs 3] [--out profiles/r23a_pair_mappings_timing.json]

65 536 pairs of 2 x 100 bases (synth.make_pairs, -I 0,1000 opp-in) on bench.py's cfg2 genome (4 x 25 Mbp), letter space, the release library.  Two legs on one session:
  (a) one gm_pair_mappings call: arrays, the pair selection on the device, one sub-batch after the other;
  (b) one gm_map_pairs call: SAM text, the pair selection on the host threads, the text of a sub-batch written beside the device work of the next.
Both are timed with the host clock around the synchronising Python wrappers, best of three after a warm-up of both; the legs alternate, and every other child starts
with (b).  The two figures stand side by side and nothing is claimed from them: one prints text and overlaps its output with the next sub-batch, the other does not.
Each run is a child process of its own under its own time limit; the first child that fails ends the run.  The arrays' digest must agree between the runs.
A last child (--laps) runs both entries once more on the library with the tuning knobs under GM_TIMING=1 and sums the stage laps the library prints: "host pair select"
(gm_map_pairs: hit_run_post_sw and pair_pass2 per pair on the host threads) and "device pair select" (gm_pair_mappings: hit_run_post_sw on the host threads, the scores
up, k_pair_sel_items and k_sel_pair_pass2, the pairs down, compute_paired_hit) -- whole stages, each with its synchronisation.
Under `rocprofv3 --kernel-trace --stats -- python tools/pair_mappings_timing.py --child --only a` the new kernels' own times are in the trace summary.

    python tools/pair_mappings_timing.py --child [--b-first] [--only a|b]      # the child form
"""
import argparse, hashlib, json, os, re, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
N_PAIRS, RLEN, REPEATS = 65536, 100, 3
CHILD_LIMIT = 420


def setup(release):
    if release: os.environ.setdefault("GM_LIB_PATH", os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    from shrimp_amd import gmapper as gm, synth
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    contigs = synth.make_genome(synth.contig_lengths("cfg2", 1.0), 2)
    mates, _ = synth.make_pairs(contigs, N_PAIRS, RLEN, 20261021)
    m1 = np.ascontiguousarray(mates[0::2], dtype=np.uint8); m2 = np.ascontiguousarray(mates[1::2], dtype=np.uint8)
    p = gm.default_params()
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    return gm, s, m1, m2, gm.PairOpts.default("opp-in", 0, 1000)


def digest_of(pm):
    h = hashlib.sha1()
    for a in [pm.pmaps, pm.pmap_off] + [x[m] for m in (0, 1) for x in (pm.hits, pm.hit_off, pm.recs, pm.umaps, pm.umap_off, pm.cigar_off)]: h.update(np.ascontiguousarray(a).tobytes())
    h.update(pm.cigar_buf[0]); h.update(pm.cigar_buf[1])
    return h.hexdigest()


def child(b_first, only):
    gm, s, m1, m2, opts = setup(True)
    times = {}; got = {}

    def timed(name, f):
        t0 = time.perf_counter(); r = f(); times.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    def leg_a(): got["a"] = timed("a: gm_pair_mappings", lambda: s.pair_mappings(m1, m2, opts)); got["a_stats"] = dict(s.stats)
    def leg_b(): got["b"] = timed("b: gm_map_pairs", lambda: s.map_pairs(m1, m2, opts=opts)); got["b_stats"] = dict(s.stats)
    legs = [l for l in ((leg_b, leg_a) if b_first else (leg_a, leg_b)) if only in (None, l.__name__[-1])]
    for _ in range(1 + REPEATS):
        for leg in legs: leg()
    best = {k: min(v[1:]) for k, v in times.items()}
    r = dict(pairs=N_PAIRS, b_first=bool(b_first), only=only, seconds=best, library=os.path.basename(os.environ["GM_LIB_PATH"]))
    if "a" in got:
        pm = got["a"]
        r.update(hits=[len(pm.hits[0]), len(pm.hits[1])], paired_mappings=len(pm.pmaps), unpaired_mappings=[len(pm.umaps[0]), len(pm.umaps[1])], digest=digest_of(pm),
                 retries_a=int(got["a_stats"]["retries"]))
    if "b" in got: r.update(sam_bytes=len(got["b"]), sam_records=int(got["b_stats"]["sam_records"]))
    print("RESULT " + json.dumps(r))


def laps():
    os.environ["GM_TIMING"] = "1"
    gm, s, m1, m2, opts = setup(False)
    s.pair_mappings(m1, m2, opts); s.map_pairs(m1, m2, opts=opts)      # warm-up
    sys.stderr.write("LAPS a\n"); sys.stderr.flush(); s.pair_mappings(m1, m2, opts)
    sys.stderr.write("LAPS b\n"); sys.stderr.flush(); s.map_pairs(m1, m2, opts=opts)
    sys.stderr.write("LAPS end\n"); sys.stderr.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", action="store_true"); ap.add_argument("--laps", action="store_true"); ap.add_argument("--b-first", action="store_true")
    ap.add_argument("--only", choices=("a", "b")); ap.add_argument("--runs", type=int, default=3); ap.add_argument("--out")
    a = ap.parse_args()
    if a.child: child(a.b_first, a.only); return
    if a.laps: laps(); return

    def run(k, extra):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__)] + extra
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if p.returncode != 0: raise SystemExit("run %s failed (%d): %s" % (k, p.returncode, (p.stdout + p.stderr)[-2000:]))
        return p
    runs = []
    for k in range(a.runs):
        p = run(k, ["--child"] + (["--b-first"] if k % 2 else []))
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]); r["run"] = k; print(json.dumps(r), flush=True); runs.append(r)
    if len({r["digest"] for r in runs}) != 1: raise SystemExit("the runs' arrays differ")
    # the stage laps of one call of each entry, tuning library
    err = run("laps", ["--laps"]).stderr
    stage = {}
    for leg, text in (("a", err.split("LAPS a\n")[1].split("LAPS b\n")[0]), ("b", err.split("LAPS b\n")[1].split("LAPS end\n")[0])):
        for name, ms in re.findall(r"pairs (.*?)\s+([0-9.]+) ms", text): stage.setdefault(leg, {}).setdefault(name.strip(), 0.0); stage[leg][name.strip()] += float(ms)
    ms = lambda c: [1e3 * r["seconds"][c] for r in runs]
    summary = dict(pairs=N_PAIRS, hits=runs[0]["hits"], paired_mappings=runs[0]["paired_mappings"], unpaired_mappings=runs[0]["unpaired_mappings"], sam_records=runs[0]["sam_records"],
                   ms_per_call={c: ms(c) for c in sorted(runs[0]["seconds"])},
                   stage_laps_ms_tuning_library=dict(gm_pair_mappings=stage.get("a", {}), gm_map_pairs=stage.get("b", {})))
    out = dict(what="%d pairs of 2 x %d bases on the cfg2 genome, letter space, release library: milliseconds of (a) one gm_pair_mappings call (arrays; pair selection on the "
                    "device; no overlap of sub-batches' output) beside (b) one gm_map_pairs call (SAM text; pair selection on the host threads; the output of a sub-batch beside "
                    "the next one's device work) on the same session and pairs -- host clock around the synchronising Python wrappers, best of %d after a warm-up, the legs "
                    "alternating, one child process a run.  Side by side; nothing is claimed from the two figures.  stage_laps: one call of each entry on the tuning library "
                    "under GM_TIMING=1, the library's own laps summed over the sub-batches (each lap ends with a stream synchronisation)" % (N_PAIRS, RLEN, REPEATS),
               runs=runs, summary=summary)
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
