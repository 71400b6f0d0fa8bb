#!/usr/bin/env python3
"""Time the front half of a chunk -- reads to pass-1 hits -- the way the chain did it before gm_read_hits and with that one call.

    python tools/pass1_timing.py [--runs 3] [--out profiles/r17a_pass1_timing.json]

131 072 reads of 100 bases (bench.py's generator) on bench.py's cfg2 genome (4 x 25 Mbp), letter space, the release library.  Two legs on one session:
  (a) gm_read_windows, then the host work that way needs -- the reverse complement of the reads, one packed read per window gathered by wins[].read -- two
      gm_sw_vector_batch_ix calls (the strand-0 windows against the reads, the strand-1 windows against their reverse complements) and gm_select_pass1;
  (b) one gm_read_hits call.
Both are timed with the host clock around the synchronising Python wrappers, (a) also step by step, best of three after a warm-up of both; the legs alternate, and
every other child starts with (b).  Each run is a child process of its own under its own time limit; the first child that fails ends the run.  The hits of the two
legs must be equal, byte for byte (on this genome the f1 cache, which only (b) emulates, changes nothing), and their digest must agree between the runs.
Under `rocprofv3 --kernel-trace --stats -- python tools/pass1_timing.py --child` the kernels' own times (k_score_windows, k_sw_vector_batch_ix, k_sel_pass1,
k_sel_pass1_f1, k_win_scan, k_win_scatter, k_sel_emit) are in the trace summary.

    python tools/pass1_timing.py --child [--b-first]      # the child form
"""
import argparse, hashlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
N_READS, RLEN, REPEATS = 131072, 100, 3
CHILD_LIMIT = 420
CMPL = np.array([3, 2, 1, 0, 0, 10, 9, 7, 8, 6, 5, 14, 13, 12, 11, 15], dtype=np.uint8)      # complement_base


def child(b_first):
    os.environ.setdefault("GM_LIB_PATH", os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    from shrimp_amd import gmapper as gm, synth
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    contigs = synth.make_genome(synth.contig_lengths("cfg2", 1.0), 2)
    reads, _ = synth.make_reads(contigs, N_READS, RLEN, 20261019)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    p = gm.default_params()
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    rw = np.ascontiguousarray(synth.pack_reads(reads))
    gm.sw_vector_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, 0, True)
    times = {}

    def timed(name, f):
        t0 = time.perf_counter(); r = f(); times.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    def leg_a():
        t0 = time.perf_counter()
        wins, off = timed("a: gm_read_windows", lambda: s.read_windows(reads))
        def host():
            rc = np.ascontiguousarray(synth.pack_reads(np.ascontiguousarray(CMPL[reads[:, ::-1]])))
            st = wins["st"]; i0 = np.nonzero(st == 0)[0]; i1 = np.nonzero(st == 1)[0]
            return i0, i1, rw[wins["read"][i0]], rc[wins["read"][i1]]
        i0, i1, r0, r1 = timed("a: host (reverse complement, a read per window)", host)
        scores = np.zeros(len(wins), dtype=np.int32)
        for name, idx, rr in (("a: gm_sw_vector_batch_ix (strand 0)", i0, r0), ("a: gm_sw_vector_batch_ix (strand 1)", i1, r1)):
            w = wins[idx]
            scores[idx] = timed(name, lambda: ix.sw_vector_batch(w["cn"], np.zeros(len(w), dtype=np.uint8), w["g_off"].astype(np.int64), w["w_len"], rr, np.full(len(w), RLEN)))
        hits, hit_off = timed("a: gm_select_pass1", lambda: s.select_pass1(wins, off, scores, RLEN))
        times.setdefault("a: whole leg", []).append(time.perf_counter() - t0)
        return hits, hit_off, len(wins)

    def leg_b():
        hits, hit_off = timed("b: gm_read_hits", lambda: s.read_hits(reads))
        return hits, hit_off, s.stats["windows"]
    order = (leg_b, leg_a) if b_first else (leg_a, leg_b)
    for _ in range(1 + REPEATS):
        got = {leg.__name__: leg() for leg in order}
    (ha, oa_, wa), (hb, ob, wb) = got["leg_a"], got["leg_b"]
    if wa != wb or not np.array_equal(oa_, ob) or ha.tobytes() != hb.tobytes(): raise SystemExit("the two legs' hits differ (%d / %d windows, %d / %d hits)" % (wa, wb, len(ha), len(hb)))
    best = {k_: min(v[1:]) for k_, v in times.items()}
    print("RESULT " + json.dumps(dict(windows=int(wa), hits=int(len(hb)), bypassed=int(s.stats["vec_bypassed"]), b_first=bool(b_first), seconds=best,
                                      digest=hashlib.sha1(np.ascontiguousarray(hb).tobytes()).hexdigest())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", action="store_true"); ap.add_argument("--b-first", action="store_true"); ap.add_argument("--runs", type=int, default=3); ap.add_argument("--out")
    a = ap.parse_args()
    if a.child: child(a.b_first); return
    runs = []
    for k in range(a.runs):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + (["--b-first"] if k % 2 else [])
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if p.returncode != 0: raise SystemExit("run %d failed (%d): %s" % (k, p.returncode, (p.stdout + p.stderr)[-2000:]))
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        r["run"] = k; runs.append(r); print(json.dumps(r), flush=True)
    if len({(r["digest"], r["windows"], r["hits"]) for r in runs}) != 1: raise SystemExit("the runs' hits differ")
    calls = list(runs[0]["seconds"])
    summary = dict(windows=runs[0]["windows"], hits=runs[0]["hits"], bypassed=runs[0]["bypassed"],
                   ms_per_call={c: [1e3 * r["seconds"][c] for r in runs] for c in sorted(calls)},
                   b_over_a=[r["seconds"]["b: gm_read_hits"] / r["seconds"]["a: whole leg"] for r in runs])
    out = dict(what="%d reads of %d bases on the cfg2 genome, letter space, release library: milliseconds from reads to pass-1 hits, (a) gm_read_windows + the host's "
                    "reverse complement and per-window read gather + two gm_sw_vector_batch_ix calls + gm_select_pass1, step by step and as a whole, against (b) one "
                    "gm_read_hits call (host clock around the synchronising Python wrappers, best of %d after a warm-up, the legs alternating), one child process a run; "
                    "the hits of the two legs are equal" % (N_READS, RLEN, REPEATS), runs=runs, summary=summary)
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
