#!/usr/bin/env python3
"""Time the back half of a chunk -- reads to mappings as arrays -- the way the chain of seams did it before gm_read_mappings and with that one call.

    python tools/read_mappings_timing.py [--runs 3] [--out profiles/r19a_read_mappings_timing.json]

131 072 reads of 100 bases (bench.py's generator) on bench.py's cfg2 genome (4 x 25 Mbp), letter space, the release library.  Two legs on one session:
  (a) one gm_read_mappings call;
  (b) gm_read_hits, then what a caller wrote before: a packed read per hit gathered by hits[].read, thresh per hit, gm_sw_vector_batch_ix on the turned hit,
      gm_sw_full_ls_batch_ix with that score as maxscore, the zeroing of the records under the threshold, gm_select_pass2 and gm_sw_full_batch_text_ix over all hits --
      existing entries only, whose kernels this library compiles to the registers the parent commit's had (profiles/r19a_kernel_regs.txt).
Both are timed with the host clock around the synchronising Python wrappers, (b) also step by step (the gather's share is reported), best of three after a warm-up of
both; the legs alternate, and every other child starts with (b).  gm_map_reads on the same session is timed beside them, with nothing claimed from it: it prints text.
Each run is a child process of its own under its own time limit; the first child that fails ends the run.  The mappings of the two legs must be equal byte for byte --
maps, map_off, the second scores and the CIGARs of the mapped hits -- and their digest must agree between the runs.
Under `rocprofv3 --kernel-trace --stats -- python tools/read_mappings_timing.py --child` the kernels' own times (k_p2_items, k_sw_vector_items, k_p2_compact,
k_sw_full_batch, k_p2_records, k_p2_sel_items, k_sel_pass2, k_sw_text against k_sw_vector_batch_ix and the _ix instantiation of k_sw_full_batch) are in the trace summary.

    python tools/read_mappings_timing.py --child [--b-first] [--only a|b]      # the child form (--only: one leg, for a kernel trace of it)
"""
import argparse, hashlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
N_READS, RLEN, REPEATS = 131072, 100, 3
CHILD_LIMIT = 420


def digest_of(maps, map_off, sv, cigars):
    h = hashlib.sha1()
    for a in (maps, map_off, sv): h.update(np.ascontiguousarray(a).tobytes())
    h.update(b"\n".join(cigars))
    return h.hexdigest()


def child(b_first, only):
    os.environ.setdefault("GM_LIB_PATH", os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    from shrimp_amd import gmapper as gm, synth
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    contigs = synth.make_genome(synth.contig_lengths("cfg2", 1.0), 2)
    reads, _ = synth.make_reads(contigs, N_READS, RLEN, 20261019)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    p = gm.default_params()
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    rw_all = np.ascontiguousarray(synth.pack_reads(reads))
    gm.sw_vector_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, 0, True)
    gm.sw_full_ls_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, True, p.anchor_width)
    times = {}

    def timed(name, f):
        t0 = time.perf_counter(); r = f(); times.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    def leg_a():
        R = timed("a: gm_read_mappings", lambda: s.read_mappings(reads))
        cig = [R.cigar(int(i)) for i in R.maps["hit"]]
        return dict(maps=R.maps, map_off=R.map_off, sv=R.score_vector, cigars=cig, n_hits=len(R.hits), aligned=int(s.stats["full_calls"]))

    def leg_b():
        t0 = time.perf_counter()
        hits, hit_off = timed("b: gm_read_hits", lambda: s.read_hits(reads))
        n = len(hits)
        rw = timed("b: host (a packed read per hit)", lambda: rw_all[hits["read"]])
        def host2():
            thr = p.sw_full_threshold
            t = (-thr * np.ones(n) if thr < 0 else hits["score_max"] * (thr / 100.0)).astype(np.int32)
            return t, hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"], np.full(n, RLEN), \
                np.stack([hits["ax"], hits["ay"], hits["alen"], hits["awidth"]], axis=1), (hits["gen_st"] == 1).astype(np.uint8)
        thresh, cn, gst, goff, wl, lens, boxes, rev = timed("b: host (thresh, the window arrays)", host2)
        sv = timed("b: gm_sw_vector_batch_ix", lambda: ix.sw_vector_batch(cn, gst, goff, wl, rw, lens))
        recs, ops, _ = timed("b: gm_sw_full_ls_batch_ix", lambda: ix.sw_full_ls_batch(cn, gst, goff, wl, rw, lens, anchors=boxes,
                                                                                     revcmpl=rev if p.tiebreak_rev else None, threshscore=thresh, maxscore=sv))
        def zero():
            z = recs.copy(); z["score"][sv < thresh] = 0
            return z
        z = timed("b: host (zeroing)", zero)
        maps, map_off = timed("b: gm_select_pass2", lambda: s.select_pass2(hits, hit_off, z))
        _, _, _, cigar, _ = timed("b: gm_sw_full_batch_text_ix", lambda: ix.sw_full_batch_text(cn, gst, z, ops, rw, lens, reverse=rev, what=("cigar",)))
        times.setdefault("b: whole leg", []).append(time.perf_counter() - t0)
        return dict(maps=maps, map_off=map_off, sv=sv, cigars=[cigar(int(i)) for i in maps["hit"]], n_hits=n, aligned=int((sv >= thresh).sum()))

    legs = [l for l in ((leg_b, leg_a) if b_first else (leg_a, leg_b)) if only in (None, l.__name__[-1])]
    got = {}
    for _ in range(1 + REPEATS):
        for leg in legs: got[leg.__name__] = leg()
        timed("gm_map_reads (text, for scale)", lambda: s.map_reads(reads))
    ref = got.get("leg_a") or got["leg_b"]
    if len(legs) == 2:
        a, b = got["leg_a"], got["leg_b"]
        same = a["maps"].tobytes() == b["maps"].tobytes() and np.array_equal(a["map_off"], b["map_off"]) and np.array_equal(a["sv"], b["sv"]) and a["cigars"] == b["cigars"]
        if not same: raise SystemExit("the two legs' mappings differ (%d / %d mappings)" % (len(a["maps"]), len(b["maps"])))
    best = {k_: min(v[1:]) for k_, v in times.items()}
    print("RESULT " + json.dumps(dict(hits=int(ref["n_hits"]), aligned=int(ref["aligned"]), mappings=int(len(ref["maps"])), b_first=bool(b_first), only=only, seconds=best,
                                      library=os.path.basename(os.environ["GM_LIB_PATH"]), digest=digest_of(ref["maps"], ref["map_off"], ref["sv"], ref["cigars"]))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", action="store_true"); ap.add_argument("--b-first", action="store_true"); ap.add_argument("--only", choices=("a", "b"))
    ap.add_argument("--runs", type=int, default=3); ap.add_argument("--out")
    a = ap.parse_args()
    if a.child: child(a.b_first, a.only); return

    def one(k, extra):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"] + extra
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if p.returncode != 0: raise SystemExit("run %d failed (%d): %s" % (k, p.returncode, (p.stdout + p.stderr)[-2000:]))
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        r["run"] = k; print(json.dumps(r), flush=True)
        return r
    runs = [one(k, ["--b-first"] if k % 2 else []) for k in range(a.runs)]
    if len({(r["digest"], r["hits"], r["mappings"]) for r in runs}) != 1: raise SystemExit("the runs' mappings differ")
    ms = lambda rs, c: [1e3 * r["seconds"][c] for r in rs]
    summary = dict(hits=runs[0]["hits"], aligned=runs[0]["aligned"], removed_by_the_second_threshold=runs[0]["hits"] - runs[0]["aligned"], mappings=runs[0]["mappings"],
                   ms_per_call={c: ms(runs, c) for c in sorted(runs[0]["seconds"])},
                   a_over_b=[r["seconds"]["a: gm_read_mappings"] / r["seconds"]["b: whole leg"] for r in runs],
                   gather_share_of_b=[r["seconds"]["b: host (a packed read per hit)"] / r["seconds"]["b: whole leg"] for r in runs])
    out = dict(what="%d reads of %d bases on the cfg2 genome, letter space, release library: milliseconds from reads to mappings as arrays, (a) one gm_read_mappings call "
                    "against (b) gm_read_hits + a packed read per hit + gm_sw_vector_batch_ix + gm_sw_full_ls_batch_ix + zeroing + gm_select_pass2 + "
                    "gm_sw_full_batch_text_ix, step by step and as a whole (host clock around the synchronising Python wrappers, best of %d after a warm-up, the legs "
                    "alternating), one child process a run; gm_map_reads beside them for scale only; the mappings of the two legs are equal" % (N_READS, RLEN, REPEATS),
               runs=runs, summary=summary)
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
