#!/usr/bin/env python3
"""Time the two selection seams beside the other calls of a chunk's chain, so that a reader sees what share of the chain selection is.

    python tools/select_timing.py [--runs 3] [--out profiles/r11a_select_timing.json]

131 072 reads of 100 bases (bench.py's generator) on bench.py's cfg2 genome (4 x 25 Mbp), letter space, the release library.  The chain of a chunk:
  gm_read_windows -> gm_sw_vector_batch_ix -> gm_select_pass1 -> gm_sw_vector_batch_ix on the hits (hit_run_full_sw's second score) -> gm_sw_full_ls_batch_ix ->
  gm_select_pass2 -> gm_sw_full_batch_text_ix
Every call is timed with the host clock around the Python wrapper (each ends in a device synchronise; the wrapper's own array handling is inside, the preparation of
the next call's arguments is not), best of three after a warm-up pass of the whole chain.  Each run is a child process of its own under its own time limit; the first
child that fails ends the run.  The children print the numbers of windows, hits and mappings and a digest of the mappings, which must agree between the runs and with
the records gm_map_reads counts on the same session.  Under `rocprofv3 --kernel-trace --stats -- python tools/select_timing.py --child` the selection kernels' own
times (k_sel_pass1, k_win_scan, k_sel_emit, k_sel_pass2) are in the trace summary.

    python tools/select_timing.py --child      # the child form
"""
import argparse, hashlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
N_READS, RLEN, REPEATS = 131072, 100, 3
CHILD_LIMIT = 420
CMPL = np.array([3, 2, 1, 0, 0, 10, 9, 7, 8, 6, 5, 14, 13, 12, 11, 15], dtype=np.uint8)      # complement_base


def child():
    os.environ.setdefault("GM_LIB_PATH", os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    from shrimp_amd import gmapper as gm, synth
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    contigs = synth.make_genome(synth.contig_lengths("cfg2", 1.0), 2)
    reads, _ = synth.make_reads(contigs, N_READS, RLEN, 20261019)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    p = gm.default_params()
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    rw = np.ascontiguousarray(synth.pack_reads(reads)); rc = np.ascontiguousarray(synth.pack_reads(np.ascontiguousarray(CMPL[reads[:, ::-1]])))
    gm.sw_vector_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, 0, True)
    gm.sw_full_ls_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, True, p.anchor_width)
    times = {}

    def timed(name, f):
        t0 = time.perf_counter(); r = f(); times.setdefault(name, []).append(time.perf_counter() - t0)
        return r
    for _ in range(1 + REPEATS):
        wins, off = timed("gm_read_windows", lambda: s.read_windows(reads))
        st = wins["st"]; rd = wins["read"]
        both = np.where((st == 1)[:, None], rc[rd], rw[rd]); lens = np.full(len(wins), RLEN); zero = np.zeros(len(wins), dtype=np.uint8)      # pass 1: the forward window, strand st of the read
        scores = timed("gm_sw_vector_batch_ix (pass 1)", lambda: ix.sw_vector_batch(wins["cn"], zero, wins["g_off"].astype(np.int64), wins["w_len"], both, lens))
        hits, hit_off = timed("gm_select_pass1", lambda: s.select_pass1(wins, off, scores, RLEN))
        n = len(hits); cn, gst, goff, wl = hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"]
        hr = rw[hits["read"]]; hl = np.full(n, RLEN)
        thresh = (hits["score_max"] * (p.sw_full_threshold / 100.0)).astype(np.int32)
        anchors = np.stack([hits["ax"], hits["ay"], hits["alen"], hits["awidth"]], axis=1)
        sv = timed("gm_sw_vector_batch_ix (pass 2)", lambda: ix.sw_vector_batch(cn, gst, goff, wl, hr, hl))
        recs, ops, _ = timed("gm_sw_full_ls_batch_ix", lambda: ix.sw_full_ls_batch(cn, gst, goff, wl, hr, hl, anchors=anchors, revcmpl=gst, threshscore=thresh, maxscore=sv))
        recs = recs.copy(); recs["score"][sv < thresh] = 0
        maps, map_off = timed("gm_select_pass2", lambda: s.select_pass2(hits, hit_off, recs))
        k = maps["hit"]
        timed("gm_sw_full_batch_text_ix", lambda: ix.sw_full_batch_text(cn[k], gst[k], recs[k], ops, hr[k], hl[k], reverse=gst[k], what=("cigar", "edit")))
    s.map_reads(reads)
    if s.stats["sam_records"] != len(maps): raise SystemExit("the chain has %d mappings, gm_map_reads printed %d records" % (len(maps), s.stats["sam_records"]))
    best = {k_: min(v[1:]) for k_, v in times.items()}
    print("RESULT " + json.dumps(dict(windows=int(len(wins)), hits=int(n), mappings=int(len(maps)), seconds=best,
                                      digest=hashlib.sha1(np.ascontiguousarray(maps).tobytes()).hexdigest())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", action="store_true"); ap.add_argument("--runs", type=int, default=3); ap.add_argument("--out")
    a = ap.parse_args()
    if a.child: child(); return
    runs = []
    for k in range(a.runs):
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, cwd=ROOT)
        if p.returncode != 0: raise SystemExit("run %d failed (%d): %s" % (k, p.returncode, (p.stdout + p.stderr)[-2000:]))
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        r["run"] = k; runs.append(r); print(json.dumps(r), flush=True)
    if len({(r["digest"], r["windows"], r["hits"], r["mappings"]) for r in runs}) != 1: raise SystemExit("the runs' mappings differ")
    calls = list(runs[0]["seconds"])
    summary = dict(windows=runs[0]["windows"], hits=runs[0]["hits"], mappings=runs[0]["mappings"],
                   ms_per_call={c: [1e3 * r["seconds"][c] for r in runs] for c in calls},
                   chain_ms=[1e3 * sum(r["seconds"].values()) for r in runs],
                   selection_share=[(r["seconds"]["gm_select_pass1"] + r["seconds"]["gm_select_pass2"]) / sum(r["seconds"].values()) for r in runs])
    out = dict(what="%d reads of %d bases on the cfg2 genome, letter space, release library: milliseconds of every call of a chunk's chain (host clock around the "
                    "synchronising Python wrapper, best of %d after a warm-up pass), one child process a run" % (N_READS, RLEN, REPEATS), runs=runs, summary=summary)
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
