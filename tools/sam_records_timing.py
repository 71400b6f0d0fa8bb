#!/usr/bin/env python3
"""Time gm_sam_records, the last call of a chunk's chain, and put gm_map_reads' own host finalisation of the same reads beside it.

    python tools/sam_records_timing.py [--runs 3] [--out profiles/r12a_sam_records_timing.json]

131 072 reads of 100 bases (bench.py's generator) on bench.py's cfg2 genome (4 x 25 Mbp), letter space, the release library.  A child process runs the chain
  gm_read_windows -> gm_sw_vector_batch_ix -> gm_select_pass1 -> gm_sw_vector_batch_ix on the hits -> gm_sw_full_ls_batch_ix -> gm_select_pass2 ->
  gm_sw_full_batch_text_ix (all hits, reverse = gen_st) -> gm_sam_records
once, then calls gm_sam_records 1 + REPEATS times on those arrays (a warm-up first) and gm_map_reads 1 + REPEATS times on the same reads, in turn.  The seam's time is
the host clock around the synchronising C call itself (the Python wrapper's array handling is outside), best of the repeats; beside it stand the bytes it made and
ms_host of gm_map_stats_t -- the wall time of the mapping entry's host finalisation (selection, mapping qualities and record text, on the session's host threads),
summed over its sub-batches -- best of the repeats.  The two numbers measure different things (a call of one thread with its uploads and its copy back against a
stage that many host threads share and that also holds the selection) and are for the reader's comparison only.  Each run is a child process of its own under its
own time limit; the first child that fails ends the run.  The children print a digest of the text, which must agree between the runs, and how many reads' bytes differ from gm_map_reads' (reads that own equal windows, and the f1 cache the chain does not emulate).
Under `rocprofv3 --kernel-trace --stats -- python tools/sam_records_timing.py --child` the kernels' own times (k_sam_records, k_win_scan) are in the trace summary.

    python tools/sam_records_timing.py --child      # the child form
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
    L = gm.lib()
    if L.gm_device_count() < 1: raise SystemExit("no HIP device")
    contigs = synth.make_genome(synth.contig_lengths("cfg2", 1.0), 2)
    reads, _ = synth.make_reads(contigs, N_READS, RLEN, 20261019)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    p = gm.default_params()
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    rw = np.ascontiguousarray(synth.pack_reads(reads)); rc = np.ascontiguousarray(synth.pack_reads(np.ascontiguousarray(CMPL[reads[:, ::-1]])))
    gm.sw_vector_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, 0, True)
    gm.sw_full_ls_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, True, p.anchor_width)
    wins, off = s.read_windows(reads)
    st = wins["st"]; rd = wins["read"]
    both = np.where((st == 1)[:, None], rc[rd], rw[rd]); lens = np.full(len(wins), RLEN); zero = np.zeros(len(wins), dtype=np.uint8)
    scores = ix.sw_vector_batch(wins["cn"], zero, wins["g_off"].astype(np.int64), wins["w_len"], both, lens)
    hits, hit_off = s.select_pass1(wins, off, scores, RLEN)
    n = len(hits); cn, gst, goff, wl = hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"]
    hr = rw[hits["read"]]; hl = np.full(n, RLEN)
    thresh = (hits["score_max"] * (p.sw_full_threshold / 100.0)).astype(np.int32)
    anchors = np.stack([hits["ax"], hits["ay"], hits["alen"], hits["awidth"]], axis=1)
    sv = ix.sw_vector_batch(cn, gst, goff, wl, hr, hl)
    recs, ops, _ = ix.sw_full_ls_batch(cn, gst, goff, wl, hr, hl, anchors=anchors, revcmpl=gst, threshscore=thresh, maxscore=sv)
    recs = recs.copy(); recs["score"][sv < thresh] = 0
    maps, map_off = s.select_pass2(hits, hit_off, recs)
    _, _, _, cigar, _ = ix.sw_full_batch_text(cn, gst, recs, ops, hr, hl, reverse=gst, what=("cigar",))
    # the clock goes around the C call itself
    c_call = L.gm_sam_records; seam, host = [], []
    def clocked(*a):
        t0 = time.perf_counter(); rc_ = c_call(*a); seam.append(time.perf_counter() - t0)
        return rc_
    L.gm_sam_records = clocked
    for _ in range(1 + REPEATS):
        text, read_off = s.sam_records(reads, hits, recs, maps, map_off, cigar, score_vector=sv)
        entry = s.map_reads(reads); host.append(s.stats["ms_host"])
    L.gm_sam_records = c_call
    if text.count(b"\n") != len(maps): raise SystemExit("%d mappings, %d records" % (len(maps), text.count(b"\n")))
    mine = [text[int(read_off[r]):int(read_off[r + 1])] for r in range(N_READS)]
    theirs = [b""] * N_READS
    for l in entry.splitlines(keepends=True): theirs[int(l[1:l.index(b"\t")])] += l
    print("RESULT " + json.dumps(dict(mappings=int(len(maps)), bytes_out=len(text), ms_gm_sam_records=1e3 * min(seam[1:]), ms_host_gm_map_reads=min(host[1:]),
                                      reads_differing_from_gm_map_reads=sum(1 for a, b in zip(mine, theirs) if a != b), digest=hashlib.sha1(text).hexdigest())))


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
    if len({(r["digest"], r["mappings"], r["bytes_out"]) for r in runs}) != 1: raise SystemExit("the runs' text differs")
    summary = dict(mappings=runs[0]["mappings"], bytes_out=runs[0]["bytes_out"], reads_differing_from_gm_map_reads=runs[0]["reads_differing_from_gm_map_reads"],
                   ms_gm_sam_records=[r["ms_gm_sam_records"] for r in runs], ms_host_gm_map_reads=[r["ms_host_gm_map_reads"] for r in runs])
    out = dict(what="%d reads of %d bases on the cfg2 genome, letter space, release library: milliseconds of one gm_sam_records call over the chunk (host clock around "
                    "the synchronising C call, best of %d after a warm-up) and, beside it, ms_host of gm_map_stats_t for gm_map_reads on the same reads (the wall time "
                    "of the mapping entry's host finalisation -- selection, mapping qualities, record text, on the session's host threads -- summed over its "
                    "sub-batches; best of %d); one child process a run" % (N_READS, RLEN, REPEATS, REPEATS),
               runs=runs, summary=summary)
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
