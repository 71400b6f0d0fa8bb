#!/usr/bin/env python3
"""Time the back half of a colour-space chunk -- colour reads to mappings as arrays -- the way the chain of seams did it before gm_read_mappings_cs and with that one call.

    python tools/read_mappings_cs_timing.py [--runs 3] [--out profiles/r20a_read_mappings_cs_timing.json]

131 072 reads of 50 colours (bench.py's cfg4 generator) on a colour-space index of bench.py's cfg2 genome (4 x 25 Mbp), the release library.  Two legs on one session:
  (a) one gm_read_mappings_cs call;
  (b) gm_read_hits, then what a caller wrote before: a packed read and a primer letter per hit, thresh per hit, gm_sw_full_cs_batch_ix, a thread-local post_sw_setup derived
      from the session's scores, gm_post_sw_batch_ix, gm_select_pass2, the rounding-guard recipe (the device posteriors of a flagged read through the single seam post_sw,
      gm_select_pass2 again), gm_sw_full_batch_text_ix with 'H' over all hits -- existing entries only.
Both are timed with the host clock around the synchronising Python wrappers, (b) also step by step, best of three after a warm-up of both; the legs alternate, and every
other child starts with (b).  gm_map_reads_cs on the same session is timed beside them, with nothing claimed from it: it prints text and overlaps sub-batches.
Each run is a child process of its own under its own time limit; the first child that fails ends the run.  The mappings of the two legs must be equal -- every integer of
maps, map_off and the CIGARs of the mapped hits, the posteriors within 1e-9 relative -- and the digest of the integers and CIGARs must agree between the runs.
Under `rocprofv3 --kernel-trace --stats -- python tools/read_mappings_cs_timing.py --child --only a` (or b) the kernels' own times are in the trace summary.

    python tools/read_mappings_cs_timing.py --child [--b-first] [--only a|b]      # the child form (--only: one leg, for a kernel trace of it)
"""
import argparse, hashlib, json, math, os, subprocess, sys, time
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
N_READS, NCOL, REPEATS = 131072, 50, 3
CHILD_LIMIT = 420
INT_FIELDS = ("read", "hit", "score_full", "pct_score_full", "mqv", "flags")


def digest_of(maps, map_off, cigars):
    h = hashlib.sha1()
    for f in INT_FIELDS: h.update(np.ascontiguousarray(maps[f]).tobytes())
    h.update(np.ascontiguousarray(map_off).tobytes()); h.update(b"\n".join(cigars))
    return h.hexdigest()


def child(b_first, only):
    os.environ.setdefault("GM_LIB_PATH", os.path.join(ROOT, "shrimp_amd", "libgmapper_hip_release.so"))
    from shrimp_amd import gmapper as gm, synth
    if gm.lib().gm_device_count() < 1: raise SystemExit("no HIP device")
    contigs = synth.make_genome(synth.contig_lengths("cfg2", 1.0), 2)
    reads, _ = synth.make_cs_reads(contigs, N_READS, NCOL, 20261021)
    reads = np.ascontiguousarray(reads, dtype=np.uint8)
    cols = np.ascontiguousarray(reads[:, 1:]); ib_all = np.ascontiguousarray(reads[:, 0])
    p = gm.default_params_cs()
    ix = gm.Index(contigs, params=p); s = gm.Session(ix, params=p)
    rw_all = np.ascontiguousarray(synth.pack_reads(cols))
    gm.sw_full_cs_setup(1400, 1000, p.a_gap_open_score, p.a_gap_extend_score, p.b_gap_open_score, p.b_gap_extend_score, p.match_score, p.mismatch_score, p.crossover_score,
                        True, p.anchor_width, p.indel_taboo_len)
    # post_sw_setup as gmapper-cs calls it (ref: gmapper.c:2557-2572, 2959-2963): what the caller of the chain owes
    alpha = p.crossover_score / (math.log(p.pr_xover / 3) / math.log(2.0))
    pr_mm = 1.0 / (1.0 + 1.0 / 3.0 * math.pow(2.0, (float(p.match_score) - float(p.mismatch_score)) / alpha))
    beta = float(p.match_score) - 2 * alpha - alpha * math.log(1 - pr_mm) / math.log(2.0)
    gm.post_sw_setup(1400, pr_mm, p.pr_xover, math.pow(2.0, float(p.a_gap_open_score) / alpha), math.pow(2.0, float(p.a_gap_extend_score) / alpha),
                     math.pow(2.0, float(p.b_gap_open_score) / alpha), math.pow(2.0, (float(p.b_gap_extend_score) - beta) / alpha))
    times = {}; redos = {}

    def timed(name, f):
        t0 = time.perf_counter(); r = f(); times.setdefault(name, []).append(time.perf_counter() - t0)
        return r

    def leg_a():
        R = timed("a: gm_read_mappings_cs", lambda: s.read_mappings_cs(cols, initbp=ib_all))
        redos["a"] = int(s.stats["post_sw_host_redo"])
        return dict(maps=R.maps, map_off=R.map_off, cigars=[R.cigar(int(i)) for i in R.maps["hit"]], n_hits=len(R.hits))

    def leg_b():
        t0 = time.perf_counter()
        hits, hit_off = timed("b: gm_read_hits", lambda: s.read_hits(cols, initbp=ib_all))
        n = len(hits)
        rw, ib = timed("b: host (a packed read and a primer letter per hit)", lambda: (rw_all[hits["read"]], ib_all[hits["read"]]))
        def host2():
            thr = p.sw_full_threshold
            t = (-thr * np.ones(n) if thr < 0 else hits["score_max"] * (thr / 100.0)).astype(np.int32)
            return t, hits["cn"], hits["gen_st"].astype(np.uint8), hits["g_off"].astype(np.int64), hits["w_len"], np.full(n, NCOL), \
                np.stack([hits["ax"], hits["ay"], hits["alen"], hits["awidth"]], axis=1), (hits["gen_st"] == 1).astype(np.uint8)
        thresh, cn, gst, goff, wl, lens, boxes, rev = timed("b: host (thresh, the window arrays)", host2)
        recs, ops, strings = timed("b: gm_sw_full_cs_batch_ix", lambda: ix.sw_full_cs_batch(cn, gst, goff, wl, rw, lens, ib, boxes, revcmpl=rev if p.tiebreak_rev else None,
                                                                                           threshscore=thresh))
        post, qralign, _ = timed("b: gm_post_sw_batch_ix", lambda: ix.post_sw_batch(cn, gst, recs, ops, rw, lens, ib))
        maps, map_off = timed("b: gm_select_pass2", lambda: s.select_pass2(hits, hit_off, recs, post))
        qbuf = qralign.buffer
        def guard():
            nonlocal post, qbuf
            flagged = sorted(set(maps["read"][(maps["flags"] & 1) != 0].tolist())); k = 0
            if not flagged: return maps, map_off, 0
            strings.prefetch(); post = post.copy(); qb = bytearray(qbuf)
            for r in flagged:
                for i in range(int(hit_off[r]), int(hit_off[r + 1])):
                    if recs[i]["score"] <= 0 or post[i]["by_host"]: continue
                    db, qr = strings(i)
                    one = gm.post_sw(rw[i], int(ib[i]), db, qr, int(recs[i]["read_start"]))
                    post[i]["posterior"] = one["posterior"]; post[i]["by_host"] = 1; k += 1
                    qb[int(recs[i]["ops_off"]):int(recs[i]["ops_off"]) + int(recs[i]["n_ops"])] = one["qralign"].encode()
            qbuf = bytes(qb)
            m2, o2 = s.select_pass2(hits, hit_off, recs, post)
            return m2, o2, k
        maps, map_off, k = timed("b: the guard recipe (post_sw of flagged reads, gm_select_pass2 again)", guard)
        redos["b"] = int(post["by_host"].sum())
        _, _, _, cigar, _ = timed("b: gm_sw_full_batch_text_ix", lambda: ix.sw_full_batch_text(cn, gst, recs, ops, rw, lens, initbp=ib, qralign=qbuf, reverse=rev, clip="H",
                                                                                              what=("cigar",), colour_space=True))
        times.setdefault("b: whole leg", []).append(time.perf_counter() - t0)
        return dict(maps=maps, map_off=map_off, cigars=[cigar(int(i)) for i in maps["hit"]], n_hits=n)

    legs = [l for l in ((leg_b, leg_a) if b_first else (leg_a, leg_b)) if only in (None, l.__name__[-1])]
    got = {}
    for _ in range(1 + REPEATS):
        for leg in legs: got[leg.__name__] = leg()
        timed("gm_map_reads_cs (text, for scale)", lambda: s.map_reads_cs(reads))
    ref = got.get("leg_a") or got["leg_b"]
    bit_equal = None
    if len(legs) == 2:
        a, b = got["leg_a"], got["leg_b"]
        same = all(np.array_equal(a["maps"][f], b["maps"][f]) for f in INT_FIELDS) and np.array_equal(a["map_off"], b["map_off"]) and a["cigars"] == b["cigars"] and \
            all((np.abs(a["maps"][f] - b["maps"][f]) <= 1e-9 * np.abs(b["maps"][f])).all() for f in ("posterior", "z0", "z1"))
        if not same: raise SystemExit("the two legs' mappings differ (%d / %d mappings)" % (len(a["maps"]), len(b["maps"])))
        bit_equal = a["maps"].tobytes() == b["maps"].tobytes()
    best = {k_: min(v[1:]) for k_, v in times.items()}
    print("RESULT " + json.dumps(dict(hits=int(ref["n_hits"]), mappings=int(len(ref["maps"])), b_first=bool(b_first), only=only, seconds=best, host_redos=redos,
                                      doubles_bit_equal=bit_equal, library=os.path.basename(os.environ["GM_LIB_PATH"]), digest=digest_of(ref["maps"], ref["map_off"], ref["cigars"]))))


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
    summary = dict(hits=runs[0]["hits"], mappings=runs[0]["mappings"], host_redos=runs[0]["host_redos"], doubles_bit_equal=[r["doubles_bit_equal"] for r in runs],
                   ms_per_call={c: ms(runs, c) for c in sorted(runs[0]["seconds"])},
                   a_over_b=[r["seconds"]["a: gm_read_mappings_cs"] / r["seconds"]["b: whole leg"] for r in runs])
    out = dict(what="%d reads of %d colours on a colour-space index of the cfg2 genome, release library: milliseconds from colour reads to mappings as arrays, (a) one "
                    "gm_read_mappings_cs call against (b) gm_read_hits + a packed read per hit + gm_sw_full_cs_batch_ix + gm_post_sw_batch_ix + gm_select_pass2 + the guard "
                    "recipe + gm_sw_full_batch_text_ix, step by step and as a whole (host clock around the synchronising Python wrappers, best of %d after a warm-up, the "
                    "legs alternating), one child process a run; gm_map_reads_cs beside them for scale only; the mappings of the two legs are equal" % (N_READS, NCOL, REPEATS),
               runs=runs, summary=summary)
    print(json.dumps(summary, indent=1))
    if a.out:
        with open(a.out, "w") as f: json.dump(out, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
