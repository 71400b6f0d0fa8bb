#!/usr/bin/env python3
"""Generate tests/golden/* from the REFERENCE binary built by oracle/Makefile.ref.

Runs only in the build container (needs /root/reference).  Fixtures are data only:
inputs (2-bit/4-bit packed codes in .npz) and the reference's SAM output (gz, @PG line dropped
because it embeds the command line, gmapper/gmapper.c:3007), plus known-answer records from the
reference's own sw_vector()/sw_full_ls() (oracle/ref_kat.cpp).

    make -f oracle/Makefile.ref && python tools/make_golden.py
"""
import gzip, os, subprocess, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from shrimp_amd import synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REF = os.path.join(ROOT, "oracle", "_ref", "gmapper-ls")
OUT = os.path.join(ROOT, "tests", "golden")


def stress_genome(seed=77):
    """Small repeat-rich genome: tandem repeats (lists beyond the cutoff), dispersed copies of a
    family with a few mutations, homopolymers, N runs, IUPAC codes, a contig shorter than a window."""
    rng = np.random.Generator(np.random.PCG64(seed))
    def rnd(n): return rng.integers(0, 4, size=n, dtype=np.uint8)
    fam = rnd(400)
    c1 = [rnd(30000)]
    for k in range(25):
        f = fam.copy()
        m = rng.integers(0, 400, size=4); f[m] = (f[m] + 1) & 3
        c1 += [f, rnd(int(rng.integers(50, 3000)))]
    c1 += [np.tile(np.array([0, 1, 2, 3, 3, 2, 1, 0, 2], dtype=np.uint8), 1500), rnd(20000)]   # 9-mer tandem x1500
    c1 += [np.zeros(300, dtype=np.uint8), rnd(5000), np.full(120, 15, dtype=np.uint8), rnd(40000)]
    c1 = np.concatenate(c1)
    c2 = rnd(120000)
    c2[5000:5400] = fam                      # family copy on another contig
    c2[60000:60010] = 15
    iu = rng.integers(0, 120000, size=40); c2[iu] = rng.integers(4, 15, size=40).astype(np.uint8)
    c3 = rnd(70)                             # shorter than a 100bp read's window
    c4 = np.concatenate([rnd(50000), c1[2000:2600], rnd(3000), c1[2000:2600][::-1].copy(), rnd(20000)])
    return [c1, c2, c3, c4]


def stress_reads(contigs, n, L, seed=78):
    reads, _ = synth.make_reads([c for c in contigs if len(c) > 2 * L + 40], n, L, seed, p_sub=0.03, p_ins=0.004, p_del=0.004)
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    # the source contigs may contain codes > 3; clamp sampled IUPAC to N for reads and sprinkle extra Ns
    reads = np.where(reads > 3, 15, reads).astype(np.uint8)
    k = rng.integers(0, n, size=n // 20)
    reads[k, rng.integers(0, L, size=k.size)] = 15
    return reads


def write_fa_codes(path, names, seqs):
    T = np.frombuffer(b"ACGTUMRWSYKVHDBN", dtype=np.uint8)
    with open(path, "wb") as f:
        for nm, s in zip(names, seqs):
            f.write(b">" + nm + b"\n")
            t = T[s]
            for k in range(0, len(t), 70):
                f.write(t[k:k + 70].tobytes() + b"\n")


def run_case(name, contigs, reads, extra=()):
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.fa")
        write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
        write_fa_codes(r, [b"r%d" % i for i in range(len(reads))], list(reads))
        p = subprocess.run([REF, "-N", "4", *extra, r, g], capture_output=True, check=True)
        body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    np.savez_compressed(os.path.join(OUT, name + ".npz"),
                        **{"contig%d" % i: c for i, c in enumerate(contigs)}, reads=reads)
    with gzip.open(os.path.join(OUT, name + ".sam.gz"), "wb", compresslevel=9) as f:
        f.write(body)
    n_map = sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))
    print(f"{name}: {len(reads)} reads -> {n_map} SAM records")


def n1_noisy_case():
    """-n 1 on noisy reads (9 % substitutions): reads whose only evidence is ONE k-mer match still map -- no region counts, a window per anchor (gmapper.c:2610-2625)"""
    contigs = synth.make_genome([400000, 250000], 77)
    reads, _ = synth.make_reads(contigs, 4000, 70, 78, p_sub=0.09, p_ins=0.004, p_del=0.004)
    run_case("n1_noisy_70bp", contigs, reads, extra=("-n", "1"))
    # reads built to have exactly ONE list entry: a 14-base block (one placement of the span-14 default seed) left intact, a substitution next to it on either side
    # and every 4th base from there on; -h 30% lets their alignments through.  390 of 400 map with -n 1, none without it.
    rng = np.random.default_rng(5); L = 60
    one = np.empty((400, L), dtype=np.uint8)
    for i in range(len(one)):
        c = contigs[rng.integers(0, len(contigs))]
        p = int(rng.integers(0, len(c) - L)); r = c[p:p + L].copy()
        b = int(rng.integers(0, L - 14 + 1))
        for j in list(range(b - 1, -1, -4)) + list(range(b + 14, L, 4)): r[j] = (r[j] + 1 + rng.integers(0, 3)) & 3
        if rng.random() < 0.5: r = (3 - r[::-1]).astype(np.uint8)
        one[i] = r
    run_case("n1_onehit_60bp", contigs, one, extra=("-n", "1", "-h", "30%"))


F1_TWIN = np.array([8, 9, 10, 15], dtype=np.uint8)      # S Y K N: the letters hash_genome_window (common/util.h:221-241, base & 3) folds onto A C G T


def f1_twins_inputs():
    """A 400-base segment and, EARLIER in list order, its copy with runs of 22 IUPAC twins every 40 bases; 300 exact 60-base reads of the clean segment.  A clean window
    and its damaged copy share an f1 cache slot, so with the cache on (the default) a read whose damaged copy scores below the threshold takes that score for the
    clean window too and comes out unmapped; under -Z every read maps 60M."""
    rng = np.random.default_rng(11)
    g = rng.integers(0, 4, 40000).astype(np.uint8)
    seg = g[25000:25400].copy()
    twin = seg.copy()
    for lo in range(40, 321, 40): twin[lo:lo + 22] = F1_TWIN[seg[lo:lo + 22]]
    g[5000:5400] = twin
    reads = np.stack([seg[o:o + 60] for o in range(20, 320)]).astype(np.uint8)
    return [g], reads


def f1_twins_case():
    contigs, reads = f1_twins_inputs()
    run_case("f1_twins_60bp", contigs, reads)                            # the reference's default: the cache on
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.fa")
        write_fa_codes(g, [b"contig1"], contigs)
        write_fa_codes(r, [b"r%d" % i for i in range(len(reads))], list(reads))
        p = subprocess.run([REF, "-N", "4", "-Z", r, g], capture_output=True, check=True)
        body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    with gzip.open(os.path.join(OUT, "f1_twins_60bp@no_cache.sam.gz"), "wb", compresslevel=9) as f:
        f.write(body)
    mapped = lambda text: {l.split(b"\t")[0] for l in text.split(b"\n") if l and not l.startswith(b"@") and not int(l.split(b"\t")[1]) & 4}
    with gzip.open(os.path.join(OUT, "f1_twins_60bp.sam.gz"), "rb") as f: on = mapped(f.read())
    off = mapped(body)
    print("f1_twins_60bp@no_cache: %d reads mapped, %d with the cache, %d only without it" % (len(off), len(on), len(off - on)))
    assert len(off - on) >= 20, "the draw does not show the cache: fewer than 20 reads map only under -Z"


def mirna_case():
    """-M mirna: the mode's option bundle (gmapper.c:1497-1517: -H, -U, anchor width 0, gap opens -255, no f1 cache, -n 1, window 100 %, --local, no mapping
    qualities) with its five default seeds of span 20 / weight 14 (leading and trailing zeros, gmapper-defaults.h:230-238) on 22-base reads"""
    contigs = synth.make_genome([300000, 200000], 91)
    reads, _ = synth.make_reads(contigs, 3000, 22, 92, p_sub=0.04, p_ins=0.0, p_del=0.0)
    run_case("mirna_22bp", contigs, reads, extra=("-M", "mirna"))


def read_fa(path):
    names, seqs = [], []
    for line in open(path, "rb"):
        line = line.strip()
        if not line: continue
        if line.startswith(b">"): names.append(line[1:].split()[0]); seqs.append(b"")
        else: seqs[-1] += line
    return names, seqs


CODE = {c: i for i, c in enumerate(b"ACGTUMRWSYKVHDBN")}


def to_codes(seq):
    return np.array([CODE[c] for c in seq.upper()], dtype=np.uint8)


def run_pair_case(name, contigs, contig_names, m1, m2, names1, names2, mode, ins):
    """mates adjacent in one file, as gmapper expects in paired mode (ref: gmapper.c:2319-2322)"""
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.fa")
        write_fa_codes(g, contig_names, contigs)
        names = [n for pair in zip(names1, names2) for n in pair]
        seqs = [q for pair in zip(list(m1), list(m2)) for q in pair]
        write_fa_codes(r, names, seqs)
        p = subprocess.run([REF, "-N", "4", "-p", mode, "-I", "%d,%d" % ins, r, g], capture_output=True, check=True)
        body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **{"contig%d" % i: c for i, c in enumerate(contigs)},
                        mates1=np.asarray(m1), mates2=np.asarray(m2),
                        names1=np.array(names1), names2=np.array(names2), contig_names=np.array(contig_names),
                        mode=np.array(mode), ins=np.array(ins))
    with gzip.open(os.path.join(OUT, name + ".sam.gz"), "wb", compresslevel=9) as f:
        f.write(body)
    n_rec = sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))
    print("%s: %d pairs -> %d SAM records" % (name, len(m1), n_rec))


def paired_cases():
    # (1) the reference's own pairing fixture (not_in_dist/test_pairing): 24 pairs, mates of 30 and 50 bp, under all four pair modes
    fx = "/root/reference/not_in_dist/test_pairing"
    gn, gs = read_fa(os.path.join(fx, "reference-pairing.fa"))
    rn, rs = read_fa(os.path.join(fx, "reads-pairing.fa"))
    contigs = [to_codes(q) for q in gs]
    m1 = np.stack([to_codes(q) for q in rs[0::2]]); m2 = np.stack([to_codes(q) for q in rs[1::2]])
    for mode in ("opp-in", "opp-out", "col-fw", "col-bw"):
        run_pair_case("pairfix_" + mode, contigs, gn, m1, m2, rn[0::2], rn[1::2], mode, (0, 500))
    # (2) cfg5-like: 2 x 150 bp opp-in pairs, insert ~ N(300, 30), 1 % substitutions, uniform genome
    contigs = synth.make_genome([600_000, 400_000], 55)
    reads, _ = synth.make_pairs(contigs, 1500, 150, 5)
    n = len(reads) // 2
    run_pair_case("cfg5s_2x150_1Mbp", contigs, [b"contig1", b"contig2"], reads[0::2], reads[1::2],
                  [b"p%d/1" % i for i in range(n)], [b"p%d/2" % i for i in range(n)], "opp-in", (100, 600))
    # (3) pairs on the repeat-rich stress genome (half-paired rescue, duplicate pruning, unpaired mates)
    sg = stress_genome()
    r2, _ = synth.make_pairs([c for c in sg if len(c) > 2000], 1200, 100, 6, ins_mean=250, ins_sd=40, ins_min=120, p_sub=0.02)
    r2 = np.where(r2 > 3, 15, r2).astype(np.uint8)
    n = len(r2) // 2
    run_pair_case("stress_pairs_2x100", sg, [b"contig%d" % (i + 1) for i in range(len(sg))], r2[0::2], r2[1::2],
                  [b"q%d:1" % i for i in range(n)], [b"q%d:2" % i for i in range(n)], "opp-in", (100, 600))


def chimeric_pairs_case():
    """pairs whose mates come from different places (every third pair of the cfg5-like set takes the second mate of another pair): both mates map on their own, never
    as a pair -- what --single-best-mapping --all-contigs turns into IMPROPER pairs (output.c:1178-1226); the default run is the base golden"""
    z = np.load(os.path.join(OUT, "cfg5s_2x150_1Mbp.npz"))
    contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    N = 600
    m1 = z["mates1"][:N].copy(); m2 = z["mates2"][:N].copy()
    src = np.arange(N); src[0::3] = (src[0::3] + 301) % N
    m2 = m2[src]
    run_pair_case("chimeric_pairs_2x150", contigs, [bytes(x) for x in z["contig_names"]], m1, m2, [b"c%d/1" % i for i in range(N)], [b"c%d/2" % i for i in range(N)], "opp-in", (100, 600))


OPTION_CASES = {
    # tag: (base golden whose inputs are reused, reference command-line options)
    "chim_single_best_all": ("chimeric_pairs_2x150", ["--single-best-mapping", "--all-contigs"]),
    "chim_single_best_all_noimp": ("chimeric_pairs_2x150", ["--single-best-mapping", "--all-contigs", "--no-improper-mappings"]),
    "chim_single_best": ("chimeric_pairs_2x150", ["--single-best-mapping"]),
    "strata":    ("stress_60bp", ["--strata"]),
    "max3_o5":   ("stress_60bp", ["--max-alignments", "3", "-o", "5"]),
    "scores":    ("stress_100bp_unal", ["-m", "8", "-i", "-12", "-g", "-30", "-q", "-28", "-e", "-5", "-f", "-4", "-h", "60%", "-w", "150%",
                                        "-l", "80%", "-r", "50%", "-o", "6", "-a", "10", "--sam-unaligned"]),
    "seeds":     ("cfg2s_100bp_2Mbp", ["-s", "1111101111,110110110110111,1110100111010111", "-z", "40"]),
    "pairs_strata": ("stress_pairs_2x100", ["--strata", "-o", "4"]),
    "local":     ("stress_100bp_unal", ["--local", "--sam-unaligned"]),
    "local60":   ("stress_60bp", ["--local", "-h", "40%"]),
    "local_cfg2": ("cfg2s_100bp_2Mbp", ["--local"]),
    "ungapped":  ("stress_100bp_unal", ["--local", "-U", "--sam-unaligned"]),
    "ungapped60_n1": ("stress_60bp", ["--local", "-U", "-n", "1", "-h", "45%"]),
    # output policy of read_output / readpair_output (output.c:955-1008,1070-1291): the best mapping only, per class or over all classes (with an improper pair of two
    # unpaired mappings when both are good), no Z tags with --all-contigs, no mapping qualities at all
    "single_best": ("stress_60bp", ["--single-best-mapping"]),
    "all_contigs": ("stress_60bp", ["--all-contigs"]),
    "no_mapq": ("stress_100bp_unal", ["--no-mapping-qualities", "--sam-unaligned"]),
    "pairs_single_best": ("stress_pairs_2x100", ["--single-best-mapping"]),
    "pairs_single_best_all": ("stress_pairs_2x100", ["--single-best-mapping", "--all-contigs"]),
    "pairs_single_best_all_noimp": ("stress_pairs_2x100", ["--single-best-mapping", "--all-contigs", "--no-improper-mappings"]),
    "pairs_no_mapq": ("stress_pairs_2x100", ["--no-mapping-qualities"]),
    # the optional tail of the SAM records (output.c:452-465,729-756): --extra-sam-fields (ZM / ZR / ZV / ZH / ZE), --read-group, --sam-r2 (paired mode)
    # (inputs without N: the reference's reverse_alignment_edit_string never returns on a letter it does not know -- its assert(0) is compiled out)
    "extra_fields": ("cfg2s_100bp_2Mbp", ["--extra-sam-fields"]),
    "extra_fields_rg_unal": ("n1_noisy_70bp", ["--extra-sam-fields", "--read-group", "grp1,sampleA", "--sam-unaligned"]),
    "rg_unal": ("stress_100bp_unal", ["--read-group", "grp1,sampleA", "--sam-unaligned"]),
    "pairs_r2_rg_extra": ("cfg5s_2x150_1Mbp", ["--sam-r2", "--read-group", "grp1,sampleA", "--extra-sam-fields"]),
    "pairs_r2_rg": ("stress_pairs_2x100", ["--sam-r2", "--read-group", "grp1,sampleA"]),
    # region geometry of the k-mer hit counts (--region-bits, --region-overlap)
    "regions_10_30": ("stress_60bp", ["--region-bits", "10", "--region-overlap", "30"]),
    "regions_12_200": ("cfg2s_100bp_2Mbp", ["--region-bits", "12", "--region-overlap", "200"]),
    # -t: the full-SW tie-breaks are not reversed for hits on the negative strand (Tflag off; mapping.c:378,393)
    "tiebreak_off": ("stress_100bp_unal", ["-t", "--sam-unaligned"]),
    "pairs_tiebreak_off": ("stress_pairs_2x100", ["-t"]),
    # -F / -C: only the read as given / only its reverse complement
    "positive": ("stress_60bp", ["-F"]),
    "negative": ("stress_60bp", ["-C"]),
    # -n 1 on its own: no region counts at all, every list entry becomes an anchor and every anchor a window (gmapper.c:2610-2624)
    "n1":        ("stress_60bp", ["-n", "1"]),
    "hashed":    ("stress_60bp", ["-H"]),
    "hashed_w16": ("cfg2s_100bp_2Mbp", ["-H", "-s", "11111111101111111,1111110111011101111,111101110010000101111011"]),
    "pairs_hashed": ("stress_pairs_2x100", ["-H", "-o", "3"]),
    "pairs_local": ("stress_pairs_2x100", ["--local"]),
    "pairs_ungapped": ("stress_pairs_2x100", ["--local", "-U"]),
    # --no-half-paired: mate-pair region counts in the anchor lists (use_mp_region_counts = 1), no unpaired rescue
    "no_half_paired": ("stress_pairs_2x100", ["--no-half-paired"]),
    "cfg5_no_half_paired": ("cfg5s_2x150_1Mbp", ["--no-half-paired"]),
    # -n 3 in paired mode: a region marked once counts when the mate has hits within reach (use_mp_region_counts 2, or 3 with --no-half-paired; hit list mode 3,
    # gmapper.c:2657-2673); -n 2 in paired mode: no region counts at all, a window per anchor
    "pairs_n3": ("stress_pairs_2x100", ["-n", "3"]),
    "pairs_n3_nhp": ("stress_pairs_2x100", ["-n", "3", "--no-half-paired"]),
    "cfg5_n3": ("cfg5s_2x150_1Mbp", ["-n", "3"]),
    "cfg5_n3_nhp": ("cfg5s_2x150_1Mbp", ["-n", "3", "--no-half-paired"]),
    "pairs_n2": ("stress_pairs_2x100", ["-n", "2"]),
    "pairs_hashed_n3": ("stress_pairs_2x100", ["-H", "-n", "3"]),                       # hashed seeds under the mate-pair modes of the generic lookup kernel
    "pairs_local_n3_nhp": ("stress_pairs_2x100", ["--local", "-n", "3", "--no-half-paired"]),
    "cfg5_n2": ("cfg5s_2x150_1Mbp", ["-n", "2"]),
    # the score sets of tests/golden/sw_kat_scores.txt.gz through the whole program (-m match, -i mismatch, -g / -e open / extend along the genome, -q / -f along the read)
    "scores_unit": ("stress_100bp_unal", ["-m", "1", "-i", "-1", "-g", "-1", "-e", "-1", "-q", "-1", "-f", "-1", "--sam-unaligned"]),
    "scores_swapped": ("stress_100bp_unal", ["-m", "10", "-i", "-15", "-g", "-20", "-e", "-2", "-q", "-45", "-f", "-9", "--sam-unaligned"]),
    "scores_large": ("stress_100bp_unal", ["-m", "32", "-i", "-60", "-g", "-100", "-e", "-20", "-q", "-90", "-f", "-25", "--sam-unaligned"]),
    "scores_linear": ("stress_60bp", ["-m", "10", "-i", "-15", "-g", "0", "-e", "-12", "-q", "0", "-f", "-9"]),
    "pairs_scores_swapped": ("stress_pairs_2x100", ["-m", "10", "-i", "-15", "-g", "-20", "-e", "-2", "-q", "-45", "-f", "-9"]),
}


# colour-space option sets (gmapper-cs): inputs of a committed colour-space golden, the reference's SAM body as <base>@<tag>.sam.gz
CS_OPTION_CASES = {
    "cs_local":        ("cfg4s_50col_2Mbp", ["--local"]),
    "cs_local_unal":   ("stress_cs_60col_unal", ["--local", "--sam-unaligned"]),
    "cs_ungapped":     ("cfg4s_50col_2Mbp", ["--local", "-U"]),
    "cs_ungapped_unal": ("stress_cs_60col_unal", ["--local", "-U", "--sam-unaligned", "-h", "40%"]),
    "cs_tiebreak_off": ("stress_cs_60col_unal", ["-t", "--sam-unaligned"]),
    "cs_xover_taboo":  ("stress_cs_60col_unal", ["-x", "-25", "--indel-taboo-len", "3", "--pr-xover", "0.05", "--sam-unaligned"]),
    "cs_no_mapq":      ("cfg4s_50col_2Mbp", ["--no-mapping-qualities"]),         # global sw_full_cs, no post_sw: sw_full_cs's own strings and counts in the output
    "cs_single_best":  ("stress_cs_60col_unal", ["--single-best-mapping", "--sam-unaligned"]),
    "cs_extra_rg":     ("cfg4s_50col_2Mbp", ["--extra-sam-fields", "--read-group", "grp1,sampleA", "--sam-unaligned"]),
    # other scores in colour space; cs_gate_under / cs_gate_over: large gap and crossover penalties on either side of the gate between the two pass-2 kernels of the
    # GPU library (60 colours + windows of 84 = 144 moves, a move at most 71 + 40 = 111: 15984, or 72 + 40 = 112: 16128, against 16000)
    "cs_scores_swapped": ("stress_cs_60col_unal", ["-m", "10", "-i", "-15", "-x", "-20", "-g", "-20", "-e", "-2", "-q", "-45", "-f", "-9", "--sam-unaligned"]),
    "cs_gate_under":   ("stress_cs_60col_unal", ["-x", "-40", "-g", "-60", "-e", "-11", "-q", "-55", "-f", "-10", "--sam-unaligned"]),
    "cs_gate_over":    ("stress_cs_60col_unal", ["-x", "-40", "-g", "-60", "-e", "-12", "-q", "-55", "-f", "-10", "--sam-unaligned"]),
}


def cs_option_cases(only=None):
    for tag, (base, extra) in CS_OPTION_CASES.items():
        if only and tag not in only: continue
        z = np.load(os.path.join(OUT, base + ".npz"))
        contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
        with tempfile.TemporaryDirectory() as d:
            g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfasta")
            write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
            synth.write_csfasta_reads(r, z["reads"])
            p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-cs"), "-N", "4", *extra, r, g], capture_output=True, check=True)
            body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG") and not l.startswith(b"@RG"))
        with gzip.open(os.path.join(OUT, "%s@%s.sam.gz" % (base, tag)), "wb", compresslevel=9) as f:
            f.write(body)
        print("%s@%s: %d SAM records" % (base, tag, sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))))


CS_PAIR_OPTION_CASES = {        # tag -> (base colour-space pair golden, extra gmapper-cs options)
    "cs_pairs_local": ("cs_pairs_50col_opp-in", ["--local"]),
    "cs_pairs_local_colbw": ("cs_pairs_50col_col-bw", ["--local"]),
    "cs_pairs_n3": ("cs_pairs_50col_opp-in", ["-n", "3"]),                                # paired match mode 3 in colour space; with --no-half-paired on a mode that reverses a mate
    "cs_pairs_n3_colbw_nhp": ("cs_pairs_50col_col-bw", ["-n", "3", "--no-half-paired"]),
    "cs_pairs_n2": ("cs_pairs_50col_opp-in", ["-n", "2"]),
    "cs_pairs_r2_extra": ("cs_pairs_50col_col-bw", ["--sam-r2", "--extra-sam-fields"]),
}


def cs_pair_option_cases(only=None):
    """non-default options on the committed colour-space pairs (mates adjacent in one csfasta file, as cs_pair_case writes them): only the reference's SAM body is stored"""
    for tag, (base, extra) in CS_PAIR_OPTION_CASES.items():
        if only and tag not in only: continue
        z = np.load(os.path.join(OUT, base + ".npz"))
        contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
        m1, m2 = z["mates1"], z["mates2"]; n = len(m1)
        with tempfile.TemporaryDirectory() as d:
            g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfasta")
            write_fa_codes(g, [bytes(x) for x in z["contig_names"]], contigs)
            with open(r, "wb") as f:
                for i in range(n):
                    for nm, row in ((bytes(z["names1"][i]), m1[i]), (bytes(z["names2"][i]), m2[i])):
                        f.write(b">" + nm + b"\n" + b"ACGT"[row[0]:row[0] + 1] + bytes(b"0123"[c] if c < 4 else ord(".") for c in row[1:]) + b"\n")
            ins = tuple(int(x) for x in z["ins"])
            p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-cs"), "-N", "4", "-p", str(z["mode"]), "-I", "%d,%d" % ins, "--sam-unaligned", *extra, r, g], capture_output=True, check=True)
            body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG") and not l.startswith(b"@RG"))
        with gzip.open(os.path.join(OUT, "%s@%s.sam.gz" % (base, tag)), "wb", compresslevel=9) as f:
            f.write(body)
        print("%s@%s: %d SAM records" % (base, tag, sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))))


def option_cases(only=None):
    """non-default options on inputs that are already committed: only the reference's SAM body is stored (<base>@<tag>.sam.gz)"""
    for tag, (base, extra) in OPTION_CASES.items():
        if only and tag not in only: continue
        z = np.load(os.path.join(OUT, base + ".npz"))
        contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
        with tempfile.TemporaryDirectory() as d:
            g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.fa")
            if "mates1" in z.files:
                cn = [bytes(x) for x in z["contig_names"]]
                write_fa_codes(g, cn, contigs)
                names = [bytes(n) for pair in zip(z["names1"], z["names2"]) for n in pair]
                seqs = [q for pair in zip(list(z["mates1"]), list(z["mates2"])) for q in pair]
                write_fa_codes(r, names, seqs)
                extra = ["-p", str(z["mode"]), "-I", "%d,%d" % tuple(int(x) for x in z["ins"]), *extra]
            else:
                write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
                write_fa_codes(r, [b"r%d" % i for i in range(len(z["reads"]))], list(z["reads"]))
            p = subprocess.run([REF, "-N", "4", *extra, r, g], capture_output=True, check=True)
            body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG") and not l.startswith(b"@RG"))     # (--read-group adds an @RG header line)
        with gzip.open(os.path.join(OUT, "%s@%s.sam.gz" % (base, tag)), "wb", compresslevel=9) as f:
            f.write(body)
        print("%s@%s: %d SAM records" % (base, tag, sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))))


def index_cases():
    """the reference's own index files (-S) for a tiny genome + the SAM it produces from them (-L); also with hashed seeds (-H)"""
    _index_case("idxfix", "11110111,1101011011", [])
    _index_case("idxfix_h", "1111011101111011,11011101101110111011", ["-H"])


def index_genome(short_and_n=False):
    """chrA / chrB of the index fixtures; short_and_n: + chrC / chrD / chrE of 31, 32 and 33 bases (a span-32 seed has no k-mer, one, two) and four single Ns: on
    chrA's second and last-but-one base (its first and last span-32 k-mer hold them under a 0 of the mask 1010...01 and nowhere else) and on chrB's first and last
    base (under the first and the last 1)"""
    rng = np.random.default_rng(5)
    c1 = rng.integers(0, 4, 12000, dtype=np.uint8); c1[3000:3040] = 15; c1[7000:7003] = [5, 6, 14]
    c2 = rng.integers(0, 4, 7003, dtype=np.uint8)
    if not short_and_n: return [c1, c2], [b"chrA", b"chrB"]
    short = [rng.integers(0, 4, n, dtype=np.uint8) for n in (31, 32, 33)]
    c1[1] = 15; c1[-2] = 15; c2[0] = 15; c2[-1] = 15
    return [c1, c2] + short, [b"chrA", b"chrB", b"chrC", b"chrD", b"chrE"]


def _index_case(dirname, seeds, extra, genome=None):
    import shutil
    contigs, names = genome if genome is not None else index_genome()
    c1, c2 = contigs[:2]
    reads, _ = synth.make_reads([c1, c2], 400, 50, 91)
    d = os.path.join(OUT, dirname); shutil.rmtree(d, ignore_errors=True); os.makedirs(d)
    with tempfile.TemporaryDirectory() as t:
        g = os.path.join(t, "g.fa"); r = os.path.join(t, "r.fa")
        write_fa_codes(g, names, contigs)
        write_fa_codes(r, [b"r%d" % i for i in range(len(reads))], list(reads))
        subprocess.run([REF, *extra, "-s", seeds, "-S", os.path.join(d, "idx"), g], capture_output=True, check=True)
        p = subprocess.run([REF, "-N", "2", "-L", os.path.join(d, "idx"), r], capture_output=True, check=True)
        body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    _npz_fixed(os.path.join(d, "inputs.npz"), **{"contig%d" % i: c for i, c in enumerate(contigs)}, reads=reads, seeds=np.array(seeds), contig_names=np.array(names))
    _gz_fixed(os.path.join(d, "from_index.sam.gz"), body)
    print(dirname + ": %d SAM records from the reference's -L run; files:" % sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@")), sorted(os.listdir(d)))


def _gz_fixed(path, data):
    """gzip without the time stamp: the same bytes on every run"""
    with open(path, "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, compresslevel=9, mtime=0) as f: f.write(data)


def _npz_fixed(path, **arrays):
    """np.savez_compressed with the members' time stamps fixed"""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)); info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f: np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def seeds_cases():
    """--seeds-only: the seed sets of tests/oracle_api.py SEED_SETS through the reference on committed inputs (SEED_RUNS), with --extra-sam-fields --sam-unaligned:
    the match count of a window (ZM) sees a seed's lists go missing where the SAM's other fields do not.  Only the records are stored, without the header.
    Then the two index fixtures of SEED_INDEX_CASES."""
    from tests import oracle_api as oa
    import shutil
    total = 0
    inputs = {}
    for run, (base, n, cs, n1) in oa.SEED_RUNS.items():
        if base not in inputs:
            z = np.load(os.path.join(OUT, base + ".npz"))
            inputs[base] = ([z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))], z["reads"])
    for name, (seeds, hashed) in oa.SEED_SETS.items():
        for run in oa.seed_runs(name):
            base, n, cs, n1 = oa.SEED_RUNS[run]
            contigs, reads = inputs[base]; reads = reads[:n] if n else reads
            with tempfile.TemporaryDirectory() as d:
                g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfasta" if cs else "r.fa")
                write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
                if cs: synth.write_csfasta_reads(r, reads)
                else: write_fa_codes(r, [b"r%d" % i for i in range(len(reads))], list(reads))
                # The reference does not return from --extra-sam-fields when a record on the negative strand has an N in its edit string (reverse_alignment_edit_string,
                # gmapper/output.c:83-122, knows A C G T only and spins): stress_100bp_unal has such reads and is stored without the extra fields (SEED_RUNS_NO_EXTRA).
                # Every run has a time limit, so that another such input ends the generator instead of hanging it.
                cmd = ["timeout", "-k", "5", "120", os.path.join(ROOT, "oracle", "_ref", "gmapper-cs" if cs else "gmapper-ls"), "-N", "4", "-s", ",".join(seeds),
                       *(["-H"] if hashed else []), *(["-n", "1"] if n1 else []), *([] if run in oa.SEED_RUNS_NO_EXTRA else ["--extra-sam-fields"]), "--sam-unaligned", r, g]
                p = subprocess.run(cmd, capture_output=True)
                assert p.returncode == 0, (name, run, p.returncode, p.stderr[-2000:])
            body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@"))
            path = os.path.join(OUT, "%s@seeds_%s%s.sam.gz" % (base, name, "_n1" if n1 else ""))
            _gz_fixed(path, body)
            recs = [l.split(b"\t", 3) for l in body.split(b"\n") if l]
            mapped = [t for t in recs if not int(t[1]) & 4]
            size = os.path.getsize(path); total += size
            assert size <= 734_000, (path, size)
            print("%s@seeds_%s%s: %d reads -> %d records, %d mapped, %d reads mapped, %d bytes" % (base, name, "_n1" if n1 else "", len(reads), len(recs), len(mapped),
                                                                                                  len({t[0] for t in mapped}), size))
    print("seed-set goldens: %d bytes" % total)
    seed_index_cases()


def seed_index_cases():
    from tests import oracle_api as oa
    for name, (seeds, hashed) in oa.SEED_INDEX_CASES.items():
        _index_case(name, ",".join(seeds), ["-H"] if hashed else [], genome=index_genome(short_and_n=True))
        d = os.path.join(OUT, name)
        for f in sorted(os.listdir(d)):      # the reference stamps its gzip files with the time: re-pack them so that a second run gives the same bytes
            if f.startswith("idx."):
                with gzip.open(os.path.join(d, f), "rb") as h: data = h.read()
                _gz_fixed(os.path.join(d, f), data)
            assert os.path.getsize(os.path.join(d, f)) <= 734_000, (name, f)
        print(name + ":", {f: os.path.getsize(os.path.join(d, f)) for f in sorted(os.listdir(d))})


def local_kat_cases():
    kat = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat"), "600", "local"], capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat_local.txt.gz"), "wb", compresslevel=9) as f:
        f.write(kat)
    print("sw_kat_local:", kat.count(b"\nL ") + 1, "sw_full_ls local-mode answers")


def cs_kat_cases():
    kat = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat_cs"), "700"], capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat_cs.txt.gz"), "wb", compresslevel=9) as f:
        f.write(kat)
    print("sw_kat_cs:", kat.count(b"\nC ") + 1, "colour-space vector,", kat.count(b"\nS "), "sw_full_cs")
    katl = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat_cs"), "400", "local"], capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat_cs_local.txt.gz"), "wb", compresslevel=9) as f:
        f.write(katl)
    print("sw_kat_cs_local:", katl.count(b"\nL ") + 1, "sw_full_cs in local mode")
    katx = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat_cs"), "500", "xover"], capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat_cs_xover.txt.gz"), "wb", compresslevel=9) as f:
        f.write(katx)
    print("sw_kat_cs_xover:", katx.count(b"\nX ") + 1, "sw_full_cs with per-position crossover scores,", katx.count(b"\nY "), "of them in local mode")
    katr = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat_cs"), "300", "rna"], capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat_cs_rna.txt.gz"), "wb", compresslevel=9) as f:
        f.write(katr)
    print("sw_kat_cs_rna:", katr.count(b"\nC ") + 1, "colour-space vector,", katr.count(b"\nS "), "+", katr.count(b"\nL "), "sw_full_cs (global + local), all on an RNA genome with is_rna = true")


def score_kat_cases():
    """the letter- and colour-space known answers once more under other score sets than the defaults (oracle/ref_kat.cpp, ref_kat_cs.cpp, mode "scores"): a P line with the
    setups' arguments opens each set"""
    for exe, name in (("ref_kat", "sw_kat_scores"), ("ref_kat_cs", "sw_kat_cs_scores")):
        kat = subprocess.run([os.path.join(ROOT, "oracle", "_ref", exe), "150", "scores"], capture_output=True, check=True).stdout
        path = os.path.join(OUT, name + ".txt.gz")
        with gzip.open(path, "wb", compresslevel=9) as f:
            f.write(kat)
        assert os.path.getsize(path) < 350_000, "cut cases per set, not sets"
        kinds = {}
        for l in kat.split(b"\n"):
            if l: kinds[l[:1].decode()] = kinds.get(l[:1].decode(), 0) + 1
        print("%s: %d sets," % (name, kinds.pop("P")), ", ".join("%d %s" % (v, k) for k, v in sorted(kinds.items())), "records")


def post_kat_cases():
    """the reference's own post_sw() on its own sw_full_cs results of sw_kat_cs.txt.gz (oracle/ref_kat_post.cpp), and its own sw_gapless() (oracle/ref_kat_gapless.cpp)"""
    src = gzip.open(os.path.join(OUT, "sw_kat_cs.txt.gz"), "rb").read()
    kat = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat_post")], input=src, capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat_post.txt.gz"), "wb", compresslevel=9) as f:
        f.write(kat)
    print("sw_kat_post:", kat.count(b"\nP "), "post_sw answers")
    kat = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat_gapless"), "1200"], capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat_gapless.txt.gz"), "wb", compresslevel=9) as f:
        f.write(kat)
    print("sw_kat_gapless:", kat.count(b"\nG ") + 1, "sw_gapless answers")
    katr = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat_gapless"), "600", "rna"], capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat_gapless_rna.txt.gz"), "wb", compresslevel=9) as f:
        f.write(katr)
    print("sw_kat_gapless_rna:", katr.count(b"\nG ") + 1, "colour-space sw_gapless answers on RNA genomes with is_rna = true")


def run_cs_case(name, contigs, reads, extra=()):
    """colour-space reads (codes[n, 1 + colours]) through the reference's gmapper-cs"""
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfasta")
        write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
        synth.write_csfasta_reads(r, reads)
        p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-cs"), "-N", "4", *extra, r, g], capture_output=True, check=True)
        body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    np.savez_compressed(os.path.join(OUT, name + ".npz"),
                        **{"contig%d" % i: c for i, c in enumerate(contigs)}, reads=reads)
    with gzip.open(os.path.join(OUT, name + ".sam.gz"), "wb", compresslevel=9) as f:
        f.write(body)
    n_map = sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))
    print(f"{name}: {len(reads)} colour-space reads -> {n_map} SAM records")


def cs_cases():
    contigs = synth.make_genome(synth.contig_lengths("cfg2", 0.02), 4)
    reads, _ = synth.make_cs_reads(contigs, 3000, 50, 4)
    run_cs_case("cfg4s_50col_2Mbp", contigs, reads)
    sg = stress_genome()
    reads, _ = synth.make_cs_reads([c for c in sg if len(c) > 200], 2000, 60, 5, p_col=0.03, p_dot=0.004)
    run_cs_case("stress_cs_60col_unal", sg, reads, extra=("--sam-unaligned",))
    # the reference's own colour-space index files (-S) for a tiny genome + the SAM gmapper-cs produces from them (-L)
    import shutil
    rng = np.random.default_rng(6)
    c1 = rng.integers(0, 4, 12000, dtype=np.uint8); c1[3000:3040] = 15; c1[7000:7003] = [5, 6, 14]
    c2 = rng.integers(0, 4, 7003, dtype=np.uint8)
    contigs = [c1, c2]; names = [b"chrA", b"chrB"]
    reads, _ = synth.make_cs_reads(contigs, 400, 40, 92)
    seeds = "11110111,1101011011"
    refcs = os.path.join(ROOT, "oracle", "_ref", "gmapper-cs")
    d = os.path.join(OUT, "idxfix_cs"); shutil.rmtree(d, ignore_errors=True); os.makedirs(d)
    with tempfile.TemporaryDirectory() as t:
        g = os.path.join(t, "g.fa"); r = os.path.join(t, "r.csfasta")
        write_fa_codes(g, names, contigs)
        synth.write_csfasta_reads(r, reads)
        subprocess.run([refcs, "-s", seeds, "-S", os.path.join(d, "idx"), g], capture_output=True, check=True)
        p = subprocess.run([refcs, "-N", "2", "-L", os.path.join(d, "idx"), r], capture_output=True, check=True)
        body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    np.savez_compressed(os.path.join(d, "inputs.npz"), contig0=c1, contig1=c2, reads=reads, seeds=np.array(seeds), contig_names=np.array(names))
    with gzip.open(os.path.join(d, "from_index.sam.gz"), "wb", compresslevel=9) as f:
        f.write(body)
    print("idxfix_cs: %d SAM records from gmapper-cs -L; files:" % sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@")), sorted(os.listdir(d)))


def cs_pair_case():
    """colour-space pairs through the reference's gmapper-cs -p <mode> (mates adjacent in one csfasta file): opp-in with unmappable mates and skipped
    cycles; the three modes that reverse a mate (read_reverse swaps the strands of a colour read) on 300 pairs each"""
    contigs = synth.make_genome([600_000, 400_000], 55)
    cn = [b"contig1", b"contig2"]; ins = (100, 600)
    rcl = lambda x: synth.COMPLEMENT[x[:, ::-1]]
    for mode, npairs, seed in (("opp-in", 800, 15), ("opp-out", 300, 21), ("col-fw", 300, 22), ("col-bw", 300, 23)):
        reads, _ = synth.make_pairs(contigs, npairs, 50, seed, ins_mean=250, ins_sd=30)
        a, b = reads[0::2].copy(), reads[1::2].copy()               # make_pairs yields opp-in mates: the other orientations are derived from them
        if mode == "opp-out": a, b = rcl(a), rcl(b)
        elif mode == "col-fw": b = rcl(b)
        elif mode == "col-bw": a = rcl(a)
        m1 = synth.cs_from_letters(a, 1); m2 = synth.cs_from_letters(b, 2)
        rng = np.random.default_rng(17)                               # some mates that map nowhere: half-paired records, unaligned pairs
        for i in range(len(m1)):
            if i % 20 == 7: m2[i, 1:] = rng.integers(0, 4, m2.shape[1] - 1)
            if i % 50 == 3: m1[i, 1:] = rng.integers(0, 4, m1.shape[1] - 1); m2[i, 1:] = rng.integers(0, 4, m2.shape[1] - 1)
            if i % 33 == 5: m1[i, 10] = 15                              # a skipped cycle ('.')
        n = len(m1); names1 = [b"p%d/1" % i for i in range(n)]; names2 = [b"p%d/2" % i for i in range(n)]
        name = "cs_pairs_50col_" + mode
        with tempfile.TemporaryDirectory() as d:
            g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfasta")
            write_fa_codes(g, cn, contigs)
            with open(r, "wb") as f:
                for i in range(n):
                    for nm, row in ((names1[i], m1[i]), (names2[i], m2[i])):
                        f.write(b">" + nm + b"\n" + b"ACGT"[row[0]:row[0] + 1] + bytes(b"0123"[c] if c < 4 else ord(".") for c in row[1:]) + b"\n")
            p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-cs"), "-N", "4", "-p", mode, "-I", "%d,%d" % ins, "--sam-unaligned", r, g], capture_output=True, check=True)
            body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **{"contig%d" % i: c for i, c in enumerate(contigs)}, mates1=m1, mates2=m2,
                            names1=np.array(names1), names2=np.array(names2), contig_names=np.array(cn), mode=np.array(mode), ins=np.array(ins))
        with gzip.open(os.path.join(OUT, name + ".sam.gz"), "wb", compresslevel=9) as f:
            f.write(body)
        print("%s: %d colour-space pairs -> %d SAM records" % (name, n, sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))))


def fastq_cases():
    """FASTQ input (-Q autodetected): the QUAL strings in the SAM, once PHRED+33 (--qv-offset 33), once the default PHRED+64"""
    z = np.load(os.path.join(OUT, "stress_100bp_unal.npz"))
    contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    reads = z["reads"][:600]
    rng = np.random.default_rng(17)
    T = np.frombuffer(b"ACGTUMRWSYKVHDBN", dtype=np.uint8)
    for tag, delta, extra in (("fq33", 33, ["--qv-offset", "33"]), ("fq64", 64, [])):
        q = (rng.integers(2, 41, size=reads.shape) + delta).astype(np.uint8)
        with tempfile.TemporaryDirectory() as d:
            g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.fq")
            write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
            with open(r, "wb") as f:
                for i in range(len(reads)):
                    f.write(b"@r%d\n" % i + T[reads[i]].tobytes() + b"\n+\n" + q[i].tobytes() + b"\n")
            p = subprocess.run([REF, "-N", "4", "--sam-unaligned", *extra, r, g], capture_output=True, check=True)
            body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
        np.savez_compressed(os.path.join(OUT, "stress_100bp_%s.npz" % tag), quals=q, n_reads=np.array(len(reads)), qual_delta=np.array(delta))
        with gzip.open(os.path.join(OUT, "stress_100bp_%s.sam.gz" % tag), "wb", compresslevel=9) as f:
            f.write(body)
        print("stress_100bp_%s: %d SAM records" % (tag, sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))))


def cs_fastq_cases():
    """colour-space FASTQ (csfastq, PHRED+33): per-position crossover scores, post_sw with read QVs, QUAL from post_sw, CQ:Z"""
    z = np.load(os.path.join(OUT, "cfg4s_50col_2Mbp.npz"))
    contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    reads = z["reads"][:1500]
    rng = np.random.default_rng(19)
    q = (rng.integers(2, 36, size=(reads.shape[0], reads.shape[1] - 1)) + 33).astype(np.uint8)
    tab = np.full(16, ord("."), dtype=np.uint8); tab[:4] = np.frombuffer(b"0123", dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfastq")
        write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
        with open(r, "wb") as f:
            for i in range(len(reads)):
                f.write(b"@r%d\n" % i + b"ACGT"[reads[i, 0]:reads[i, 0] + 1] + tab[reads[i, 1:]].tobytes() + b"\n+\n" + q[i].tobytes() + b"\n")
        p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-cs"), "-N", "4", "--sam-unaligned", r, g], capture_output=True)
        if p.returncode != 0:
            print(p.stderr.decode()[-2000:]); raise SystemExit(1)
        body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
        pl = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-cs"), "-N", "4", "--sam-unaligned", "--local", r, g], capture_output=True, check=True)      # the same reads with --local
        body_l = b"".join(l + b"\n" for l in pl.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    np.savez_compressed(os.path.join(OUT, "cfg4s_50col_fq.npz"), quals=q, n_reads=np.array(len(reads)), qual_delta=np.array(33))
    with gzip.open(os.path.join(OUT, "cfg4s_50col_fq.sam.gz"), "wb", compresslevel=9) as f:
        f.write(body)
    with gzip.open(os.path.join(OUT, "cfg4s_50col_fq@cs_fq_local.sam.gz"), "wb", compresslevel=9) as f:
        f.write(body_l)
    print("cfg4s_50col_fq: %d SAM records" % sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@")))


def paired_fastq_case():
    """paired FASTQ (mates adjacent in one file, PHRED+33): QUAL strings in the paired and half-paired records"""
    z = np.load(os.path.join(OUT, "stress_pairs_2x100.npz"))
    contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    cn = [bytes(x) for x in z["contig_names"]]
    m1, m2 = z["mates1"][:400], z["mates2"][:400]
    n1 = [bytes(x) for x in z["names1"]][:400]; n2 = [bytes(x) for x in z["names2"]][:400]
    rng = np.random.default_rng(23)
    q1 = (rng.integers(2, 41, size=m1.shape) + 33).astype(np.uint8); q2 = (rng.integers(2, 41, size=m2.shape) + 33).astype(np.uint8)
    T = np.frombuffer(b"ACGTUMRWSYKVHDBN", dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.fq")
        write_fa_codes(g, cn, contigs)
        with open(r, "wb") as f:
            for i in range(len(m1)):
                f.write(b"@" + n1[i] + b"\n" + T[m1[i]].tobytes() + b"\n+\n" + q1[i].tobytes() + b"\n")
                f.write(b"@" + n2[i] + b"\n" + T[m2[i]].tobytes() + b"\n+\n" + q2[i].tobytes() + b"\n")
        p = subprocess.run([REF, "-N", "4", "--qv-offset", "33", "--sam-unaligned", "-p", str(z["mode"]), "-I", "%d,%d" % tuple(int(x) for x in z["ins"]), r, g],
                           capture_output=True, check=True)
        body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    np.savez_compressed(os.path.join(OUT, "stress_pairs_fq33.npz"), quals1=q1, quals2=q2, n_pairs=np.array(len(m1)), qual_delta=np.array(33))
    with gzip.open(os.path.join(OUT, "stress_pairs_fq33.sam.gz"), "wb", compresslevel=9) as f:
        f.write(body)
    print("stress_pairs_fq33: %d SAM records" % sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@")))


def main():
    os.makedirs(OUT, exist_ok=True)
    if "--fastq-only" in sys.argv:
        fastq_cases(); cs_fastq_cases(); paired_fastq_case(); return
    if "--cs-only" in sys.argv:
        cs_cases(); return
    if "--cs-kat-only" in sys.argv:
        cs_kat_cases(); return
    if "--local-kat-only" in sys.argv:
        local_kat_cases(); return
    if "--post-kat-only" in sys.argv:
        post_kat_cases(); return
    if "--score-kat-only" in sys.argv:
        score_kat_cases(); return
    if "--cs-kat-only" in sys.argv:
        cs_kat_cases(); return
    if "--cs-pair-option-tags" in sys.argv:
        cs_pair_option_cases(only=sys.argv[sys.argv.index("--cs-pair-option-tags") + 1].split(",")); return
    if "--cs-pair-options-only" in sys.argv:
        cs_pair_option_cases(); return
    if "--cs-option-tags" in sys.argv:
        cs_option_cases(only=sys.argv[sys.argv.index("--cs-option-tags") + 1].split(",")); return
    if "--cs-options-only" in sys.argv:
        cs_option_cases(); return
    if "--index-only" in sys.argv:
        index_cases(); return
    if "--options-only" in sys.argv:
        option_cases(); return
    if "--option-tags" in sys.argv:                                   # --option-tags pairs_n3,cfg5_n3: just these
        option_cases(only=sys.argv[sys.argv.index("--option-tags") + 1].split(",")); return
    if "--chimeric-only" in sys.argv:
        chimeric_pairs_case(); option_cases(only=["chim_single_best_all", "chim_single_best_all_noimp", "chim_single_best"]); return
    if "--mirna-only" in sys.argv:
        mirna_case(); return
    if "--n1-only" in sys.argv:
        n1_noisy_case(); return
    if "--f1-twins-only" in sys.argv:
        f1_twins_case(); return
    if "--paired-only" in sys.argv:
        paired_cases(); return
    contigs, reads, _ = synth.make_config("cfg1")
    run_case("cfg1_36bp_1Mbp", contigs, reads)
    contigs, reads, _ = synth.make_config("cfg2", scale=0.02, n_reads=5000)
    run_case("cfg2s_100bp_2Mbp", contigs, reads)
    sg = stress_genome()
    run_case("stress_60bp", sg, stress_reads(sg, 3000, 60))
    run_case("stress_100bp_unal", sg, stress_reads(sg, 1500, 100, seed=90), extra=("--sam-unaligned",))
    kat = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_kat"), "1500"], capture_output=True, check=True).stdout
    with gzip.open(os.path.join(OUT, "sw_kat.txt.gz"), "wb", compresslevel=9) as f:
        f.write(kat)
    print("sw_kat:", kat.count(b"\nV ") + 1, "vector,", kat.count(b"\nF "), "full")
    paired_cases()
    chimeric_pairs_case()
    option_cases()
    n1_noisy_case()
    f1_twins_case()
    mirna_case()
    cs_option_cases()
    index_cases()
    cs_kat_cases()
    post_kat_cases()
    local_kat_cases()
    score_kat_cases()
    cs_cases()
    fastq_cases()
    cs_fastq_cases()
    paired_fastq_case()


def text_cases():
    """Text input: reads as the file's characters -- lower case, X / x / . for N, U, ambiguity codes; csfasta with '.', '4', 'N' for a skipped
    cycle and a lower-case primer -- through the reference with --sam-unaligned: what it prints verbatim from the file's text (SEQ of unaligned reads,
    CS:Z) and what it normalises.  Fixtures: the read lines themselves + the reference's SAM.  (With --local the reference exits on a reverse-strand
    clip that holds X or U -- "error in getting reverse complement", gmapper/output.c:213-216 -- so there is no golden for that.)"""
    rng = np.random.Generator(np.random.PCG64(2024))
    def run(exe, extra, reads_path, genome_path):
        p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", exe), "-N", "2", *extra, reads_path, genome_path], capture_output=True, check=True)
        return b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    z = np.load(os.path.join(OUT, "stress_100bp_unal.npz")); contigs = [z["contig%d" % i] for i in range(len(z.files) - 1)]; reads = z["reads"][:400]
    LET = b"ACGTUMRWSYKVHDBN"; lines = []
    for r in reads:
        t = bytearray(LET[c] for c in r)
        for i, c in enumerate(r):
            if c == 15: t[i] = b"NnXx."[rng.integers(0, 5)]
            elif rng.random() < 0.15: t[i] = t[i] + 32
        lines.append(bytes(t))
    for k in range(0, 400, 9):                        # reads that cannot map: SEQ shows their text (X . U kept, ambiguity codes -> N)
        t = bytearray(lines[k])
        for q in rng.integers(0, 100, 25): t[q] = b"XUx.uRYK"[rng.integers(0, 8)]
        lines[k] = bytes(t)
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.fa")
        write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
        with open(r, "wb") as f:
            for i, t in enumerate(lines): f.write(b">r%d\n" % i + t + b"\n")
        sam = run("gmapper-ls", ["--sam-unaligned"], r, g)
    with gzip.open(os.path.join(OUT, "text_ls_reads.txt.gz"), "wb", compresslevel=9) as f: f.write(b"\n".join(lines) + b"\n")
    with gzip.open(os.path.join(OUT, "text_ls_unal.sam.gz"), "wb", compresslevel=9) as f: f.write(sam)
    z = np.load(os.path.join(OUT, "stress_cs_60col_unal.npz")); contigs = [z["contig%d" % i] for i in range(len(z.files) - 1)]; reads = z["reads"][:300]
    lines = []
    for r in reads:
        t = bytearray(b"ACGT"[r[0]:r[0] + 1])
        for c in r[1:]: t += (b"0123"[c:c + 1] if c < 4 else b".4Nn"[rng.integers(0, 4):][:1])
        if rng.random() < 0.2: t[0] = t[0] + 32
        lines.append(bytes(t))
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfasta")
        write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
        with open(r, "wb") as f:
            for i, t in enumerate(lines): f.write(b">r%d\n" % i + t + b"\n")
        sam = run("gmapper-cs", ["--sam-unaligned"], r, g)
    with gzip.open(os.path.join(OUT, "text_cs_reads.txt.gz"), "wb", compresslevel=9) as f: f.write(b"\n".join(lines) + b"\n")
    with gzip.open(os.path.join(OUT, "text_cs_unal.sam.gz"), "wb", compresslevel=9) as f: f.write(sam)


def file_cases():
    """File input: reads files as users have them -- gzip, '#' comments, sequences folded over lines, descriptions after the name, reads of
    several lengths mixed, FASTQ with folded sequences, a read longer than --longest-read -- through the reference with --sam-unaligned.  Fixtures:
    the files themselves (data the reference read) + the reference's SAM."""
    rng = np.random.Generator(np.random.PCG64(4242))
    sg = stress_genome()
    def run(exe, extra, reads_path, genome_path):
        p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", exe), "-N", "2", "--sam-unaligned", *extra, reads_path, genome_path], capture_output=True, check=True)
        return b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    LET = b"ACGTUMRWSYKVHDBN"
    sets = [stress_reads(sg, 150, L, seed=300 + L) for L in (36, 50, 75, 100, 130)]
    recs = [(L, r) for rs in sets for L, r in ((rs.shape[1], x) for x in rs)]
    order = rng.permutation(len(recs))
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(sg))], sg)
        # (1) FASTA, gzip, folded lines, comments, descriptions
        fa = bytearray(b"# reads of five lengths\n; second comment line\n")
        for n, k in enumerate(order):
            L, r = recs[k]; t = bytes(LET[c] for c in r)
            fa += b">read_%d  len=%d some description\twith a tab\n" % (n, L)
            w = int(rng.integers(20, 80))
            for o in range(0, L, w): fa += t[o:o + w] + b"\n"
            if n % 37 == 0: fa += b"# a comment between reads\n"
        fa += b">too_long\n" + bytes(LET[c] for c in rng.integers(0, 4, 1100)) + b"\n>after_long\n" + bytes(LET[c] for c in recs[0][1]) + b"\n"
        with gzip.open(os.path.join(d, "r.fa.gz"), "wb") as f: f.write(bytes(fa))
        sam = run("gmapper-ls", [], os.path.join(d, "r.fa.gz"), g)
        with gzip.open(os.path.join(OUT, "file_ls_mixed.fa.gz"), "wb", compresslevel=9) as f: f.write(bytes(fa))
        with gzip.open(os.path.join(OUT, "file_ls_mixed.sam.gz"), "wb", compresslevel=9) as f: f.write(sam)
        print("file_ls_mixed:", sum(1 for l in sam.split(b"\n") if l and not l.startswith(b"@")), "records")
        # (2) FASTQ (PHRED+33), plain, sequence and qualities folded, three lengths
        fq = bytearray()
        for n, k in enumerate(order[:300]):
            L, r = recs[k]; t = bytes(LET[c] for c in r); q = bytes((rng.integers(2, 40, L) + 33).astype(np.uint8))
            fq += b"@fq%d extra\n" % n
            if n % 3 == 0: fq += t[:L // 2] + b"\n" + t[L // 2:] + b"\n+fq%d\n" % n + q[:L // 3] + b"\n" + q[L // 3:] + b"\n"
            else: fq += t + b"\n+\n" + q + b"\n"
        open(os.path.join(d, "r.fq"), "wb").write(bytes(fq))
        sam = run("gmapper-ls", ["--qv-offset", "33"], os.path.join(d, "r.fq"), g)
        with gzip.open(os.path.join(OUT, "file_ls_mixed.fq.gz"), "wb", compresslevel=9) as f: f.write(bytes(fq))
        with gzip.open(os.path.join(OUT, "file_ls_mixed_fq.sam.gz"), "wb", compresslevel=9) as f: f.write(sam)
        print("file_ls_mixed_fq:", sum(1 for l in sam.split(b"\n") if l and not l.startswith(b"@")), "records")
        # (3) csfasta, two lengths (reads of the committed colour-space cases, cut)
        z = np.load(os.path.join(OUT, "stress_cs_60col_unal.npz")); cc = [z["contig%d" % i] for i in range(len(z.files) - 1)]; cr = z["reads"][:400]
        gc = os.path.join(d, "gc.fa"); write_fa_codes(gc, [b"contig%d" % (i + 1) for i in range(len(cc))], cc)
        cf = bytearray(b"# csfasta\n")
        for n, r in enumerate(cr):
            L = 60 if n % 2 else 45
            cf += b">c%d_F3\n" % n + b"ACGT"[r[0]:r[0] + 1] + bytes(b"0123"[c] if c < 4 else ord(".") for c in r[1:1 + L]) + b"\n"
        with gzip.open(os.path.join(d, "r.csfasta.gz"), "wb") as f: f.write(bytes(cf))
        sam = run("gmapper-cs", [], os.path.join(d, "r.csfasta.gz"), gc)
        with gzip.open(os.path.join(OUT, "file_cs_mixed.csfasta.gz"), "wb", compresslevel=9) as f: f.write(bytes(cf))
        with gzip.open(os.path.join(OUT, "file_cs_mixed.sam.gz"), "wb", compresslevel=9) as f: f.write(sam)
        print("file_cs_mixed:", sum(1 for l in sam.split(b"\n") if l and not l.startswith(b"@")), "records")


def cs_paired_fastq_cases():
    """csfastq pairs (PHRED+33) through gmapper-cs -p <mode>: QV-dependent crossover scores and post_sw error rates for both mates, QUAL / CQ:Z in paired, half-paired
    and unaligned records; opp-in and a mode that reverses a mate (col-bw)"""
    for mode in ("opp-in", "col-bw"):
        z = np.load(os.path.join(OUT, "cs_pairs_50col_%s.npz" % mode))
        contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
        cn = [bytes(x) for x in z["contig_names"]]
        N = 300
        m1, m2 = z["mates1"][:N], z["mates2"][:N]; n1 = [bytes(x) for x in z["names1"]][:N]; n2 = [bytes(x) for x in z["names2"]][:N]
        rng = np.random.default_rng(31)
        q1 = (rng.integers(2, 36, size=(N, m1.shape[1] - 1)) + 33).astype(np.uint8); q2 = (rng.integers(2, 36, size=(N, m2.shape[1] - 1)) + 33).astype(np.uint8)
        tab = np.full(16, ord("."), dtype=np.uint8); tab[:4] = np.frombuffer(b"0123", dtype=np.uint8)
        with tempfile.TemporaryDirectory() as d:
            g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfastq")
            write_fa_codes(g, cn, contigs)
            with open(r, "wb") as f:
                for i in range(N):
                    for nm, row, q in ((n1[i], m1[i], q1[i]), (n2[i], m2[i], q2[i])):
                        f.write(b"@" + nm + b"\n" + b"ACGT"[row[0]:row[0] + 1] + tab[row[1:]].tobytes() + b"\n+\n" + q.tobytes() + b"\n")
            p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-cs"), "-N", "4", "--sam-unaligned", "-p", mode, "-I", "%d,%d" % tuple(int(x) for x in z["ins"]), r, g],
                               capture_output=True)
            if p.returncode != 0:
                print(p.stderr.decode()[-1500:]); raise SystemExit(1)
            body = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
            pl = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-cs"), "-N", "4", "--sam-unaligned", "--local", "-p", mode, "-I", "%d,%d" % tuple(int(x) for x in z["ins"]), r, g],
                                capture_output=True)
            if pl.returncode != 0:
                print(pl.stderr.decode()[-1500:]); raise SystemExit(1)
            with gzip.open(os.path.join(OUT, "cs_pairs_fq_%s@cs_pairs_fq_local.sam.gz" % mode), "wb", compresslevel=9) as f:      # the same pairs with --local
                f.write(b"".join(l + b"\n" for l in pl.stdout.split(b"\n") if l and not l.startswith(b"@PG")))
        np.savez_compressed(os.path.join(OUT, "cs_pairs_fq_%s.npz" % mode), quals1=q1, quals2=q2, n_pairs=np.array(N), qual_delta=np.array(33))
        with gzip.open(os.path.join(OUT, "cs_pairs_fq_%s.sam.gz" % mode), "wb", compresslevel=9) as f:
            f.write(body)
        print("cs_pairs_fq_%s: %d SAM records" % (mode, sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@"))))


def pair_file_cases():
    """paired file input: (1) gmapper -1 a.fq.gz -2 b.fq.gz, PHRED+33, mates cut to a mix of lengths; (2) one FASTA file with the mates adjacent (folded lines,
    comments).  Fixtures: the files themselves + the reference's SAM."""
    z = np.load(os.path.join(OUT, "stress_pairs_2x100.npz"))
    contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    cn = [bytes(x) for x in z["contig_names"]]
    N = 360; m1, m2 = z["mates1"][:N], z["mates2"][:N]
    rng = np.random.default_rng(77); T = np.frombuffer(b"ACGTUMRWSYKVHDBN", dtype=np.uint8)
    l1 = rng.choice([100, 80, 64], size=N); l2 = rng.choice([100, 60], size=N)
    ins = tuple(int(x) for x in z["ins"])
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); write_fa_codes(g, cn, contigs)
        a = bytearray(); b = bytearray(); il = bytearray(b"# pairs, mates adjacent\n")
        for i in range(N):
            s1 = T[m1[i][:l1[i]]].tobytes(); s2 = T[m2[i][100 - l2[i]:]].tobytes()     # mate 2 keeps its 3' part, so that the pair still spans the insert
            q1 = bytes((rng.integers(2, 40, l1[i]) + 33).astype(np.uint8)); q2 = bytes((rng.integers(2, 40, l2[i]) + 33).astype(np.uint8))
            a += b"@q%d/1 first mate\n" % i + s1 + b"\n+\n" + q1 + b"\n"; b += b"@q%d/2\n" % i + s2 + b"\n+\n" + q2 + b"\n"
            il += b">q%d/1\n" % i + s1[:50] + b"\n" + s1[50:] + b"\n>q%d/2 desc\n" % i + s2 + b"\n"
        with gzip.open(os.path.join(d, "a.fq.gz"), "wb") as f: f.write(bytes(a))
        with gzip.open(os.path.join(d, "b.fq.gz"), "wb") as f: f.write(bytes(b))
        open(os.path.join(d, "il.fa"), "wb").write(bytes(il))
        run = lambda args: b"".join(l + b"\n" for l in subprocess.run([REF, "-N", "4", "--sam-unaligned", "-p", str(z["mode"]), "-I", "%d,%d" % ins, *args, g],
                                                                        capture_output=True, check=True).stdout.split(b"\n") if l and not l.startswith(b"@PG"))
        sam12 = run(["--qv-offset", "33", "-1", os.path.join(d, "a.fq.gz"), "-2", os.path.join(d, "b.fq.gz")])
        samil = run([os.path.join(d, "il.fa")])
    for nm, data in (("file_pairs_1.fq.gz", bytes(a)), ("file_pairs_2.fq.gz", bytes(b)), ("file_pairs_il.fa.gz", bytes(il)), ("file_pairs_12.sam.gz", sam12), ("file_pairs_il.sam.gz", samil)):
        with gzip.open(os.path.join(OUT, nm), "wb", compresslevel=9) as f: f.write(data)
    print("file_pairs_12:", sum(1 for l in sam12.split(b"\n") if l and not l.startswith(b"@")), "records; file_pairs_il:", sum(1 for l in samil.split(b"\n") if l and not l.startswith(b"@")))


PREPROCESS_CASES = {
    # tag: (input fixture, options of the reference, gm_params_t fields): the read loop's preprocessing (ref: gmapper.c:262-284,427-472,495-521)
    "pre_trim": ("pre_reads.fa.gz", ["--trim-front", "3", "--trim-end", "5"], {"trim_front": 3, "trim_end": 5}),
    "pre_q_default": ("pre_reads.fq.gz", ["--qv-offset", "64"], {}),                                    # --min-avg-qv is 10 unless told otherwise: low-quality reads get no record
    "pre_q_min20": ("pre_reads.fq.gz", ["--qv-offset", "64", "--min-avg-qv", "20"], {"min_avg_qv": 20}),
    "pre_q_none": ("pre_reads.fq.gz", ["--qv-offset", "64", "--min-avg-qv", "-1"], {"min_avg_qv": -1}),
    "pre_q_illumina": ("pre_reads.fq.gz", ["--qv-offset", "64", "--trim-illumina"], {"trim_illumina": 1}),
    "pre_q_ignore": ("pre_reads.fq.gz", ["--qv-offset", "64", "--ignore-qvs"], {"ignore_qvs": 1}),
    "pre_q_trim": ("pre_reads.fq.gz", ["--qv-offset", "64", "--trim-front", "2", "--trim-end", "3", "--trim-illumina"], {"trim_front": 2, "trim_end": 3, "trim_illumina": 1}),
}


def preprocess_cases():
    """The read loop's preprocessing through the reference: --trim-front / --trim-end, --trim-illumina, --min-avg-qv (default 10), --ignore-qvs on a FASTA and a FASTQ
    (PHRED+64) file of mixed lengths, and --trim-second on the pair files of pair_file_cases.  Fixtures: the files + the reference's SAM per option set."""
    rng = np.random.Generator(np.random.PCG64(5151))
    sg = stress_genome()
    LET = b"ACGTUMRWSYKVHDBN"
    sets = [stress_reads(sg, 120, L, seed=500 + L) for L in (50, 75, 100)]
    recs = [r for rs in sets for r in rs]
    order = rng.permutation(len(recs))
    fa = bytearray(); fq = bytearray()
    for n, k in enumerate(order):
        r = recs[k]; L = len(r); t = bytes(LET[c] for c in r)
        fa += b">t%d\n" % n + t + b"\n"
        kind = n % 6
        if kind == 0: q = rng.integers(2, 9, L)                                    # poor read: mean below 10
        elif kind == 1: q = rng.integers(8, 24, L)                                 # mean around 15: kept by default, dropped at 20
        else: q = rng.integers(15, 41, L)
        if kind in (2, 3): q[L - int(rng.integers(1, 12)):] = 2                    # an Illumina "B" tail (PHRED+64: 'B' = quality 2)
        if n % 41 == 0: q[:] = 2                                                   # all B: --trim-illumina leaves nothing
        fq += b"@t%d\n" % n + t + b"\n+\n" + bytes((q + 64).astype(np.uint8)) + b"\n"
    with gzip.open(os.path.join(OUT, "pre_reads.fa.gz"), "wb", compresslevel=9) as f: f.write(bytes(fa))
    with gzip.open(os.path.join(OUT, "pre_reads.fq.gz"), "wb", compresslevel=9) as f: f.write(bytes(fq))
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(sg))], sg)
        open(os.path.join(d, "pre_reads.fa.gz"), "wb").write(gzip.compress(bytes(fa))); open(os.path.join(d, "pre_reads.fq.gz"), "wb").write(gzip.compress(bytes(fq)))
        for tag, (src, extra, _) in PREPROCESS_CASES.items():
            p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", "gmapper-ls"), "-N", "2", "--sam-unaligned", *extra, os.path.join(d, src), g], capture_output=True)
            if p.returncode != 0: print(p.stderr.decode()[-1500:]); raise SystemExit(1)
            sam = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
            with gzip.open(os.path.join(OUT, tag + ".sam.gz"), "wb", compresslevel=9) as f: f.write(sam)
            print(tag + ":", sum(1 for l in sam.split(b"\n") if l and not l.startswith(b"@")), "records")
    # pairs: --trim-second (the second mate only; the reference trims a first mate after packing it, see gm_check_pair_trim)
    z = np.load(os.path.join(OUT, "stress_pairs_2x100.npz"))
    contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    cn = [bytes(x) for x in z["contig_names"]]; ins = tuple(int(x) for x in z["ins"])
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); write_fa_codes(g, cn, contigs)
        for nm in ("file_pairs_1.fq.gz", "file_pairs_2.fq.gz"): open(os.path.join(d, nm), "wb").write(open(os.path.join(OUT, nm), "rb").read())
        p = subprocess.run([REF, "-N", "4", "--sam-unaligned", "-p", str(z["mode"]), "-I", "%d,%d" % ins, "--qv-offset", "33", "--trim-second", "--trim-front", "2", "--trim-end", "4",
                            "-1", os.path.join(d, "file_pairs_1.fq.gz"), "-2", os.path.join(d, "file_pairs_2.fq.gz"), g], capture_output=True)
        if p.returncode != 0: print(p.stderr.decode()[-1500:]); raise SystemExit(1)
        sam = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
    with gzip.open(os.path.join(OUT, "pre_pairs_trim_second.sam.gz"), "wb", compresslevel=9) as f: f.write(sam)
    print("pre_pairs_trim_second:", sum(1 for l in sam.split(b"\n") if l and not l.startswith(b"@")), "records")


FORMAT_CASES = {
    # tag: (base golden, program, options): the reference's SHRiMP-format / pretty output, whole (its #FORMAT line included)
    "fmt_shrimp": ("stress_60bp", "gmapper-ls", ["--shrimp-format"]),
    "fmt_pretty_R": ("stress_60bp", "gmapper-ls", ["-P", "-R"]),
    "fmt_local_pretty": ("stress_100bp_unal", "gmapper-ls", ["--local", "-P"]),
    "fmt_cs_shrimp_R": ("stress_cs_60col_unal", "gmapper-cs", ["--shrimp-format", "-R"]),
    "fmt_cs_pretty": ("stress_cs_60col_unal", "gmapper-cs", ["-P"]),
    # pairs: one line per mate under the mate's own name, ">name" for the unmapped mate of a half-paired mapping
    "fmt_pairs_shrimp_R": ("stress_pairs_2x100", "gmapper-ls", ["--shrimp-format", "-R"]),
    "fmt_pairs_pretty": ("pairfix_opp-out", "gmapper-ls", ["-P"]),
    "fmt_pairs_colbw": ("pairfix_col-bw", "gmapper-ls", ["--shrimp-format"]),
    "fmt_cs_pairs_pretty_R": ("cs_pairs_50col_col-bw", "gmapper-cs", ["-P", "-R"]),
    "fmt_cs_pairs_shrimp": ("cs_pairs_50col_opp-in", "gmapper-cs", ["--shrimp-format"]),
}


def format_cases():
    for tag, (base, exe, extra) in FORMAT_CASES.items():
        z = np.load(os.path.join(OUT, base + ".npz"))
        contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
        with tempfile.TemporaryDirectory() as d:
            g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.fa")
            write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
            if "mates1" in z.files:
                write_fa_codes(g, [bytes(x) for x in z["contig_names"]], contigs)
                names = [bytes(n) for pair in zip(z["names1"], z["names2"]) for n in pair]
                seqs = [q for pair in zip(list(z["mates1"]), list(z["mates2"])) for q in pair]
                if exe == "gmapper-cs":
                    tab = np.full(16, ord("."), dtype=np.uint8); tab[:4] = np.frombuffer(b"0123", dtype=np.uint8)
                    with open(r, "wb") as f:
                        for nm, q in zip(names, seqs): f.write(b">" + nm + b"\n" + b"ACGT"[q[0]:q[0] + 1] + tab[q[1:]].tobytes() + b"\n")
                else: write_fa_codes(r, names, seqs)
                extra = ["-p", str(z["mode"]), "-I", "%d,%d" % tuple(int(x) for x in z["ins"]), *extra]
            elif exe == "gmapper-cs": synth.write_csfasta_reads(r, z["reads"])
            else: write_fa_codes(r, [b"r%d" % i for i in range(len(z["reads"]))], list(z["reads"]))
            p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", exe), "-N", "4", *extra, r, g], capture_output=True, check=True)
        with gzip.open(os.path.join(OUT, "%s@%s.txt.gz" % (base, tag)), "wb", compresslevel=9) as f:
            f.write(p.stdout)
        print("%s@%s: %d mappings" % (base, tag, p.stdout.count(b"\n>")))


RNA_CASES = {
    # tag: (binary, genome fixture, read fixtures, options of the reference): RNA sequences -- uracil and no thymine (ref: fasta.c:528-542).  A contig's flag decides its
    # reverse complement (A -> U) and its colour translation (U read as T; genome.c:1107-1118); the LAST contig's flag is genome_is_rna, which the SW calls get
    # (genome.c:1063-1064; mapping.c:375-388,1318-1327); a letter-space read's own flag decides its reverse complement (gmapper.c:487).
    "rna_ls": ("gmapper-ls", "rna_genome.fa.gz", ["rna_reads_ls.fa.gz"], []),
    "rna_ls_pairs": ("gmapper-ls", "rna_genome.fa.gz", ["rna_pairs_1.fa.gz", "rna_pairs_2.fa.gz"], ["-p", "opp-in", "-I", "100,500"]),
    "rna_ls_last_dna": ("gmapper-ls", "rna_genome_last_dna.fa.gz", ["rna_reads_ls.fa.gz"], []),
    "rna_cs": ("gmapper-cs", "rna_genome.fa.gz", ["rna_reads_cs.fa.gz"], []),
    "rna_cs_fq": ("gmapper-cs", "rna_genome.fa.gz", ["rna_reads_cs.fq.gz"], ["--qv-offset", "33"]),
    "rna_cs_last_dna": ("gmapper-cs", "rna_genome_last_dna.fa.gz", ["rna_reads_cs.fa.gz"], []),
    "rna_cs_last_rna": ("gmapper-cs", "rna_genome_last_rna.fa.gz", ["rna_reads_cs.fa.gz"], []),
    "rna_cs_ungapped": ("gmapper-cs", "rna_genome.fa.gz", ["rna_reads_cs.fa.gz"], ["--local", "-U"]),
}


def rna_cases():
    """RNA genomes and RNA reads through the reference.  Fixtures: three genome files (two RNA contigs; the same + a DNA contig last; the DNA contig first), letter-space
    reads spelled in RNA, in DNA and in both, mate files, colour reads with and without QVs, and the reference's SAM for each combination of RNA_CASES."""
    rng = np.random.Generator(np.random.PCG64(9090))
    def contig(n, p_last):                                                          # codes 0..2 + `last` (3 = T, 4 = U), the last letter rare so that colour reads survive
        return rng.choice(np.array([0, 1, 2, 9], dtype=np.uint8), size=n, p=[0.32, 0.30, 0.30, 0.08])
    rna1 = contig(30000, 0); rna2 = contig(20000, 0); dna3 = contig(20000, 0)
    rna1[rna1 == 9] = 4; rna2[rna2 == 9] = 4; dna3[dna3 == 9] = 3
    rna2[5000:5040] = 15                                                            # a run of N
    LET = b"ACGTUMRWSYKVHDBN"
    def fa(names, seqs):
        out = bytearray()
        for nm, sq in zip(names, seqs):
            out += b">" + nm + b"\n"; t = bytes(LET[c] for c in sq)
            for k in range(0, len(t), 60): out += t[k:k + 60] + b"\n"
        return bytes(out)
    genomes = {"rna_genome.fa.gz": fa([b"rna1", b"rna2"], [rna1, rna2]),
               "rna_genome_last_dna.fa.gz": fa([b"rna1", b"rna2", b"dna3"], [rna1, rna2, dna3]),
               "rna_genome_last_rna.fa.gz": fa([b"dna3", b"rna1", b"rna2"], [dna3, rna1, rna2])}
    contigs = [rna1, rna2, dna3]
    def draw(L, nsub, indel):
        c = contigs[int(rng.integers(0, 3))]
        p = int(rng.integers(0, len(c) - L - 8)); s = c[p:p + L + 4].copy()
        if indel == 1: s = np.delete(s, int(rng.integers(10, L - 10)))
        elif indel == 2: s = np.insert(s, int(rng.integers(10, L - 10)), int(rng.integers(0, 3)))
        s = s[:L].copy()
        for _ in range(nsub): s[int(rng.integers(0, L))] = int(rng.integers(0, 3))
        return s
    def revcomp(s, rna):                                                            # a molecule's other strand, spelled like the first
        cm = np.array([4 if rna else 3, 2, 1, 0, 0, 10, 9, 7, 8, 6, 5, 14, 13, 12, 11, 15], dtype=np.uint8)
        return cm[s[::-1]]
    # letter space: 360 reads of 60 letters
    ls = bytearray()
    for n in range(360):
        s = draw(60, int(rng.integers(0, 4)), int(rng.integers(0, 6)) if n % 3 == 0 else 0)
        rna = bool((s == 4).any())
        if n % 2: s = revcomp(s, rna)
        kind = n % 12
        if kind == 5: s = np.where(s == 4, 3, s).astype(np.uint8)                  # an RNA molecule spelled with T
        elif kind == 7:                                                            # both U and T: not RNA to the reference
            s = s.copy(); idx = np.flatnonzero((s == 4) | (s == 3))
            if len(idx) >= 2: s[idx[0]] = 3; s[idx[1]] = 4
        elif kind == 9: s = s.copy(); s[int(rng.integers(0, 60))] = 15
        ls += b">r%d\n" % n + bytes(LET[c] for c in s) + b"\n"
    # mates: opp-in, inserts of 150-400, the molecule spelled in its contig's alphabet
    m1 = bytearray(); m2 = bytearray()
    for n in range(160):
        c = contigs[int(rng.integers(0, 2))]; ins = int(rng.integers(150, 400)); p = int(rng.integers(0, len(c) - ins))
        frag = c[p:p + ins].copy()
        for _ in range(int(rng.integers(0, 4))): frag[int(rng.integers(0, ins))] = int(rng.integers(0, 3))
        a = frag[:50]; b = revcomp(frag[-50:], True)
        if n % 2: a, b = b, a
        if n % 10 == 3: b = draw(50, 0, 0)                                          # a mate from somewhere else
        m1 += b">p%d/1\n" % n + bytes(LET[x] for x in a) + b"\n"; m2 += b">p%d/2\n" % n + bytes(LET[x] for x in b) + b"\n"
    # colour space: 400 reads of 40 colours (primer T), with QVs in the FASTQ twin
    cm4 = np.array([[0, 1, 2, 3], [1, 0, 3, 2], [2, 3, 0, 1], [3, 2, 1, 0]])
    cs = bytearray(); cq = bytearray()
    for n in range(400):
        s = draw(40, 0, int(rng.integers(0, 6)) if n % 4 == 0 else 0)
        if n % 2: s = revcomp(s, False)
        s = np.where(s == 4, 3, s); s = np.where(s > 3, 0, s)
        cols = [int(cm4[3][s[0]])] + [int(cm4[s[k]][s[k + 1]]) for k in range(39)]
        for _ in range(int(rng.integers(0, 3))): cols[int(rng.integers(0, 40))] = int(rng.integers(0, 4))
        t = b"T" + bytes(48 + c for c in cols)
        if n % 37 == 0: t = t[:20] + b"." + t[21:]
        q = rng.integers(8, 38, 40)
        cs += b">c%d\n" % n + t + b"\n"; cq += b"@c%d\n" % n + t + b"\n+\n" + bytes((q + 33).astype(np.uint8)) + b"\n"
    reads = {"rna_reads_ls.fa.gz": bytes(ls), "rna_pairs_1.fa.gz": bytes(m1), "rna_pairs_2.fa.gz": bytes(m2), "rna_reads_cs.fa.gz": bytes(cs), "rna_reads_cs.fq.gz": bytes(cq)}
    for nm, data in {**genomes, **reads}.items():
        with gzip.open(os.path.join(OUT, nm), "wb", compresslevel=9) as f: f.write(data)
    with tempfile.TemporaryDirectory() as d:
        for nm, data in genomes.items(): open(os.path.join(d, nm[:-3]), "wb").write(data)
        for nm, data in reads.items(): open(os.path.join(d, nm), "wb").write(gzip.compress(data))
        for tag, (binary, g, rds, extra) in RNA_CASES.items():
            files = [os.path.join(d, r) for r in rds]
            if len(files) == 2: files = ["-1", files[0], "-2", files[1]]
            p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", binary), "-N", "2", "--sam-unaligned", *extra, *files, os.path.join(d, g[:-3])], capture_output=True)
            if p.returncode != 0: print(p.stderr.decode()[-1500:]); raise SystemExit(1)
            sam = b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG"))
            with gzip.open(os.path.join(OUT, tag + ".sam.gz"), "wb", compresslevel=9) as f: f.write(sam)
            recs = [l for l in sam.split(b"\n") if l and not l.startswith(b"@")]
            print(tag + ":", len(recs), "records,", sum(1 for l in recs if not int(l.split(b"\t")[1]) & 4), "mapped")


# Paired mode at its edges (tests/test_pair_edges.py): mates of 40 and 60 bases under -I 200,400, perfect matches cut from a fragment of f bases.  The reference pairs
# an opp-in fragment iff 180 <= f <= 420; the other modes' mates are the opp-in mates with one or both reverse-complemented (as cs_pair_case derives them), which moves
# both transitions up by PE_SHIFT[mode].
PE_LEN = (40, 60); PE_INS = (200, 400); PE_HALF = 24
PE_SHIFT = {"opp-in": 0, "opp-out": 100, "col-fw": 60, "col-bw": 40}
PE_OPTION_SETS = {None: [], "pe_nhp": ["--no-half-paired"], "pe_n3": ["-n", "3"], "pe_n3_nhp": ["-n", "3", "--no-half-paired"]}
PE_CS_OPTION_SETS = {None: [], "pe_nhp": ["--no-half-paired"]}
PH_OPTION_SETS = {None: [], "ph_o3_strata": ["-o", "3", "--strata"]}


def _rc(x): return synth.COMPLEMENT[x[::-1]]


def pe_mates(c1, c2, p, f, strand, mode, shifted=False):
    """the mates of the fragment [p, p + f): mate 1 (40 bases) from contig c1, mate 2 (60 bases) from contig c2 -- one contig unless the pair is a cross-contig one.
    strand "m": the fragment's reverse complement was sequenced.  shifted: mate 2 spans 62 bases of the fragment and lacks the two in its middle."""
    n2 = PE_LEN[1] + (2 if shifted else 0)
    if strand == "p": a = c1[p:p + PE_LEN[0]]; t = _rc(c2[p + f - n2:p + f])
    else: a = _rc(c1[p + f - PE_LEN[0]:p + f]); t = c2[p:p + n2]
    if shifted: t = np.delete(t, [n2 // 2 - 1, n2 // 2])
    b = t
    if mode == "opp-out": a, b = _rc(a), _rc(b)
    elif mode == "col-fw": b = _rc(b)
    elif mode == "col-bw": a = _rc(a)
    assert len(a) == PE_LEN[0] and len(b) == PE_LEN[1]
    return a.astype(np.uint8), b.astype(np.uint8)


def pe_pairs(contigs, mode, t_lo, t_hi):
    """the pairs of one pair_edges fixture and their names, which say what each pair is:
         lo_<s>_<f> / hi_<s>_<f>    the sweep: f = t - 24 ... t + 24 about the lower / upper transition, fragment strand s (p / m), starts 41 apart on contig 1
         slo_p_<f> / shi_p_<f>      the shifted series: the same offsets, a 2-base deletion in the middle of mate 2
         x_<s>_<k>                  cross-contig: mate 1 from contig 1, mate 2 from the same offsets of contig 2, f in the middle of the bounds
         e_<c><a|b>_<s>_<lo|hi>_<d> ends: the fragment begins d bases behind the first base (a) or ends d bases before the last base (b) of contig c, f just inside a bound"""
    c1, c2 = contigs
    out = []; p = 1000
    for series, t, strands, shifted in (("lo", t_lo, "pm", False), ("hi", t_hi, "pm", False), ("slo", t_lo, "p", True), ("shi", t_hi, "p", True)):
        for s in strands:
            for f in range(t - PE_HALF, t + PE_HALF + 1):
                out.append((b"%s_%s_%d" % (series.encode(), s.encode(), f), pe_mates(c1, c1, p, f, s, mode, shifted))); p += 41
    for s in "pm":
        for k in range(10):
            out.append((b"x_%s_%d" % (s.encode(), k), pe_mates(c1, c2, p, (t_lo + t_hi) // 2, s, mode))); p += 41
    assert p + t_hi + PE_HALF + 100 < len(c1) - 1000
    for ci, c in enumerate(contigs):
        for end in "ab":
            for s in "pm":
                for which, f in (("lo", t_lo), ("hi", t_hi)):
                    for d in (0, 1, 7, 30):
                        q = d if end == "a" else len(c) - d - f
                        out.append((b"e_%d%s_%s_%s_%d" % (ci + 1, end.encode(), s.encode(), which.encode(), d), pe_mates(c, c, q, f, s, mode)))
    names = [n for n, _ in out]
    return np.stack([m[0] for _, m in out]), np.stack([m[1] for _, m in out]), names


def _ref_pairs_body(contigs, cn, m1, m2, names, mode, ins, extra, cs=False):
    """the reference's SAM body (no @PG / @RG line) for mates adjacent in one file; cs: m1 / m2 are colour reads behind their primer, through gmapper-cs --sam-unaligned"""
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfasta" if cs else "r.fa")
        write_fa_codes(g, cn, contigs)
        n1 = [n + b"/1" for n in names]; n2 = [n + b"/2" for n in names]
        if cs:
            with open(r, "wb") as f:
                for i in range(len(m1)):
                    for nm, row in ((n1[i], m1[i]), (n2[i], m2[i])):
                        f.write(b">" + nm + b"\n" + b"ACGT"[row[0]:row[0] + 1] + bytes(b"0123"[c] if c < 4 else ord(".") for c in row[1:]) + b"\n")
        else:
            write_fa_codes(r, [n for pair in zip(n1, n2) for n in pair], [q for pair in zip(list(m1), list(m2)) for q in pair])
        exe = os.path.join(ROOT, "oracle", "_ref", "gmapper-cs" if cs else "gmapper-ls")
        p = subprocess.run([exe, "-N", "4", "-p", mode, "-I", "%d,%d" % ins, *(["--sam-unaligned"] if cs else []), *extra, r, g], capture_output=True, check=True)
    return b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG") and not l.startswith(b"@RG"))


def _paired_names(body):
    """names of the pairs the SAM body holds as proper pairs (flag 0x2)"""
    return {l.split(b"\t")[0] for l in body.split(b"\n") if l and not l.startswith(b"@") and int(l.split(b"\t")[1]) & 2}


def _write_pair_fixture(name, contigs, cn, m1, m2, names, mode, ins, option_sets, cs=False):
    for tag, extra in option_sets.items():
        body = _ref_pairs_body(contigs, cn, m1, m2, names, mode, ins, extra, cs)
        with gzip.open(os.path.join(OUT, name + ("@" + tag if tag else "") + ".sam.gz"), "wb", compresslevel=9) as f:
            f.write(body)
        print("%s%s: %d pairs -> %d SAM records, %d proper pairs" % (name, "@" + tag if tag else "", len(m1),
              sum(1 for l in body.split(b"\n") if l and not l.startswith(b"@")), len(_paired_names(body))))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **{"contig%d" % i: c for i, c in enumerate(contigs)}, mates1=m1, mates2=m2,
                        names1=np.array([n + b"/1" for n in names]), names2=np.array([n + b"/2" for n in names]), contig_names=np.array(cn),
                        mode=np.array(mode), ins=np.array(ins))


def pair_edges_cases():
    """pair_edges_<mode> (letter space, four option sets), pair_edges_cs_opp-in / _col-bw (colour space, two option sets), pair_heap_tandem / pair_heap_ties"""
    contigs = synth.make_genome([30000, 30000], 77); cn = [b"contig1", b"contig2"]
    for mode, s in PE_SHIFT.items():
        t_lo, t_hi = 180 + s, 420 + s
        m1, m2, names = pe_pairs(contigs, mode, t_lo, t_hi)
        _write_pair_fixture("pair_edges_" + mode, contigs, cn, m1, m2, names, mode, PE_INS, PE_OPTION_SETS)
    # colour space: the windows are longer, so the transitions lie elsewhere -- one coarse run over f = 100 ... 600 on one strand finds them
    for mode in ("opp-in", "col-bw"):
        fs = list(range(100, 601))
        mm = [pe_mates(contigs[0], contigs[0], 1000 + 41 * k, f, "p", mode) for k, f in enumerate(fs)]
        a = synth.cs_from_letters(np.stack([m[0] for m in mm]), 1, p_col=0); b = synth.cs_from_letters(np.stack([m[1] for m in mm]), 2, p_col=0)
        names = [b"c_%d" % f for f in fs]
        got = _paired_names(_ref_pairs_body(contigs, cn, a, b, names, mode, PE_INS, [], cs=True))
        mid = (PE_INS[0] + PE_INS[1]) // 2 + PE_SHIFT[mode]
        assert b"c_%d" % mid in got, "the coarse colour-space run does not pair the middle of the bounds"
        t_lo = t_hi = mid
        while b"c_%d" % (t_lo - 1) in got: t_lo -= 1
        while b"c_%d" % (t_hi + 1) in got: t_hi += 1
        print("pair_edges_cs_%s: the reference pairs %d <= f <= %d" % (mode, t_lo, t_hi))
        m1, m2, names = pe_pairs(contigs, mode, t_lo, t_hi)
        _write_pair_fixture("pair_edges_cs_" + mode, contigs, cn, synth.cs_from_letters(m1, 1, p_col=0), synth.cs_from_letters(m2, 2, p_col=0), names, mode, PE_INS,
                            PE_CS_OPTION_SETS, cs=True)
    # the pair heap: 60 opp-in pairs inside a tandem repeat of 12 copies of a 150-base unit; every copy of mate 1 pairs with every copy of mate 2 within -I 0,2000, far
    # more window pairs than the 30 slots of the heap of readpair_get_vector_hits.  3 % substitutions per copy give distinct keys, 0 % all ties.
    for name, div in (("pair_heap_tandem", 0.03), ("pair_heap_ties", 0.0)):
        rng = np.random.Generator(np.random.PCG64(1207))
        unit = rng.integers(0, 4, 150, dtype=np.uint8); copies = []
        for _ in range(12):
            u = unit.copy(); k = rng.random(150) < div
            u[k] = (u[k] + rng.integers(1, 4, int(k.sum()))) & 3
            copies.append(u)
        c1 = np.concatenate([rng.integers(0, 4, 3000, dtype=np.uint8), *copies, rng.integers(0, 4, 3000, dtype=np.uint8)]).astype(np.uint8)
        c2 = rng.integers(0, 4, 8000, dtype=np.uint8)
        m1, m2, names = [], [], []
        for i in range(60):
            f = int(rng.integers(150, 321)); p = 3000 + int(rng.integers(0, 1800 - f + 1))
            a, b = pe_mates(c1, c1, p, f, "pm"[i % 2], "opp-in")
            m1.append(a); m2.append(b); names.append(b"h%d_%s_%d" % (i, b"pm"[i % 2:i % 2 + 1], f))
        _write_pair_fixture(name, [c1, c2], cn, np.stack(m1), np.stack(m2), names, "opp-in", (0, 2000), PH_OPTION_SETS)


# Many and short contigs (tests/test_many_contigs.py).  One i.i.d. sequence S cut into consecutive contigs: global coordinates are those of the uncut S, only the contig
# table differs.  These fixtures store S and the contig lengths, not one array per contig: <name>.npz holds S, contig_len, the reads (or mates1 / mates2, names, mode,
# ins) and, per read, what it was placed on (kind) and where in S (pos).
CT_SPANS = (14, 19)                                     # the smallest and the largest span of the default seeds
CT_KINDS = ("random", "first", "last", "fill", "inside", "border", "over")
CT_FAR = (1, CT_SPANS[0] - 1, 20, 30)                   # bases on the far side of a border
CT_NAMED = (0, 63, 64, 65, 255, 256, 32767, 32768, 65534, 65535)
# (-U: the reference refuses it without --local, "cannot use global (or bfast) and ungapped mode at the same time", gmapper.c:2331)
CT_OPTION_SETS = {None: [], "local": ["--local"], "n1": ["-n", "1"], "ungapped": ["--local", "-U"], "extra": ["--extra-sam-fields"]}


def ct_window(L): return L * 140 // 100                 # the default window: 140 % of the read


def ct_classes(L):
    """the short contigs' lengths for reads of L"""
    W = ct_window(L)
    return [1, 5, CT_SPANS[0] - 1, CT_SPANS[0], CT_SPANS[1], L - 1, L, L + 1, W - 1, W, W + 1]


def ct_layout(rng, L, n_long=85, n_short=215):
    """contig lengths: every long contig (300 to 2 000 bases) with one to a few short ones behind it, each class of ct_classes at least five times"""
    cls = ct_classes(L)
    shorts = [cls[i % len(cls)] for i in range(n_short)]; rng.shuffle(shorts)
    longs = [int(rng.integers(300, 500)) for _ in range(n_long - 15)] + [int(rng.integers(500, 2001)) for _ in range(15)]; rng.shuffle(longs)
    k = 1 + rng.multinomial(n_short - n_long, [1.0 / n_long] * n_long)
    lens, it = [], iter(shorts)
    for l, kk in zip(longs, k): lens.append(l); lens += [next(it) for _ in range(kk)]
    lens = np.array(lens, dtype=np.uint32)
    for c in cls: assert int((lens == c).sum()) >= 5, c
    assert any(lens[i] >= 300 and lens[i + 1] < L for i in range(len(lens) - 1))
    return lens


def ct_offsets(lens): return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))])


def ct_contigs(S, lens): return np.split(S, ct_offsets(lens)[1:-1])


def ct_places(rng, lens, L, n_reads):
    """(kind, position in S) of the reads: the placements the issue lists, then reads anywhere"""
    off = ct_offsets(lens); n = len(lens); W = ct_window(L); total = int(off[-1])
    longs = [c for c in range(1, n - 1) if lens[c] >= 300]
    out = []
    for c in rng.permutation(longs)[:60]: out.append(("first", off[c]))
    for c in rng.permutation(longs)[:60]: out.append(("last", off[c + 1] - L))
    for c in np.nonzero(lens == L)[0]: out += [("fill", off[c])] * 2
    for c in np.nonzero((lens > L) & (lens < W))[0]: out.append(("inside", off[c] + int(rng.integers(0, lens[c] - L + 1))))
    for k in CT_FAR:
        right = [c for c in range(n - 1) if lens[c] >= 300 and lens[c + 1] >= k]          # the far side is contig c + 1
        left = [c for c in range(n - 1) if lens[c + 1] >= 300 and lens[c] >= k]           # ... contig c
        for c in rng.permutation(right)[:20]: out.append(("border", off[c + 1] - (L - k)))
        for c in rng.permutation(left)[:20]: out.append(("border", off[c + 1] - k))
    over = [c for c in range(1, n - 1) if lens[c] <= CT_SPANS[1]]
    for c in rng.permutation(over)[:80]: out.append(("over", off[c] - (L - int(lens[c])) // 2))
    while len(out) < n_reads: out.append(("random", int(rng.integers(0, total - L - 2))))
    ends = [("random", int(off[c]) + int(rng.integers(0, int(lens[c]) - L - 1))) for c in (0, n - 1) if lens[c] >= L + 2 for _ in range(6)]      # the first and the last contig
    out = ends + [out[i] for i in rng.permutation(len(out))][:n_reads - len(ends)]
    out = [(k, min(max(int(p), 0), total - L)) for k, p in out]
    return [out[i] for i in rng.permutation(len(out))]


def ct_draw_reads(rng, S, places, L, p_sub=0.02):
    """reads of L bases at the places: a fifth exact, the others with 2 % substitutions, one in ten of the reads placed freely or on a contig's end with a 1-base indel;
    half of them reverse-complemented"""
    reads = np.empty((len(places), L), dtype=np.uint8)
    for i, (kind, p) in enumerate(places):
        src = S[p:p + L + 2].copy()
        if kind in ("random", "first", "last") and rng.random() < 0.1:
            at = int(rng.integers(15, L - 15))
            src = np.delete(src, at) if rng.random() < 0.5 else np.insert(src, at, int(rng.integers(0, 4)))
        r = src[:L].copy()
        if rng.random() >= 0.2:
            m = rng.random(L) < p_sub
            r[m] = (r[m] + rng.integers(1, 4, int(m.sum()))) & 3
        if rng.random() < 0.5: r = _rc(r)
        reads[i] = r
    return reads


def ct_spans(lens, p, L):
    """the contigs the L bases at p of S lie on: first and last index"""
    off = ct_offsets(lens)
    return int(np.searchsorted(off, p, side="right") - 1), int(np.searchsorted(off, p + L - 1, side="right") - 1)


def _ct_body(exe, lens, S, write_reads, extra, suffix=".fa"):
    """the reference's SAM (no @PG / @RG line) on S cut into contigs of lens"""
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r" + suffix)
        write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(lens))], ct_contigs(S, lens))
        write_reads(r)
        p = subprocess.run([os.path.join(ROOT, "oracle", "_ref", exe), "-N", "4", *extra, r, g], capture_output=True)
        if p.returncode != 0: print(p.stderr.decode()[-2000:]); raise SystemExit(1)
    return b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG") and not l.startswith(b"@RG"))


def _ct_write(name, tag, body):
    path = os.path.join(OUT, name + ("@" + tag if tag else "") + ".sam.gz")
    with gzip.open(path, "wb", compresslevel=9) as f: f.write(body)
    assert os.path.getsize(path) <= 734_000, (path, os.path.getsize(path))


def ct_records(body):
    """mapped records of a SAM text: (name, flag, contig index, 0-based position)"""
    out = []
    for l in body.split(b"\n"):
        if not l or l.startswith(b"@"): continue
        t = l.split(b"\t")
        if not int(t[1]) & 4: out.append((t[0], int(t[1]), int(t[2][len(b"contig"):]) - 1, int(t[3]) - 1))
    return out


def ct_split_conditions(lens, L, kinds, pos, default_body, local_body):
    """the conditions of split_60bp / split_cs_50col (the generator asserts them, tests/test_many_contigs.py asserts them again from the committed files).  A record on a
    contig shorter than the window has a clipped window (w_len = the contig's length)."""
    W = ct_window(L)
    recs = ct_records(default_body)
    clipped = sum(1 for _, _, cn, _ in recs if lens[cn] < W)
    mapped = {int(n[1:]) for n, _, _, _ in recs}
    spanning = [i for i in range(len(kinds)) if CT_KINDS[kinds[i]] in ("border", "over")]
    for i in spanning: a, b = ct_spans(lens, int(pos[i]), L); assert b > a, i
    span_mapped = sum(1 for i in spanning if i in mapped)
    short_local = sum(1 for _, _, cn, _ in ct_records(local_body) if lens[cn] < L)
    return dict(clipped=clipped, spanning_mapped=span_mapped, spanning_unmapped=len(spanning) - span_mapped, short_local=short_local)


def ct_split_case(name, S, lens, L, n_reads, rng, cs=False, option_sets=CT_OPTION_SETS):
    places = ct_places(rng, lens, L, n_reads)
    letters = ct_draw_reads(rng, S, places, L)
    reads = synth.cs_from_letters(letters, 41, p_col=0.02) if cs else letters
    exe = "gmapper-cs" if cs else "gmapper-ls"
    wr = (lambda r: synth.write_csfasta_reads(r, reads)) if cs else (lambda r: write_fa_codes(r, [b"r%d" % i for i in range(len(reads))], list(reads)))
    bodies = {}
    for tag, extra in option_sets.items():
        bodies[tag] = _ct_body(exe, lens, S, wr, extra, ".csfasta" if cs else ".fa")
        _ct_write(name, tag, bodies[tag])
        print("%s%s: %d reads -> %d mapped records" % (name, "@" + tag if tag else "", len(reads), len(ct_records(bodies[tag]))))
    kinds = np.array([CT_KINDS.index(k) for k, _ in places], dtype=np.uint8); pos = np.array([p for _, p in places], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), S=S, contig_len=np.asarray(lens, dtype=np.uint32), reads=reads, kind=kinds, pos=pos)
    return kinds, pos, bodies


def ct_cut(rng, total, n, shorts):
    """total bases cut into exactly n contigs: the short lengths given, the rest at random"""
    rest = total - sum(shorts); m = n - len(shorts)
    cuts = np.sort(rng.choice(np.arange(200, rest - 200), m - 1, replace=False))
    longs = np.diff(np.concatenate([[0], cuts, [rest]]))
    lens = [int(x) for x in longs]
    for s in shorts: lens.insert(int(rng.integers(1, len(lens))), s)
    assert len(lens) == n and sum(lens) == total
    return np.array(lens, dtype=np.uint32)


def ct_mates(S, p, f, strand, L=60):
    """opp-in mates of L bases from the fragment [p, p + f) of S; strand "m": the fragment's reverse complement was sequenced"""
    a, b = S[p:p + L].astype(np.uint8), _rc(S[p + f - L:p + f]).astype(np.uint8)
    return (a, b) if strand == "p" else (b, a)


def ct_pairs_case(rng):
    """split_pairs_2x60: opp-in mates of 60 bases from fragments of 125 to 260 bases under -I 100,300 (pair_edges: the reference pairs such fragments well inside these
    bounds).  adj: the mates on two adjacent contigs; one: on either side of a 1-base contig; in: both inside one contig of 130 to 250 bases; ctl: both inside a long one"""
    L = 60; ins = (100, 300); lens = []
    for u in range(70):
        lens.append(int(rng.integers(300, 600)))
        if u % 3 == 0: lens.append(1)
        elif u % 3 == 1: lens.append(int(rng.integers(130, 251)))
    lens.append(int(rng.integers(300, 600)))
    lens = np.array(lens, dtype=np.uint32); off = ct_offsets(lens); n = len(lens)
    S = rng.integers(0, 4, int(off[-1]), dtype=np.uint8)
    frags = []                                                          # (name, p, f)
    adj = [c for c in range(n - 1) if lens[c] >= L and lens[c + 1] >= L]
    for i in range(90):
        c = adj[i % len(adj)]; b = int(off[c + 1])
        while True:
            f = int(rng.integers(140, 261)); d = int(rng.integers(L, f - L + 1))
            if d <= lens[c] and f - d <= lens[c + 1]: break
        frags.append((b"adj_%d" % i, b - d, f))
    ones = [c for c in range(1, n - 1) if lens[c] == 1]
    for i in range(46):
        c = ones[i % len(ones)]; f = int(rng.integers(140, 261)); d = int(rng.integers(L, f - L))
        frags.append((b"one_%d" % i, int(off[c]) - d, f))
    mids = [c for c in range(n) if 130 <= lens[c] <= 250]
    for i in range(46):
        c = mids[i % len(mids)]; f = int(rng.integers(125, int(lens[c]) + 1))
        frags.append((b"in_%d" % i, int(off[c]) + int(rng.integers(0, int(lens[c]) - f + 1)), f))
    longs = [c for c in range(n) if lens[c] >= 300]
    for i in range(60):
        c = longs[i % len(longs)]; f = int(rng.integers(140, 261))
        frags.append((b"ctl_%d" % i, int(off[c]) + int(rng.integers(0, int(lens[c]) - f + 1)), f))
    frags = [frags[i] for i in rng.permutation(len(frags))]
    m1, m2 = [], []
    for k, (nm, p, f) in enumerate(frags):
        a, b = ct_mates(S, p, f, "pm"[k % 2], L)
        a, b = a.copy(), b.copy()
        for x in (a, b):
            m = rng.random(L) < 0.01; x[m] = (x[m] + rng.integers(1, 4, int(m.sum()))) & 3
        m1.append(a); m2.append(b)
    return lens, S, np.stack(m1), np.stack(m2), [nm for nm, _, _ in frags], np.array([p for _, p, _ in frags], dtype=np.int64), np.array([f for _, _, f in frags], dtype=np.int64), ins


def ct_pair_bodies(lens, S, m1, m2, names, ins, option_sets):
    L = m1.shape[1]
    def wr(r):
        n1 = [n + b"/1" for n in names]; n2 = [n + b"/2" for n in names]
        write_fa_codes(r, [n for pair in zip(n1, n2) for n in pair], [q for pair in zip(list(m1), list(m2)) for q in pair])
    return {tag: _ct_body("gmapper-ls", lens, S, wr, ["-p", "opp-in", "-I", "%d,%d" % ins, *extra]) for tag, extra in option_sets.items()}


def ct_65536_inputs(rng):
    """65 536 contigs: fillers of 12 to 24 bases, targets of 80 to 200 at the ten named indices and at 25 pairs (b, b + 32 768) -- for every target c outside the named
    ones, c & 0x7FFF and c ^ 0x8000 are targets too, each with its own sequence"""
    N = 65536
    base = sorted(int(x) for x in rng.choice(np.arange(300, 32700), 25, replace=False))
    others = sorted(base + [b + 32768 for b in base])
    for c in others: assert (c & 0x7FFF) in others and (c ^ 0x8000) in others
    lens = rng.integers(12, 25, N).astype(np.uint32)
    lens[others] = rng.integers(80, 201, len(others)); lens[list(CT_NAMED)] = rng.integers(140, 201, len(CT_NAMED))
    off = ct_offsets(lens); S = rng.integers(0, 4, int(off[-1]), dtype=np.uint8)
    L = 60
    src = [c for c in CT_NAMED for _ in range(10)]
    high = [c for c in others if c >= 32768]; low = [c for c in others if c < 32768]
    src += [high[i % len(high)] for i in range(180)] + [low[i % len(low)] for i in range(120)]
    src = [src[i] for i in rng.permutation(len(src))]
    places = [("random", int(off[c]) + int(rng.integers(0, int(lens[c]) - L + 1))) for c in src]
    reads = ct_draw_reads(rng, S, [("fill", p) for _, p in places], L)                      # (no indels: a target may be no longer than the read + 20)
    wide = [c for c in list(CT_NAMED) + others if lens[c] >= 130]
    m1, m2, pt = [], [], []
    for k in range(100):
        c = wide[int(rng.integers(0, len(wide)))]; f = int(rng.integers(125, int(lens[c]) + 1)); p = int(off[c]) + int(rng.integers(0, int(lens[c]) - f + 1))
        a, b = ct_mates(S, p, f, "pm"[k % 2], L); m1.append(a); m2.append(b); pt.append(c)
    return lens, S, reads, np.array(src, dtype=np.int64), np.stack(m1), np.stack(m2), np.array(pt, dtype=np.int64), (50, 300)


def ct_65536_conditions(body, pair_body):
    recs = ct_records(body) + ct_records(pair_body)
    per = {c: sum(1 for _, _, cn, _ in recs if cn == c) for c in CT_NAMED}
    return per, sum(1 for _, _, cn, _ in recs if cn >= 32768)


def contigs_cases():
    rng = np.random.Generator(np.random.PCG64(6553))
    # split_60bp
    L = 60
    lens = ct_layout(rng, L); S = rng.integers(0, 4, int(lens.sum()), dtype=np.uint8)
    kinds, pos, bodies = ct_split_case("split_60bp", S, lens, L, 600, rng)
    c = ct_split_conditions(lens, L, kinds, pos, bodies[None], bodies["local"]); print("split_60bp:", len(lens), "contigs,", len(S), "bases;", c)
    assert c["clipped"] >= 40 and c["spanning_mapped"] >= 20 and c["spanning_unmapped"] >= 10 and c["short_local"] >= 10, c
    # split_64 / split_65: the same S on either side of the anchor kernel's lane-gather limit
    for n in (64, 65):
        ln = ct_cut(rng, len(S), n, [1, CT_SPANS[0], L, L + 1, ct_window(L) - 1])
        k2, p2, b2 = ct_split_case("split_%d" % n, S, ln, L, 200, rng, option_sets={None: []})
        hi = sum(1 for _, _, cn, _ in ct_records(b2[None]) if cn >= 33); last = sum(1 for _, _, cn, _ in ct_records(b2[None]) if cn == n - 1)
        print("split_%d: %d mapped records on contigs 34 and up, %d on the last" % (n, hi, last))
        assert hi >= 40 and last >= 1
    # split_cs_50col
    L = 50
    lens = ct_layout(rng, L)
    Sc = S[:int(lens.sum())] if int(lens.sum()) <= len(S) else np.concatenate([S, rng.integers(0, 4, int(lens.sum()) - len(S), dtype=np.uint8)])
    kinds, pos, bodies = ct_split_case("split_cs_50col", Sc, lens, L, 600, rng, cs=True, option_sets={None: [], "local": ["--local"]})
    c = ct_split_conditions(lens, L, kinds, pos, bodies[None], bodies["local"]); print("split_cs_50col:", len(lens), "contigs,", len(Sc), "bases;", c)
    assert c["clipped"] >= 40, c
    # split_pairs_2x60
    lens, Sp, m1, m2, names, pos, frag, ins = ct_pairs_case(rng)
    bodies = ct_pair_bodies(lens, Sp, m1, m2, names, ins, {None: [], "nhp": ["--no-half-paired"]})
    for tag, body in bodies.items(): _ct_write("split_pairs_2x60", tag, body)
    proper = _paired_names(bodies[None])
    adj_not = sum(1 for nm in names if nm.startswith(b"adj_") and nm + b"/1" not in proper and nm not in proper)
    ctl = [nm for nm in names if nm.startswith(b"ctl_")]; ctl_ok = sum(1 for nm in ctl if nm in proper or nm + b"/1" in proper)
    print("split_pairs_2x60: %d contigs, %d pairs, %d proper; %d adjacent-contig pairs not proper; %d of %d controls proper" % (len(lens), len(names), len(proper), adj_not, ctl_ok, len(ctl)))
    assert adj_not >= 30 and 10 * ctl_ok >= 8 * len(ctl)
    np.savez_compressed(os.path.join(OUT, "split_pairs_2x60.npz"), S=Sp, contig_len=lens, mates1=m1, mates2=m2, names=np.array(names), pos=pos, frag=frag,
                        mode=np.array("opp-in"), ins=np.array(ins))
    # contigs_65536: the SAM bodies only (the header is 65 536 @SQ lines the tests build themselves)
    lens, S6, reads, src, m1, m2, pt, ins = ct_65536_inputs(rng)
    strip = lambda body: b"".join(l + b"\n" for l in body.split(b"\n") if l and not l.startswith(b"@"))
    body = strip(_ct_body("gmapper-ls", lens, S6, lambda r: write_fa_codes(r, [b"r%d" % i for i in range(len(reads))], list(reads)), []))
    names = [b"p%d" % i for i in range(len(m1))]
    pbody = strip(ct_pair_bodies(lens, S6, m1, m2, names, ins, {None: []})[None])
    _ct_write("contigs_65536", None, body); _ct_write("contigs_65536", "pairs", pbody)
    per, high = ct_65536_conditions(body, pbody)
    print("contigs_65536: %d bases; mapped records per named index %s; %d on indices of 32 768 or more" % (len(S6), per, high))
    assert min(per.values()) >= 5 and high >= 150
    np.savez_compressed(os.path.join(OUT, "contigs_65536.npz"), S=S6, contig_len=lens, reads=reads, target=src, mates1=m1, mates2=m2, names=np.array(names),
                        pair_target=pt, mode=np.array("opp-in"), ins=np.array(ins))
    for f in ("split_60bp", "split_64", "split_65", "split_cs_50col", "split_pairs_2x60", "contigs_65536"):
        assert os.path.getsize(os.path.join(OUT, f + ".npz")) <= 734_000, f


def _geometry_ref_body(base, n, extra):
    """the reference's records (no header line) on the first n reads / pairs of a committed input under the options `extra`"""
    from tests import oracle_api as oa
    kind = oa.geometry_kind(base)
    z = np.load(os.path.join(OUT, base + ".npz"))
    contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    with tempfile.TemporaryDirectory() as d:
        g = os.path.join(d, "g.fa"); r = os.path.join(d, "r.csfasta" if kind == "cs" else "r.fa")
        if kind == "pairs":
            write_fa_codes(g, [bytes(x) for x in z["contig_names"]], contigs)
            names = [bytes(x) for pair in zip(z["names1"][:n], z["names2"][:n]) for x in pair]
            write_fa_codes(r, names, [q for pair in zip(list(z["mates1"][:n]), list(z["mates2"][:n])) for q in pair])
            extra = ["-p", str(z["mode"]), "-I", "%d,%d" % tuple(int(x) for x in z["ins"]), *extra]
        else:
            write_fa_codes(g, [b"contig%d" % (i + 1) for i in range(len(contigs))], contigs)
            if kind == "cs": synth.write_csfasta_reads(r, z["reads"][:n])
            else: write_fa_codes(r, [b"r%d" % i for i in range(n)], list(z["reads"][:n]))
        if base in oa.GEOMETRY_UNAL: extra = [*extra, "--sam-unaligned"]
        cmd = ["timeout", "-k", "5", "300", os.path.join(ROOT, "oracle", "_ref", "gmapper-cs" if kind == "cs" else "gmapper-ls"), "-N", "4", *extra, r, g]
        p = subprocess.run(cmd, capture_output=True)
        assert p.returncode == 0, (base, extra, p.returncode, p.stderr[-2000:])
    return b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@"))


def geometry_cases():
    """--geometry-only: the option sets of tests/oracle_api.py GEOMETRY_CASES through the reference on committed inputs.  Only the records are stored.  Prints, and asserts,
    how far each golden lies from its input's default golden, and the -a -1 and -a 99 goldens from the -a 0 one (records of the one that are not in the other)."""
    from tests import oracle_api as oa
    total = 0; bodies = {}
    for base, n in list(oa.GEOMETRY_READS.items()) + [(t.split(":")[0], n) for t, n in oa.GEOMETRY_READS_OF.items()]:
        want = oa.geometry_default_records(base, n)
        assert _geometry_ref_body(base, n, []) == want, "%s: the default golden's records of the first %d reads are not the reference's output on them" % (base, n)
    for tag, (base, extra, _, _) in oa.GEOMETRY_CASES.items():
        body = _geometry_ref_body(base, oa.geometry_reads(tag), extra)
        path = os.path.join(OUT, oa.geometry_file(tag)); _gz_fixed(path, body); bodies[tag] = body
        size = os.path.getsize(path); total += size
        recs = body.count(b"\n"); mapped = sum(1 for l in body.split(b"\n") if l and not int(l.split(b"\t", 2)[1]) & 4)
        dist = oa.sam_distance(body, oa.geometry_default_records(base, oa.geometry_reads(tag)))
        print("%-36s %-28s %5d records, %5d mapped, %5d not in the default golden, %6d bytes" % (tag, " ".join(extra), recs, mapped, dist, size))
        assert dist >= oa.GEOMETRY_MIN_DISTANCE or (tag in oa.GEOMETRY_SAME_AS_DEFAULT and dist == 0), (tag, dist)
        assert size <= 130_000, (tag, size)
    for tag, body in bodies.items():
        base, what = tag.split(":")
        if what in ("a-1", "a99"):
            dist = oa.sam_distance(body, bodies[base + ":a0"])
            print("%-36s %5d records not in %s:a0" % (tag, dist, base))
            assert dist >= oa.GEOMETRY_MIN_DISTANCE, (tag, dist)
    print("geometry goldens: %d files, %d bytes" % (len(bodies), total))


def anchor_kat_cases():
    """--anchor-kat-only: the known answers of sw_full_ls / sw_full_cs at the anchor widths -1, 0, 1, 9 and 99 (oracle/ref_kat.cpp, ref_kat_cs.cpp, mode "anchors")"""
    for exe, name, n in (("ref_kat", "sw_kat_anchors", 90), ("ref_kat_cs", "sw_kat_cs_anchors", 120)):
        kat = subprocess.run([os.path.join(ROOT, "oracle", "_ref", exe), str(n), "anchors"], capture_output=True, check=True).stdout
        path = os.path.join(OUT, name + ".txt.gz"); _gz_fixed(path, kat)
        assert os.path.getsize(path) < 400_000, "cut cases per width, not widths"
        per = {}
        for l in kat.split(b"\n"):
            if not l: continue
            if l[:1] == b"P": cur = l.split()[1].decode(); per[cur] = {}
            else: per[cur][l[:1].decode()] = per[cur].get(l[:1].decode(), 0) + 1
        print("%s: %d bytes;" % (name, os.path.getsize(path)), "; ".join("%s: %s" % (k, ", ".join("%d %s" % (c, t) for t, c in sorted(v.items()))) for k, v in per.items()))


# Reads of 128 to 1 000 bases and colours (tests/oracle_api.py LONG_INPUTS / LONG_CASES, tests/test_long_reads.py)
def long_stress_genome(seed=2025):
    """Two contigs of about 150 kbp together, for long reads.  Contig 1: 20 kbp, then the repeat part -- eight copies of a 1 500-base family at 2 % divergence with spacers
    of 300 to 2 000 bases between them, six copies in tandem of a 700-base unit at 1.4 % -- then 15 kbp, a 9-mer in tandem x 300, 10 kbp, a run of 200 N, 20 kbp.
    Contig 2: 25 kbp, a reverse-complement copy of the family, 8 kbp, a forward copy, 22 kbp.  Returns (contigs, (lo, hi): the repeat part of contig 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    def rnd(n): return rng.integers(0, 4, size=n, dtype=np.uint8)
    def copy_of(x, div):
        y = x.copy(); k = rng.random(len(x)) < div
        y[k] = (y[k] + rng.integers(1, 4, int(k.sum()))) & 3
        return y.astype(np.uint8)
    fam = rnd(1500); unit = rnd(700)
    c1 = [rnd(20000)]; lo = 20000
    for _ in range(8): c1 += [copy_of(fam, 0.02), rnd(int(rng.integers(300, 2001)))]
    c1 += [copy_of(unit, 0.014) for _ in range(6)] + [rnd(500)]
    hi = sum(len(x) for x in c1)
    c1 += [rnd(15000), np.tile(np.array([0, 1, 2, 3, 3, 2, 1, 0, 2], dtype=np.uint8), 300), rnd(10000), np.full(200, 15, dtype=np.uint8), rnd(20000)]
    c2 = [rnd(25000), synth.COMPLEMENT[copy_of(fam, 0.02)[::-1]], rnd(8000), copy_of(fam, 0.02), rnd(22000)]
    return [np.concatenate(c1).astype(np.uint8), np.concatenate(c2).astype(np.uint8)], (lo, hi)


def _long_mutate(src, L, rng, p_sub=0.03, p_ins=0.004, p_del=0.004):
    """synth.make_reads' walk along source rows of at least L + 16 bases: substitutions, insertions and deletions per base"""
    n, margin = src.shape; out = np.empty((n, L), dtype=np.uint8); ptr = np.zeros(n, dtype=np.int64); rows = np.arange(n)
    for j in range(L):
        r = rng.random(n); ins = r < p_ins; dele = (~ins) & (r < p_ins + p_del)
        ptr = np.minimum(ptr + dele, margin - 1)
        b = src[rows, ptr]
        sub = (~ins) & (rng.random(n) < p_sub)
        b = np.where(sub & (b < 4), (b + rng.integers(1, 4, size=n, dtype=np.uint8)) & 3, b)
        b = np.where(ins, rng.integers(0, 4, size=n, dtype=np.uint8), b)
        out[:, j] = b
        ptr = np.minimum(ptr + (~ins), margin - 1)
    return out


def long_reads(contigs, rep, inp):
    """the reads of an unpaired input: every second one from the repeat part.  Letter space: 3 % substitutions, 0.4 % insertions and deletions; colour space: an indel of one to
    three bases a read, 3 % colour errors, 0.4 % skipped cycles.  clean: no N in a read (the reference does not return from --extra-sam-fields on one)"""
    part = [contigs[0][rep[0]:rep[1]]]; n = inp["n"]; L = inp["len"]; k = n // 2
    if inp["kind"] == "cs":
        a = synth.make_cs_reads(part, k, L, inp["seed"], p_col=0.03, p_dot=0.004)[0]; b = synth.make_cs_reads(contigs, n - k, L, inp["seed"] + 50, p_col=0.03, p_dot=0.004)[0]
    else:
        a = synth.make_reads(part, k, L, inp["seed"], p_sub=0.03, p_ins=0.004, p_del=0.004)[0]; b = synth.make_reads(contigs, n - k, L, inp["seed"] + 50, p_sub=0.03, p_ins=0.004, p_del=0.004)[0]
    reads = np.empty((n, a.shape[1]), dtype=np.uint8)
    reads[0:2 * k:2] = a; reads[1:2 * k:2] = b[:k]; reads[2 * k:] = b[k:]
    if inp.get("clean"):
        rng = np.random.Generator(np.random.PCG64(inp["seed"] + 99)); bad = reads > 3
        reads = np.where(bad, rng.integers(0, 4, size=reads.shape, dtype=np.uint8), reads).astype(np.uint8)
    return reads


def long_pairs(contigs, rep, inp):
    """the mates of a paired input (letter codes): fragments whose insert size, as the pair mode measures it, is drawn about the middle of -I (every twentieth pair: 1 000
    beyond its upper bound, so that its mates map on their own), the share inp["share"] of the fragments from the repeat part, from either strand; each mate walks its end of the fragment
    with 3 % substitutions and 0.4 % insertions and deletions, then the pair mode turns the mates (as pe_mates)"""
    rng = np.random.Generator(np.random.PCG64(inp["seed"])); n = inp["n"]; L1, L2 = inp["len"]; lo, hi = inp["ins"]; mode = inp["mode"]
    shift = {"opp-in": 0, "opp-out": L1 + L2, "col-fw": L2, "col-bw": L1}[mode]
    A = np.empty((n, L1 + 16), dtype=np.uint8); B = np.empty((n, L2 + 16), dtype=np.uint8)
    for i in range(n):
        f = int(np.rint(rng.normal((lo + hi) / 2 + shift, (hi - lo) / 16)))
        if i % 20 == 19: f = hi + shift + 1000
        f = max(f, max(L1, L2) + 16)
        if int((i + 1) * inp["share"]) > int(i * inp["share"]): c = contigs[0]; p = int(rng.integers(rep[0], rep[1] - f))
        else: c = contigs[int(rng.integers(0, 2))]; p = int(rng.integers(0, len(c) - f))
        frag = c[p:p + f]
        if rng.random() < 0.5: frag = _rc(frag)
        frag = np.where(frag > 3, rng.integers(0, 4, size=len(frag), dtype=np.uint8), frag).astype(np.uint8)
        A[i] = frag[:L1 + 16]; B[i] = _rc(frag)[:L2 + 16]
    a = _long_mutate(A, L1, rng); b = _long_mutate(B, L2, rng)
    if mode == "opp-out": a, b = synth.COMPLEMENT[a[:, ::-1]], synth.COMPLEMENT[b[:, ::-1]]
    elif mode == "col-fw": b = synth.COMPLEMENT[b[:, ::-1]]
    elif mode == "col-bw": a = synth.COMPLEMENT[a[:, ::-1]]
    return np.ascontiguousarray(a, dtype=np.uint8), np.ascontiguousarray(b, dtype=np.uint8)


def _long_ref_body(d, cs, args, limit=300, rfile=None):
    """the reference on d/g.fa and d/r.*, under a time limit: its SAM text without the @PG / @RG lines"""
    exe = os.path.join(ROOT, "oracle", "_ref", "gmapper-cs" if cs else "gmapper-ls")
    p = subprocess.run(["timeout", "-k", "5", str(limit), exe, "-N", "4", "--sam-unaligned", *args, os.path.join(d, rfile or ("r.csfasta" if cs else "r.fa")), os.path.join(d, "g.fa")], capture_output=True)
    assert p.returncode == 0, (args, p.returncode, p.stderr[-2000:])
    return b"".join(l + b"\n" for l in p.stdout.split(b"\n") if l and not l.startswith(b"@PG") and not l.startswith(b"@RG"))


def long_cases():
    """--long-only: long_genome.npz, the inputs of LONG_INPUTS and the reference's bodies of LONG_CASES.  Prints every fixture's counts and asserts LONG_MIN on them."""
    from tests import oracle_api as oa
    contigs, rep = long_stress_genome(); cn = [b"contig1", b"contig2"]
    _npz_fixed(os.path.join(OUT, "long_genome.npz"), contig0=contigs[0], contig1=contigs[1], repeat=np.array(rep))
    print("long_genome: contigs of %d and %d bases, repeat part [%d, %d) of contig1, %d bytes" % (len(contigs[0]), len(contigs[1]), rep[0], rep[1], os.path.getsize(os.path.join(OUT, "long_genome.npz"))))
    total = 0; missed = []
    for name, inp in oa.LONG_INPUTS.items():
        cs = inp["kind"].startswith("cs"); pairs = inp["kind"].endswith("pairs")
        with tempfile.TemporaryDirectory() as d:
            write_fa_codes(os.path.join(d, "g.fa"), cn, contigs)
            if pairs:
                m1, m2 = long_pairs(contigs, rep, inp)
                if cs: m1 = synth.cs_from_letters(m1, inp["seed"] + 1, p_col=0.03); m2 = synth.cs_from_letters(m2, inp["seed"] + 2, p_col=0.03)
                n1 = [b"p%d/1" % i for i in range(inp["n"])]; n2 = [b"p%d/2" % i for i in range(inp["n"])]
                names = [x for pair in zip(n1, n2) for x in pair]; rows = [x for pair in zip(list(m1), list(m2)) for x in pair]
                if cs:
                    with open(os.path.join(d, "r.csfasta"), "wb") as f:
                        for nm, row in zip(names, rows): f.write(b">" + nm + b"\n" + b"ACGT"[row[0]:row[0] + 1] + bytes(b"0123"[c] if c < 4 else ord(".") for c in row[1:]) + b"\n")
                else: write_fa_codes(os.path.join(d, "r.fa"), names, rows)
                _npz_fixed(os.path.join(OUT, "long_%s.npz" % name), genome=np.array("long_genome"), mates1=m1, mates2=m2, names1=np.array(n1), names2=np.array(n2), mode=np.array(inp["mode"]), ins=np.array(inp["ins"]))
                more = ["-p", inp["mode"], "-I", "%d,%d" % inp["ins"]]
            else:
                reads = long_reads(contigs, rep, inp)
                if inp.get("fq"):                                       # FASTQ / csfastq input, PHRED+33: a quality of 2 to 40 a base or colour
                    q = (np.random.default_rng(inp["seed"] + 7).integers(2, 41, size=(len(reads), inp["len"])) + 33).astype(np.uint8)
                    T = np.frombuffer(b"ACGTUMRWSYKVHDBN", dtype=np.uint8); tab = np.full(16, ord("."), dtype=np.uint8); tab[:4] = np.frombuffer(b"0123", dtype=np.uint8)
                    with open(os.path.join(d, "r.csfastq" if cs else "r.fq"), "wb") as f:
                        for i in range(len(reads)):
                            seq = b"ACGT"[reads[i, 0]:reads[i, 0] + 1] + tab[reads[i, 1:]].tobytes() if cs else T[reads[i]].tobytes()
                            f.write(b"@r%d\n" % i + seq + b"\n+\n" + q[i].tobytes() + b"\n")
                    _npz_fixed(os.path.join(OUT, "long_%s.npz" % name), genome=np.array("long_genome"), reads=reads, quals=q, qual_delta=np.array(33))
                else:
                    if cs: synth.write_csfasta_reads(os.path.join(d, "r.csfasta"), reads)
                    else: write_fa_codes(os.path.join(d, "r.fa"), [b"r%d" % i for i in range(len(reads))], list(reads))
                    _npz_fixed(os.path.join(OUT, "long_%s.npz" % name), genome=np.array("long_genome"), reads=reads)
                more = []
            for st in inp["sets"]:
                tag = "%s:%s" % (name, st)
                body = _long_ref_body(d, cs, more + oa.LONG_CASES[tag][1], rfile=("r.csfastq" if cs else "r.fq") if inp.get("fq") else None)
                path = os.path.join(OUT, oa.long_file(tag)); _gz_fixed(path, body)
                c = oa.long_counts(body, inp["n"], pairs); bad = oa.long_conditions(tag, c); size = os.path.getsize(path); total += size
                print("%-32s %s, %d bytes%s" % (tag, ", ".join("%s %d" % kv for kv in c.items()), size, "  MISSES " + ",".join(bad) if bad else ""))
                if bad: missed.append((tag, bad))
                assert size <= 200_000, (tag, size)
    print("long goldens: %d cases, %d bytes" % (len(oa.LONG_CASES), total))
    assert not missed, missed


if __name__ == "__main__":
    if "--long-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); long_cases()
    elif "--geometry-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); geometry_cases()
    elif "--anchor-kat-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); anchor_kat_cases()
    elif "--seeds-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); seeds_cases()
    elif "--contigs-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); contigs_cases()
    elif "--pair-edges-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); pair_edges_cases()
    elif "--pair-file-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); pair_file_cases()
    elif "--cs-pairs-fq-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); cs_paired_fastq_cases()
    elif "--format-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); format_cases()
    elif "--file-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); file_cases()
    elif "--rna-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); rna_cases()
    elif "--preprocess-only" in sys.argv:
        os.makedirs(OUT, exist_ok=True); preprocess_cases()
    else:
        main()
