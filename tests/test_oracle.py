"""The CPU restatement (oracle/) against the reference's own outputs (tests/golden/*, generated
by tools/make_golden.py from the reference binary built from /root/reference)."""
import ctypes as C
import os
import numpy as np
import pytest
from tests import oracle_api as oa

GOLDEN = ["cfg1_36bp_1Mbp", "cfg2s_100bp_2Mbp", "stress_60bp", "stress_100bp_unal"]


@pytest.mark.parametrize("name", GOLDEN)
def test_oracle_sam_matches_reference(name, oracle_lib):
    contigs, reads, sam = oa.load_golden(name)
    s = oa.Session(contigs)
    s.set(hash_filter_calls=True, sam_unaligned=name.endswith("_unal"))
    got = oa.sam_header(contigs) + s.map_sam(reads, nthreads=4)
    s.close()
    assert got == sam, "oracle SAM differs from reference SAM for %s" % name


def test_oracle_sw_known_answers(oracle_lib):
    L = oracle_lib
    u32p = C.POINTER(C.c_uint32)
    nv = nf = 0
    db = C.create_string_buffer(4096); qr = C.create_string_buffer(4096)
    for rec in oa.load_kat():
        if rec[0] == "V":
            _, goff, glen, rlen, g, r, score = rec
            assert L.gmo_sw_vector(g.ctypes.data_as(u32p), goff, glen, r.ctypes.data_as(u32p), rlen) == score
            nv += 1
        else:
            _, goff, glen, rlen, ax, ay, alen, aw, rv, g, r, exp, edb, eqr = rec
            out = (C.c_int * 9)()
            assert L.gmo_sw_full_ls(g.ctypes.data_as(u32p), goff, glen, r.ctypes.data_as(u32p), rlen, ax, ay, alen, aw, rv,
                                    out, db, qr, 4096) == 0
            assert list(out) == exp, (goff, glen, rlen, ax, ay, alen, aw, rv)
            assert db.value.decode() == edb and qr.value.decode() == eqr
            nf += 1
    assert nv >= 1000 and nf >= 1000


def test_oracle_sharding_invariance(oracle_lib):
    """reads mapped in two halves and concatenated == mapped at once."""
    contigs, reads, sam = oa.load_golden("stress_60bp")
    s = oa.Session(contigs)
    whole = s.map_sam(reads, nthreads=2)
    h = len(reads) // 2
    # names are positional (r<i>), so only compare record payloads after the name column
    strip = lambda b: [l.split(b"\t", 1)[1] for l in b.split(b"\n") if l]
    halves = strip(s.map_sam(reads[:h], nthreads=1)) + strip(s.map_sam(reads[h:], nthreads=3))
    s.close()
    assert strip(whole) == halves


PAIRED = ["pairfix_opp-in", "pairfix_opp-out", "pairfix_col-fw", "pairfix_col-bw", "cfg5s_2x150_1Mbp", "stress_pairs_2x100"]


@pytest.mark.parametrize("name", PAIRED)
def test_oracle_paired_sam_matches_reference(name, oracle_lib):
    """paired mode (handle_readpair, half-paired rescue, paired MAPQ) incl. the reference's own pairing fixture"""
    g = oa.load_golden_pairs(name)
    s = oa.Session(g["contigs"], g["contig_names"])
    s.set_pairing(g["mode"], *g["ins"])
    got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs_sam(g["m1"], g["m2"], g["names1"], g["names2"], nthreads=4)
    s.close()
    assert got == g["sam"], "oracle paired SAM differs from the reference for %s" % name


def test_oracle_parallel_index_builder_equals_sequential(oracle_lib):
    """the bench's 3 Gbp CPU baseline uses the chunk-parallel builder; it must produce the sequential builder's index
    (N runs, contig boundaries and pieces that start inside a k-mer included)"""
    import numpy as np
    from shrimp_amd import synth
    contigs = synth.make_genome([1_300_000, 400_000, 700, 25], 9)
    contigs[0][1000:1200] = 15; contigs[1][:30] = 15; contigs[0][650_000:650_019] = 15
    s = oa.Session(contigs)
    try:
        for t in (1, 2, 3, 7, 16):
            assert s.index_selfcheck(t), t
    finally:
        s.close()


@pytest.mark.parametrize("tag", sorted(oa.OPTION_CASES))
def test_oracle_option_sets_match_reference(tag, oracle_lib):
    """non-default options (--strata, --max-alignments, -o, scores, thresholds, window geometry, anchor width, custom seeds,
    cutoff; paired --strata) against the reference binary run with the same options"""
    base, opts, _, _ = oa.OPTION_CASES[tag]
    want = oa.load_option_sam(base, tag)
    if base.startswith("stress_pairs") or base.startswith("chimeric_pairs"):
        g = oa.load_golden_pairs(base)
        s = oa.Session(g["contigs"], g["contig_names"], opts=opts)
        s.set_pairing(g["mode"], *g["ins"])
        got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs_sam(g["m1"], g["m2"], g["names1"], g["names2"], nthreads=4)
        n_reads = 2 * len(g["m1"])
    else:
        contigs, reads, _ = oa.load_golden(base)
        s = oa.Session(contigs, opts=opts)
        if "unal" in base: s.set("ungapped" not in opts, True)
        got = oa.sam_header(contigs) + s.map_sam(reads, nthreads=4)
        n_reads = len(reads)
    s.close()
    assert got == want, "oracle SAM differs from the reference for option set %s" % tag
    if tag in oa.SCORE_CASE_TAGS:                                  # a golden of the score sets must not pass by being empty
        share, indels = oa.sam_mapped_share_and_indels(want, n_reads)
        assert share >= 0.5 and indels >= 20, (tag, share, indels)


def test_oracle_mirna_mode_matches_reference(oracle_lib):
    """gmapper -M mirna on 22-base reads: hashed seeds of span 20 with zeros at both ends, -U, -n 1, window 100 %, --local"""
    contigs, reads, want = oa.load_golden("mirna_22bp")
    s = oa.Session(contigs, opts=oa.MIRNA_MODE[0])
    got = oa.sam_header(contigs) + s.map_sam(reads, nthreads=4); s.close()
    assert got == want and got.count(b"\n") > 2400


def test_oracle_n1_on_noisy_reads_matches_reference(oracle_lib):
    """-n 1 where it matters: 70-base reads with 9 % substitutions, 57 of which map only because ONE k-mer match is enough (no region counts, a window per
    anchor, gmapper.c:2610-2625)"""
    contigs, reads, want = oa.load_golden("n1_noisy_70bp")
    s = oa.Session(contigs, opts="cmw-mode=1")
    got = oa.sam_header(contigs) + s.map_sam(reads, nthreads=4)
    s2 = oa.Session(contigs)
    dflt = s2.map_sam(reads, nthreads=4)
    s.close(); s2.close()
    assert got == want
    assert dflt.count(b"\n") < got.count(b"\n") - 50          # the default mode loses them: the case does tell the two apart
    # reads built to have ONE list entry each (a 14-base block intact, substitutions around it): regions marked once must still give anchors
    contigs, reads, want = oa.load_golden("n1_onehit_60bp")
    s = oa.Session(contigs, opts="cmw-mode=1;full-threshold=30;vec-threshold=30")
    got = oa.sam_header(contigs) + s.map_sam(reads, nthreads=4)
    s.close()
    assert got == want and got.count(b"\n") > 380


def test_oracle_colour_space_kernels_match_reference_known_answers(oracle_lib):
    """S1/S2 in colour space: the restated sw_vector (first-colour row) and sw_full_cs (4 layers, crossovers, traceback,
    alignment strings) against the reference's own functions on 700 random cases x 2 tie-break directions"""
    import ctypes as C
    L = oa.load(); u32p = C.POINTER(C.c_uint32)
    nc = ns = 0
    for r in oa.load_kat_cs():
        if r[0] == "C":
            _, goff, glen, rlen, initbp, gcs, gls, rd, score = r
            got = L.gmo_sw_vector_cs(gcs.ctypes.data_as(u32p), goff, glen, rd.ctypes.data_as(u32p), rlen, gls.ctypes.data_as(u32p), initbp)
            assert got == score, (goff, glen, rlen, initbp, got, score); nc += 1
        else:
            _, (goff, glen, rlen, initbp, ax, ay, alen, awidth, rv, thresh), gls, rd, want, db, qr = r
            out = (C.c_int * 10)(); dba = C.create_string_buffer(4096); qra = C.create_string_buffer(4096)
            assert L.gmo_sw_full_cs(gls.ctypes.data_as(u32p), goff, glen, rd.ctypes.data_as(u32p), rlen, initbp, thresh, ax, ay, alen, awidth, rv,
                                    out, dba, qra, 4096) == 0
            if want[0] == 0:
                assert out[0] == 0
            else:
                assert list(out) == want and dba.value == db and qra.value == qr, (list(out), want, dba.value, db, qra.value, qr)
            ns += 1
    assert nc >= 700 and ns >= 1400


def test_oracle_sw_full_cs_local_mode_matches_reference_known_answers(oracle_lib):
    """sw_full_cs(.., local_alignment = true) (ref: sw-full-cs.c:199-203,315,439-552): 400 random cases x 2 tie-break directions from the reference's own function"""
    import ctypes as C
    L = oa.load(); u32p = C.POINTER(C.c_uint32)
    n = 0
    for r in oa.load_kat_cs("sw_kat_cs_local.txt.gz"):
        assert r[0] == "L"
        _, (goff, glen, rlen, initbp, ax, ay, alen, awidth, rv, thresh), gls, rd, want, db, qr = r
        out = (C.c_int * 10)(); dba = C.create_string_buffer(4096); qra = C.create_string_buffer(4096)
        assert L.gmo_sw_full_cs_mode(gls.ctypes.data_as(u32p), goff, glen, rd.ctypes.data_as(u32p), rlen, initbp, thresh, C.c_longlong(ax), C.c_longlong(ay), alen, awidth, rv, 1,
                                     out, dba, qra, 4096) == 0
        if want[0] == 0: assert out[0] == 0
        else: assert list(out) == want and dba.value == db and qra.value == qr, (list(out), want, dba.value, db, qra.value, qr)
        n += 1
    assert n >= 800


def test_oracle_sw_full_cs_crossover_scores_match_reference_known_answers(oracle_lib):
    """sw_full_cs with crossover_score[] (per-position scores from the QVs, ref: sw-full-cs.c:312-322, gmapper.c:532-544): 500 cases x 2 tie-break directions in global
    mode, every other case in local mode too, from the reference's own function (oracle/ref_kat_cs.cpp "xover")"""
    import ctypes as C
    L = oa.load(); u32p = C.POINTER(C.c_uint32)
    n = 0
    for r in oa.load_kat_cs("sw_kat_cs_xover.txt.gz"):
        kind, (goff, glen, rlen, initbp, ax, ay, alen, awidth, rv, thresh), gls, rd, want, db, qr, xs = r
        out = (C.c_int * 10)(); dba = C.create_string_buffer(4096); qra = C.create_string_buffer(4096)
        assert L.gmo_sw_full_cs_xover(gls.ctypes.data_as(u32p), goff, glen, rd.ctypes.data_as(u32p), rlen, initbp, thresh, C.c_longlong(ax), C.c_longlong(ay), alen, awidth, rv,
                                      1 if kind == "Y" else 0, xs.ctypes.data_as(C.POINTER(C.c_int)), out, dba, qra, 4096) == 0
        if want[0] == 0: assert out[0] == 0
        else: assert list(out) == want and dba.value == db and qra.value == qr, (kind, list(out), want, dba.value, db, qra.value, qr)
        n += 1
    assert n >= 1500


CS_GOLDEN = ["cfg4s_50col_2Mbp", "stress_cs_60col_unal"]


@pytest.mark.parametrize("name", CS_GOLDEN)
def test_oracle_colour_space_sam_matches_reference(name, oracle_lib):
    """the whole colour-space pipeline (colour index, first-colour skip, CS vector filter on the input strand, sw_full_cs,
    post_sw forward-backward, CS SAM fields) against the reference's gmapper-cs"""
    contigs, reads, sam = oa.load_golden(name)
    s = oa.Session(contigs, opts="colour=1")
    s.set(hash_filter_calls=True, sam_unaligned=name.endswith("_unal"))
    got = oa.sam_header(contigs) + s.map_sam(reads, nthreads=4)
    s.close()
    assert got == sam, "oracle colour-space SAM differs from the reference's for %s" % name


def test_oracle_colour_space_on_the_reference_index_fixture(oracle_lib):
    """custom seeds in colour space: the oracle's SAM equals what gmapper-cs printed from its own -S index files"""
    import gzip, os
    d = os.path.join(oa.ROOT, "tests", "golden", "idxfix_cs")
    z = np.load(os.path.join(d, "inputs.npz"))
    with gzip.open(os.path.join(d, "from_index.sam.gz"), "rb") as f:
        sam = f.read()
    contigs = [z["contig0"], z["contig1"]]; names = [bytes(x) for x in z["contig_names"]]
    s = oa.Session(contigs, contig_names=names, opts="colour=1;seeds=%s" % str(z["seeds"]))
    got = oa.sam_header(contigs, names) + s.map_sam(z["reads"], nthreads=2)
    s.close()
    assert got == sam


def _fastq_case(tag):
    import gzip, os
    d = os.path.join(oa.ROOT, "tests", "golden")
    contigs, reads, _ = oa.load_golden("stress_100bp_unal")
    z = np.load(os.path.join(d, "stress_100bp_%s.npz" % tag))
    with gzip.open(os.path.join(d, "stress_100bp_%s.sam.gz" % tag), "rb") as f:
        sam = f.read()
    n = int(z["n_reads"])
    return contigs, reads[:n], [bytes(q.tobytes()) for q in z["quals"]], int(z["qual_delta"]), sam


@pytest.mark.parametrize("tag", ["fq33", "fq64"])
def test_oracle_fastq_quals_match_reference(tag, oracle_lib):
    """FASTQ input: QUAL strings reversed with the read and re-based to PHRED+33 for mapped reads, as read for unmapped ones"""
    contigs, reads, quals, delta, sam = _fastq_case(tag)
    s = oa.Session(contigs); s.set(True, True)
    got = oa.sam_header(contigs) + s.map_sam_q(reads, quals, delta, nthreads=4)
    s.close()
    assert got == sam


def _cs_fastq_case():
    import gzip, os
    d = os.path.join(oa.ROOT, "tests", "golden")
    contigs, reads, _ = oa.load_golden("cfg4s_50col_2Mbp")
    z = np.load(os.path.join(d, "cfg4s_50col_fq.npz"))
    with gzip.open(os.path.join(d, "cfg4s_50col_fq.sam.gz"), "rb") as f:
        sam = f.read()
    n = int(z["n_reads"])
    return contigs, reads[:n], [bytes(q.tobytes()) for q in z["quals"]], int(z["qual_delta"]), sam


def test_oracle_colour_space_fastq_matches_reference(oracle_lib):
    """csfastq: per-position crossover scores from the QVs in sw_full_cs, post_sw with per-colour error rates, QUAL = post_sw's base
    qualities, CQ:Z -- against gmapper-cs"""
    contigs, reads, quals, delta, sam = _cs_fastq_case()
    s = oa.Session(contigs, opts="colour=1"); s.set(True, True)
    got = oa.sam_header(contigs) + s.map_sam_q(reads, quals, delta, nthreads=4)
    s.close()
    assert got == sam


def test_oracle_colour_space_fastq_local_matches_reference(oracle_lib):
    """csfastq with --local: per-position crossover scores in sw_full_cs's local mode (the left-of-band cell of a row takes the row's score, ref: sw-full-cs.c:312-322), no post_sw"""
    import gzip
    contigs, reads, quals, delta, _ = _cs_fastq_case()
    with gzip.open(os.path.join(oa.ROOT, "tests", "golden", "cfg4s_50col_fq@cs_fq_local.sam.gz"), "rb") as f: want = f.read()
    s = oa.Session(contigs, opts="colour=1;local=1"); s.set(True, True)
    got = oa.sam_header(contigs) + s.map_sam_q(reads, quals, delta, nthreads=4)
    s.close()
    assert got == want


def test_oracle_sw_full_ls_local_known_answers(oracle_lib):
    """S2 in local mode: with the anchor box (incl. the threshold-band second run) and without anchors, against the reference's own sw_full_ls"""
    L = oa.load(); u32p = C.POINTER(C.c_uint32); n = 0
    for (goff, glen, rlen, ax, ay, alen, aw, rv, no_anchor, thresh, sv), g, r, want, db, qr in oa.load_kat_local():
        out = (C.c_int * 9)(); dba = C.create_string_buffer(4096); qra = C.create_string_buffer(4096)
        assert L.gmo_sw_full_ls_local(g.ctypes.data_as(u32p), goff, glen, r.ctypes.data_as(u32p), rlen, thresh, sv, ax, ay, alen, aw, 0 if no_anchor else 1, rv,
                                      out, dba, qra, 4096) == 0
        assert list(out) == want and dba.value.decode() == db and qra.value.decode() == qr, (goff, glen, rlen, no_anchor, list(out), want)
        n += 1
    assert n >= 1000


def _paired_fastq_case():
    import gzip, os
    d = os.path.join(oa.ROOT, "tests", "golden")
    g = oa.load_golden_pairs("stress_pairs_2x100")
    z = np.load(os.path.join(d, "stress_pairs_fq33.npz"))
    with gzip.open(os.path.join(d, "stress_pairs_fq33.sam.gz"), "rb") as f:
        sam = f.read()
    n = int(z["n_pairs"])
    g = dict(g, m1=g["m1"][:n], m2=g["m2"][:n], names1=g["names1"][:n], names2=g["names2"][:n])
    return g, [bytes(q.tobytes()) for q in z["quals1"]], [bytes(q.tobytes()) for q in z["quals2"]], int(z["qual_delta"]), sam


def test_oracle_paired_fastq_matches_reference(oracle_lib):
    g, q1, q2, delta, sam = _paired_fastq_case()
    s = oa.Session(g["contigs"], g["contig_names"]); s.set(True, True)
    s.set_pairing(g["mode"], *g["ins"])
    got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs_sam_q(g["m1"], g["m2"], q1, q2, delta, g["names1"], g["names2"], nthreads=4)
    s.close()
    assert got == sam


@pytest.mark.parametrize("tag", sorted(oa.PAIR_MODE_CASES))
def test_oracle_paired_match_modes_match_reference(oracle_lib, tag):
    """-n 3 and -n 2 in paired mode (with and without --no-half-paired) against gmapper -p <mode> -n 3 / -n 2 on committed pairs; each differs from the
    default mode's output on the same pairs"""
    base, opts, _ = oa.PAIR_MODE_CASES[tag]
    g = oa.load_golden_pairs(base); want = oa.load_option_sam(base, tag)
    s = oa.Session(g["contigs"], g["contig_names"], opts=opts); s.set_pairing(g["mode"], *g["ins"])
    got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs_sam(g["m1"], g["m2"], g["names1"], g["names2"], nthreads=4)
    s.close()
    assert got == want
    assert want != g["sam"]


NO_HALF_PAIRED = [("stress_pairs_2x100", "no_half_paired"), ("cfg5s_2x150_1Mbp", "cfg5_no_half_paired")]


@pytest.mark.parametrize("base,tag", NO_HALF_PAIRED)
def test_oracle_no_half_paired_matches_reference(oracle_lib, base, tag):
    """--no-half-paired: mate-pair region counts in the anchor lists (mapping.c:545-608, use_mp_region_counts = 1) and no unpaired rescue.
    The SAM equals the reference's; that the filter itself is restated (it rarely changes the SAM: it removes anchors that cannot pair up)
    shows in the stage counts -- fewer collapsed anchors and windows than with the filter switched off."""
    g = oa.load_golden_pairs(base)
    want = oa.load_option_sam(base, tag)
    counts = {}
    for opts in ("half-paired=0", "half-paired=0;mp-match-mode=0"):
        s = oa.Session(g["contigs"], g["contig_names"], opts=opts)
        s.set_pairing(g["mode"], *g["ins"])
        got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs_sam(g["m1"], g["m2"], g["names1"], g["names2"], nthreads=4)
        counts[opts] = s.last_pair_counts()
        s.close()
        if opts == "half-paired=0": assert got == want
    a, b = counts["half-paired=0"], counts["half-paired=0;mp-match-mode=0"]
    assert a[0] < b[0] and a[1] < b[1], (a, b)


@pytest.mark.parametrize("mode", ["opp-in", "opp-out", "col-fw", "col-bw"])
def test_oracle_colour_space_pairs_match_reference(oracle_lib, mode):
    """gmapper-cs -p <mode> -I 100,600 --sam-unaligned: paired, half-paired and unaligned records with the colour-space fields; three of the modes reverse a mate"""
    g = oa.load_golden_pairs("cs_pairs_50col_" + mode)
    want = g["sam"]
    s = oa.Session(g["contigs"], g["contig_names"], opts="colour=1"); s.set(True, True)
    s.set_pairing(g["mode"], *g["ins"])
    got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs_sam(g["m1"], g["m2"], g["names1"], g["names2"], nthreads=4)
    s.close()
    assert got == want


@pytest.mark.parametrize("tag", sorted(oa.CS_PAIR_OPTION_CASES))
def test_oracle_colour_space_pairs_local_match_reference(oracle_lib, tag):
    """gmapper-cs -p <mode> -I 100,600 --sam-unaligned --local: sw_full_cs in local mode at half the threshold for the mates, no post_sw, no mapping qualities"""
    base, opts, _ = oa.CS_PAIR_OPTION_CASES[tag]
    g = oa.load_golden_pairs(base)
    want = oa.load_option_sam(base, tag)
    s = oa.Session(g["contigs"], g["contig_names"], opts=opts); s.set(True, True)
    s.set_pairing(g["mode"], *g["ins"])
    got = oa.sam_header(g["contigs"], g["contig_names"]) + s.map_pairs_sam(g["m1"], g["m2"], g["names1"], g["names2"], nthreads=4)
    s.close()
    assert got == want, next((a, b) for a, b in zip(got.split(b"\n"), want.split(b"\n")) if a != b)


@pytest.mark.parametrize("tag", sorted(oa.CS_OPTION_CASES))
def test_colour_space_local_and_ungapped_match_reference(tag):
    """gmapper-cs --local (sw_full_cs with local_alignment, ref: sw-full-cs.c:199-203,315,439-552; no post_sw, no mapping qualities) and -U (sw_gapless on colours
    with the forced first colour, ref: sw-gapless.c:84-94): the restatement against the reference's own output"""
    base, opts, _, unal = oa.CS_OPTION_CASES[tag]
    contigs, reads, _ = oa.load_golden(base)
    want = oa.load_option_sam(base, tag)
    o = oa.Session(contigs, opts=opts); o.set(sam_unaligned=unal, hash_filter_calls=("ungapped" not in opts))
    got = oa.sam_header(contigs) + o.map_sam(reads, nthreads=4); o.close()
    assert got == want
    if tag in oa.SCORE_CASE_TAGS:                                  # a golden of the score sets must not pass by being empty
        share, indels = oa.sam_mapped_share_and_indels(want, len(reads))
        assert share >= 0.5 and indels >= 20, (tag, share, indels)


@pytest.mark.parametrize("tag", sorted(oa.RNA_CASES))
def test_oracle_rna_sequences_match_reference(tag, oracle_lib):
    """RNA contigs and RNA reads (uracil and no thymine, ref: fasta.c:528-542): a contig's own flag in its reverse complement and colour translation
    (genome.c:1107-1118), the last contig's flag as genome_is_rna in sw_vector / sw_gapless / sw_full_cs (genome.c:1063-1064; mapping.c:375-388,1318-1327;
    util.h:125-205), a letter-space read's own flag in its reverse complement (gmapper.c:487) -- against gmapper-ls / gmapper-cs on the rna_* fixtures"""
    g = oa.load_rna_case(tag)
    opts = ";".join(x for x in (("colour=1" if g["colour"] else None), g["opts"]) if x)
    s = oa.Session(g["contigs"], g["contig_names"], opts=opts or None); s.set(True, True)
    if g["pairing"]:
        (n1, m1, _), (n2, m2, _) = g["reads"]
        s.set_pairing(*g["pairing"])
        body = s.map_pairs_sam(m1, m2, n1, n2, nthreads=4)
    else:
        names, codes, quals = g["reads"][0]
        if quals is not None:
            s.L.gmo_map_sam_q.restype = C.c_void_p
            s.L.gmo_map_sam_q.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_char_p, C.c_char_p, C.c_int, C.c_int]
            codes = np.ascontiguousarray(codes)
            p = s.L.gmo_map_sam_q(s.h, codes.shape[0], codes.shape[1], codes.ctypes.data_as(C.POINTER(C.c_uint8)), b"\n".join(names), b"\n".join(quals), 33, 4)
            body = C.string_at(p); s.L.gmo_free(p)
        else:
            codes = np.ascontiguousarray(codes)
            p = s.L.gmo_map_sam(s.h, codes.shape[0], codes.shape[1], codes.ctypes.data_as(C.POINTER(C.c_uint8)), b"\n".join(names), 4, None)
            body = C.string_at(p); s.L.gmo_free(p)
    s.close()
    got = oa.sam_header(g["contigs"], g["contig_names"]) + body
    assert got == g["sam"], "oracle SAM differs from the reference's for %s" % tag


def test_oracle_colour_space_kernels_with_is_rna_match_reference_known_answers(oracle_lib):
    """sw_vector (first-colour row) and sw_full_cs (global and local) with is_rna = true on RNA genomes -- lstocs reads U as T, cstols hands back U for T
    (ref: util.h:157-205; sw-vector.c:129,289; sw-full-cs.c:1191) -- against the reference's own functions: 300 vector + 1200 full-SW known answers"""
    import ctypes as C
    L = oa.load(); u32p = C.POINTER(C.c_uint32)
    nc = ns = 0
    for r in oa.load_kat_cs("sw_kat_cs_rna.txt.gz"):
        if r[0] == "C":
            _, goff, glen, rlen, initbp, gcs, gls, rd, score = r
            got = L.gmo_sw_vector_cs_rna(gcs.ctypes.data_as(u32p), goff, glen, rd.ctypes.data_as(u32p), rlen, gls.ctypes.data_as(u32p), initbp)
            assert got == score, (goff, glen, rlen, initbp, got, score); nc += 1
        else:
            kind, (goff, glen, rlen, initbp, ax, ay, alen, awidth, rv, thresh), gls, rd, want, db, qr = r
            out = (C.c_int * 10)(); dba = C.create_string_buffer(4096); qra = C.create_string_buffer(4096)
            assert L.gmo_sw_full_cs_rna(gls.ctypes.data_as(u32p), goff, glen, rd.ctypes.data_as(u32p), rlen, initbp, thresh, C.c_longlong(ax), C.c_longlong(ay), alen, awidth, rv,
                                        1 if kind == "L" else 0, out, dba, qra, 4096) == 0
            if want[0] == 0:
                assert out[0] == 0
            else:
                assert list(out) == want and dba.value == db and qra.value == qr, (list(out), want, dba.value, db, qra.value, qr)
            ns += 1
    assert nc >= 300 and ns >= 1200


def test_oracle_sw_gapless_matches_reference_known_answers(oracle_lib):
    """S1's ungapped filter: the restated sw_gapless (ref: sw-gapless.c:57-117) against the reference's own function -- 2 400 letter- and colour-space answers, and 600
    colour-space answers on RNA genomes with is_rna = true (the forced first colour through lstocs with U read as T, :84)"""
    import ctypes as C, gzip
    L = oa.load(); u32p = C.POINTER(C.c_uint32)
    words = lambda s: np.array([int(x, 16) for x in s.split(",")], dtype=np.uint32)
    n = {}
    for name, rna in (("sw_kat_gapless.txt.gz", 0), ("sw_kat_gapless_rna.txt.gz", 1)):
        with gzip.open(os.path.join(oa.ROOT, "tests", "golden", name), "rt") as f:
            for line in f:
                t = line.split()
                if t[0] != "G": continue
                glen, rlen, g_idx, r_idx, init_bp = (int(x) for x in t[1:6])
                g = words(t[6]); r = words(t[7]); gl = None if t[8] == "-" else words(t[8])
                got = L.gmo_sw_gapless(g.ctypes.data_as(u32p), glen, r.ctypes.data_as(u32p), rlen, g_idx, r_idx, None if gl is None else gl.ctypes.data_as(u32p), init_bp, rna,
                                       10, -15 if gl is None else -24)
                assert got == int(t[9]), (name, t[1:6], got, t[9]); n[name] = n.get(name, 0) + 1
    assert n["sw_kat_gapless.txt.gz"] >= 2400 and n["sw_kat_gapless_rna.txt.gz"] >= 600
