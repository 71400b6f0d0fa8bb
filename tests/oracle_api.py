"""ctypes wrapper over oracle/libgm_oracle.so (the CPU restatement).

TEST INFRASTRUCTURE: imported only by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg -- never by the product package shrimp_amd.
"""
import ctypes as C
import gzip, os, subprocess
import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_LIB = None


def build():
    src = [os.path.join(ROOT, "oracle", f) for f in ("gm_oracle_main.cpp", "gm_oracle.hpp")]
    so = os.path.join(ROOT, "oracle", "libgm_oracle.so")
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in src):
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "libgm_oracle.so"], check=True, capture_output=True)
    return so


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    L = C.CDLL(build())
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    L.gmo_sw_vector.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int]; L.gmo_sw_vector.restype = C.c_int
    L.gmo_sw_full_ls.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_int), C.c_char_p, C.c_char_p, C.c_int]
    L.gmo_sw_full_ls.restype = C.c_int
    L.gmo_sw_full_ls_local.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.POINTER(C.c_int), C.c_char_p, C.c_char_p, C.c_int]
    L.gmo_sw_full_ls_local.restype = C.c_int
    L.gmo_session_create.argtypes = [C.c_int, C.POINTER(u8p), C.POINTER(C.c_uint64), C.c_void_p]; L.gmo_session_create.restype = C.c_void_p
    L.gmo_session_create_opts.argtypes = [C.c_int, C.POINTER(u8p), C.POINTER(C.c_uint64), C.c_void_p, C.c_char_p]; L.gmo_session_create_opts.restype = C.c_void_p
    L.gmo_session_destroy.argtypes = [C.c_void_p]
    L.gmo_session_cutoff.argtypes = [C.c_void_p]; L.gmo_session_cutoff.restype = C.c_uint
    L.gmo_session_set.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.gmo_session_set_half_paired.argtypes = [C.c_void_p, C.c_int]
    L.gmo_last_pair_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.gmo_last_pair_heap_counts.argtypes = [C.POINTER(C.c_uint64)]
    L.gmo_map_sam.argtypes = [C.c_void_p, C.c_int, C.c_int, u8p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64)]; L.gmo_map_sam.restype = C.c_void_p
    L.gmo_session_set_pairing.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.gmo_map_pairs_sam.argtypes = [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int, u8p, C.c_char_p, C.c_char_p, C.c_int]; L.gmo_map_pairs_sam.restype = C.c_void_p
    L.gmo_free.argtypes = [C.c_void_p]
    L.gmo_sw_vector_cs.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, u32p, C.c_int]; L.gmo_sw_vector_cs.restype = C.c_int
    L.gmo_sw_full_cs.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_int), C.c_char_p, C.c_char_p, C.c_int]; L.gmo_sw_full_cs.restype = C.c_int
    L.gmo_index_selfcheck.argtypes = [C.c_void_p, C.c_int]; L.gmo_index_selfcheck.restype = C.c_int
    L.gmo_set_threads.argtypes = [C.c_int]
    L.gmo_map_tophits.argtypes = [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int, C.POINTER(C.c_longlong), C.c_long]; L.gmo_map_tophits.restype = C.c_long
    # the _p family: the kernels with the scores as their first argument (score_array)
    ip = C.POINTER(C.c_int)
    L.gmo_sw_vector_p.argtypes = [ip, u32p, C.c_int, C.c_int, u32p, C.c_int]; L.gmo_sw_vector_p.restype = C.c_int
    L.gmo_sw_vector_cs_p.argtypes = [ip, u32p, C.c_int, C.c_int, u32p, C.c_int, u32p, C.c_int]; L.gmo_sw_vector_cs_p.restype = C.c_int
    L.gmo_sw_vector_batch_p.argtypes = [ip, C.c_int, u32p, u32p, C.POINTER(C.c_longlong), ip, u32p, C.c_int, ip, ip, ip]; L.gmo_sw_vector_batch_p.restype = None
    L.gmo_sw_full_ls_p.argtypes = [ip, u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   ip, C.c_char_p, C.c_char_p, C.c_int]; L.gmo_sw_full_ls_p.restype = C.c_int
    L.gmo_sw_full_cs_p.argtypes = [ip, u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, ip,
                                   ip, C.c_char_p, C.c_char_p, C.c_int]; L.gmo_sw_full_cs_p.restype = C.c_int
    _LIB = L
    return L


PAIR_MODES = {"none": 0, "opp-in": 1, "opp-out": 2, "col-fw": 3, "col-bw": 4}


class Session:
    def __init__(self, contigs, contig_names=None, opts=None):
        self.L = load()
        self.contigs = [np.ascontiguousarray(c, dtype=np.uint8) for c in contigs]
        n = len(self.contigs)
        ptrs = (C.POINTER(C.c_uint8) * n)(*[c.ctypes.data_as(C.POINTER(C.c_uint8)) for c in self.contigs])
        lens = (C.c_uint64 * n)(*[len(c) for c in self.contigs])
        names = None
        if contig_names is not None:
            self._names = (C.c_char_p * n)(*[bytes(x) for x in contig_names]); names = C.cast(self._names, C.c_void_p)
        self.h = self.L.gmo_session_create_opts(n, ptrs, lens, names, opts.encode() if opts else None)

    def index_selfcheck(self, nthreads):
        """chunk-parallel index builder == sequential restatement of load_genome (genome.c:1012-1182)"""
        return bool(self.L.gmo_index_selfcheck(self.h, int(nthreads)))

    def set_pairing(self, mode, min_insert, max_insert):
        self.L.gmo_session_set_pairing(self.h, PAIR_MODES[mode] if isinstance(mode, str) else int(mode), int(min_insert), int(max_insert))

    def map_pairs_sam(self, m1, m2, names1=None, names2=None, nthreads=4):
        m1 = np.ascontiguousarray(m1, dtype=np.uint8); m2 = np.ascontiguousarray(m2, dtype=np.uint8)
        n1 = b"\n".join(bytes(x) for x in names1) if names1 is not None else None
        n2 = b"\n".join(bytes(x) for x in names2) if names2 is not None else None
        p = self.L.gmo_map_pairs_sam(self.h, m1.shape[0], m1.shape[1], m1.ctypes.data_as(C.POINTER(C.c_uint8)),
                                     m2.shape[1], m2.ctypes.data_as(C.POINTER(C.c_uint8)), n1, n2, nthreads)
        s = C.string_at(p); self.L.gmo_free(p)
        return s

    def map_pairs_sam_q(self, m1, m2, quals1, quals2, qual_delta=64, names1=None, names2=None, nthreads=4):
        m1 = np.ascontiguousarray(m1, dtype=np.uint8); m2 = np.ascontiguousarray(m2, dtype=np.uint8)
        n1 = b"\n".join(bytes(x) for x in names1) if names1 is not None else None
        n2 = b"\n".join(bytes(x) for x in names2) if names2 is not None else None
        u8p = C.POINTER(C.c_uint8)
        self.L.gmo_map_pairs_sam_q.restype = C.c_void_p
        self.L.gmo_map_pairs_sam_q.argtypes = [C.c_void_p, C.c_int, C.c_int, u8p, C.c_int, u8p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        p = self.L.gmo_map_pairs_sam_q(self.h, m1.shape[0], m1.shape[1], m1.ctypes.data_as(u8p), m2.shape[1], m2.ctypes.data_as(u8p), n1, n2,
                                       b"\n".join(quals1), b"\n".join(quals2), qual_delta, nthreads)
        s = C.string_at(p); self.L.gmo_free(p)
        return s

    def set_half_paired(self, on):
        self.L.gmo_session_set_half_paired(self.h, int(bool(on)))

    def last_pair_counts(self):
        """(collapsed anchors, windows) over both mates and strands of the last paired call"""
        o = (C.c_uint64 * 2)(); self.L.gmo_last_pair_counts(o); return int(o[0]), int(o[1])

    def last_pair_heap_counts(self):
        """(pairs whose pass-1 pair heap reached num_tmp_outputs, evictions from those heaps) over the last paired call"""
        o = (C.c_uint64 * 2)(); self.L.gmo_last_pair_heap_counts(o); return int(o[0]), int(o[1])

    def set(self, hash_filter_calls=True, sam_unaligned=False):
        self.L.gmo_session_set(self.h, int(hash_filter_calls), int(sam_unaligned))

    @property
    def cutoff(self):
        return self.L.gmo_session_cutoff(self.h)

    def map_sam(self, reads, nthreads=4):
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        n, Lr = reads.shape
        st = (C.c_uint64 * 7)()
        p = self.L.gmo_map_sam(self.h, n, Lr, reads.ctypes.data_as(C.POINTER(C.c_uint8)), None, nthreads, st)
        s = C.string_at(p)
        self.L.gmo_free(p)
        self.stats = dict(vec_calls=st[0], vec_cells=st[1], vec_bypassed=st[2], full_calls=st[3], reads_matched=st[4], dup_pruned=st[5], local_retries=st[6])
        return s

    def map_sam_q(self, reads, quals, qual_delta=64, nthreads=4):
        """FASTQ reads: quals = list of QUAL strings (bytes) as in the file"""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        n, Lr = reads.shape
        self.L.gmo_map_sam_q.restype = C.c_void_p
        self.L.gmo_map_sam_q.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        p = self.L.gmo_map_sam_q(self.h, n, Lr, reads.ctypes.data_as(C.POINTER(C.c_uint8)), None, b"\n".join(quals), qual_delta, nthreads)
        s = C.string_at(p)
        self.L.gmo_free(p)
        return s

    def tophits(self, reads, nthreads=4):
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        n, Lr = reads.shape
        cap = n * 30
        rows = np.zeros((cap, 12), dtype=np.int64)
        w = self.L.gmo_map_tophits(self.h, n, Lr, reads.ctypes.data_as(C.POINTER(C.c_uint8)), nthreads,
                                   rows.ctypes.data_as(C.POINTER(C.c_longlong)), cap)
        return rows[:w]

    def close(self):
        if self.h:
            self.L.gmo_session_destroy(self.h); self.h = None

    def __del__(self):
        try: self.close()
        except Exception: pass


def sw_vector_batch_p(sc, genome, g_off, glen, reads, rlen, genome_ls=None, initbp=None):
    """gmo_sw_vector_batch_p: the oracle's vector filter on n windows at the scores sc (score_array); genome_ls / initbp given: colour space (genome holds colours)"""
    L = load()
    u32p, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    g = np.ascontiguousarray(genome, dtype=np.uint32); r = np.ascontiguousarray(reads, dtype=np.uint32); n = r.shape[0]
    gl = None if genome_ls is None else np.ascontiguousarray(genome_ls, dtype=np.uint32)
    go = np.ascontiguousarray(g_off, dtype=np.int64); gn = np.ascontiguousarray(glen, dtype=np.int32); rl = np.ascontiguousarray(rlen, dtype=np.int32)
    ib = None if initbp is None else np.ascontiguousarray(initbp, dtype=np.int32)
    assert go.shape == gn.shape == rl.shape == (n,) and (gl is None) == (ib is None)
    out = np.zeros(n, dtype=np.int32)
    L.gmo_sw_vector_batch_p(sc, n, g.ctypes.data_as(u32p), None if gl is None else gl.ctypes.data_as(u32p), go.ctypes.data_as(C.POINTER(C.c_longlong)), gn.ctypes.data_as(ip),
                            r.ctypes.data_as(u32p), r.shape[1], rl.ctypes.data_as(ip), None if ib is None else ib.ctypes.data_as(ip), out.ctypes.data_as(ip))
    return out


def sam_header(contigs, names=None):
    names = names if names is not None else [b"contig%d" % (i + 1) for i in range(len(contigs))]
    return b"@HD\tVN:1.0\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (bytes(nm), len(c)) for nm, c in zip(names, contigs))


def load_golden_pairs(name):
    d = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(d, name + ".npz"))
    contigs = [z["contig%d" % i] for i in range(sum(1 for f in z.files if f.startswith("contig") and f[6:].isdigit()))]
    with gzip.open(os.path.join(d, name + ".sam.gz"), "rb") as f:
        sam = f.read()
    return dict(contigs=contigs, contig_names=[bytes(x) for x in z["contig_names"]], m1=z["mates1"], m2=z["mates2"],
                names1=[bytes(x) for x in z["names1"]], names2=[bytes(x) for x in z["names2"]],
                mode=str(z["mode"]), ins=tuple(int(x) for x in z["ins"]), sam=sam)


def load_golden(name):
    d = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(d, name + ".npz"))
    contigs = [z["contig%d" % i] for i in range(len(z.files) - 1)]
    with gzip.open(os.path.join(d, name + ".sam.gz"), "rb") as f:
        sam = f.read()
    return contigs, z["reads"], sam


def parse_words(s):
    return np.array([int(x, 16) for x in s.split(",")], dtype=np.uint32)


def _kat_ls_record(t):
    """one line of a letter-space known-answer file (oracle/ref_kat.cpp), split at blanks"""
    if t[0] == "V":
        return ("V", int(t[1]), int(t[2]), int(t[3]), parse_words(t[4]), parse_words(t[5]), int(t[6]))
    if t[0] == "F":
        return ("F", int(t[1]), int(t[2]), int(t[3]), int(t[4]), int(t[5]), int(t[6]), int(t[7]), int(t[8]),
                parse_words(t[9]), parse_words(t[10]), [int(x) for x in t[11:20]], t[20], t[21])
    # L: goff glen rlen ax ay alen awidth rv no_anchor thresh sv | genome read | 9 ints | dbalign qralign
    return (tuple(int(x) for x in t[1:12]), parse_words(t[12]), parse_words(t[13]), [int(x) for x in t[14:23]], t[23], t[24])


def load_kat():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sw_kat.txt.gz"), "rt") as f:
        for line in f:
            yield _kat_ls_record(line.split())


# name -> match, mismatch, a (open-r, ext-r), b (open-q, ext-q), colour-space crossover: the score sets of the known answers in tests/golden/sw_kat_scores.txt.gz
SCORE_SETS = {
    "unit": (1, -1, -1, -1, -1, -1, -1),
    "linear": (10, -15, 0, -12, 0, -9, -14),
    "swapped": (10, -15, -20, -2, -45, -9, -20),
    "steep": (7, -40, -60, -1, -25, -30, -40),
    "large": (32, -60, -100, -20, -90, -25, -60),
}


def _score_opts(name, colour=False):
    m, mm, ao, ae, bo, be, x = SCORE_SETS[name]
    return "match=%d;mismatch=%d;open-r=%d;ext-r=%d;open-q=%d;ext-q=%d" % (m, mm, ao, ae, bo, be) + (";crossover=%d" % x if colour else "")


def _score_fields(name, colour=False):
    m, mm, ao, ae, bo, be, x = SCORE_SETS[name]
    d = dict(match_score=m, mismatch_score=mm, a_gap_open_score=ao, a_gap_extend_score=ae, b_gap_open_score=bo, b_gap_extend_score=be)
    if colour: d["crossover_score"] = x
    return d


def sam_mapped_share_and_indels(body, n_reads):
    """(share of the reads with a mapped record, number of records whose CIGAR holds an I or a D) of a SAM text"""
    names, indels = set(), 0
    for l in body.split(b"\n"):
        if not l or l.startswith(b"@"): continue
        t = l.split(b"\t")
        if int(t[1]) & 4: continue
        names.add((t[0], int(t[1]) & 0xC0)); indels += (b"I" in t[5] or b"D" in t[5])      # (the mates of a pair share their name: the first / second bits tell them apart)
    return len(names) / n_reads, indels


# Non-default option sets whose reference output is committed as <base>@<tag>.sam.gz (tools/make_golden.py OPTION_CASES):
# tag -> (base golden, oracle option string (the reference's long option names), product gm_params_t fields, seeds, sam_unaligned)
# (-o N sets num_outputs = N and num_tmp_outputs = 20 + N, gmapper.c:1915-1918: the fields name both)
OPTION_CASES = {
    "strata": ("stress_60bp", "strata=1", dict(strata=1), None),
    "max3_o5": ("stress_60bp", "max-alignments=3;report=5", dict(max_alignments=3, num_outputs=5, num_tmp_outputs=25), None),
    "scores": ("stress_100bp_unal", "match=8;mismatch=-12;open-r=-30;open-q=-28;ext-r=-5;ext-q=-4;full-threshold=60;vec-threshold=60;"
               "match-window=150;cmw-overlap=80;cmw-threshold=50;report=6;anchor-width=10",
               dict(match_score=8, mismatch_score=-12, a_gap_open_score=-30, b_gap_open_score=-28, a_gap_extend_score=-5, b_gap_extend_score=-4,
                    sw_full_threshold=60.0, sw_vect_threshold=60.0, window_len=150.0, window_overlap=80.0, window_gen_threshold=50.0,
                    num_outputs=6, num_tmp_outputs=26, anchor_width=10, sam_unaligned=1), None),
    "seeds": ("cfg2s_100bp_2Mbp", "seeds=1111101111,110110110110111,1110100111010111;cutoff=40", dict(list_cutoff=40),
              ["1111101111", "110110110110111", "1110100111010111"]),
    "pairs_strata": ("stress_pairs_2x100", "strata=1;report=4", dict(strata=1, num_outputs=4, num_tmp_outputs=24), None),
    # --local: sw_full_ls with local_alignment = 1 (soft clips), no mapping qualities (MAPQ 255, no Z0/Z1)
    "local": ("stress_100bp_unal", "local=1", dict(local_alignment=1, sam_unaligned=1), None),
    "local60": ("stress_60bp", "local=1;full-threshold=40;vec-threshold=40", dict(local_alignment=1, sw_full_threshold=40.0, sw_vect_threshold=40.0), None),
    "local_cfg2": ("cfg2s_100bp_2Mbp", "local=1", dict(local_alignment=1), None),
    # -U: ungapped filter (sw_gapless) in pass 1, one window per anchor, anchor_width 0, gap opens -255, no f1 cache; needs --local
    "ungapped": ("stress_100bp_unal", "local=1;ungapped=1", dict(local_alignment=1, ungapped=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255,
                                                                    hash_filter_calls=0, sam_unaligned=1), None),
    "ungapped60_n1": ("stress_60bp", "local=1;ungapped=1;cmw-mode=1;full-threshold=45;vec-threshold=45",
                      dict(local_alignment=1, ungapped=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255, hash_filter_calls=0, match_mode=1,
                           sw_full_threshold=45.0, sw_vect_threshold=45.0), None),
    # output policy (output.c:955-1008,1070-1291)
    "single_best": ("stress_60bp", "single-best-mapping=1", dict(single_best_mapping=1), None),
    "all_contigs": ("stress_60bp", "all-contigs=1", dict(all_contigs=1), None),
    "no_mapq": ("stress_100bp_unal", "no-mapping-qualities=1", dict(no_mapping_qualities=1, sam_unaligned=1), None),
    "pairs_single_best": ("stress_pairs_2x100", "single-best-mapping=1", dict(single_best_mapping=1), None),
    "pairs_single_best_all": ("stress_pairs_2x100", "single-best-mapping=1;all-contigs=1", dict(single_best_mapping=1, all_contigs=1), None),
    "pairs_single_best_all_noimp": ("stress_pairs_2x100", "single-best-mapping=1;all-contigs=1;no-improper-mappings=1",
                                    dict(single_best_mapping=1, all_contigs=1, no_improper_mappings=1), None),
    "pairs_no_mapq": ("stress_pairs_2x100", "no-mapping-qualities=1", dict(no_mapping_qualities=1), None),
    # chimeric pairs (mates from different places): improper pairs of two unpaired mappings with --single-best-mapping --all-contigs (output.c:1178-1226)
    "chim_single_best_all": ("chimeric_pairs_2x150", "single-best-mapping=1;all-contigs=1", dict(single_best_mapping=1, all_contigs=1), None),
    "chim_single_best_all_noimp": ("chimeric_pairs_2x150", "single-best-mapping=1;all-contigs=1;no-improper-mappings=1",
                                   dict(single_best_mapping=1, all_contigs=1, no_improper_mappings=1), None),
    "chim_single_best": ("chimeric_pairs_2x150", "single-best-mapping=1", dict(single_best_mapping=1), None),
    # --region-bits / --region-overlap
    "regions_10_30": ("stress_60bp", "region-bits=10;region-overlap=30", dict(region_bits=10, region_overlap=30), None),
    "regions_12_200": ("cfg2s_100bp_2Mbp", "region-bits=12;region-overlap=200", dict(region_bits=12, region_overlap=200), None),
    # -t: Tflag off
    "tiebreak_off": ("stress_100bp_unal", "tiebreak-off=1", dict(tiebreak_rev=0, sam_unaligned=1), None),
    "pairs_tiebreak_off": ("stress_pairs_2x100", "tiebreak-off=1", dict(tiebreak_rev=0), None),
    # -F / -C: one strand only (mapping.c:879-880)
    "positive": ("stress_60bp", "positive=1", dict(strand_only=1), None),
    "negative": ("stress_60bp", "negative=1", dict(strand_only=2), None),
    # -n 1: use_region_counts off -- all list entries are anchors, a window per anchor, one k-mer match is enough (gmapper.c:2610-2625)
    "n1": ("stress_60bp", "cmw-mode=1", dict(match_mode=1), None),
    # -H: hashed seeds (4^12 lists per seed, any weight)
    "hashed": ("stress_60bp", "hash-spaced-kmers=1", dict(hash_seeds=1), None),
    "hashed_w16": ("cfg2s_100bp_2Mbp", "hash-spaced-kmers=1;seeds=11111111101111111,1111110111011101111,111101110010000101111011", dict(hash_seeds=1),
                   ["11111111101111111", "1111110111011101111", "111101110010000101111011"]),
    "pairs_hashed": ("stress_pairs_2x100", "hash-spaced-kmers=1;report=3", dict(hash_seeds=1, num_outputs=3, num_tmp_outputs=23), None),
    "pairs_local": ("stress_pairs_2x100", "local=1", dict(local_alignment=1), None),
    "pairs_ungapped": ("stress_pairs_2x100", "local=1;ungapped=1", dict(local_alignment=1, ungapped=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255,
                                                                        hash_filter_calls=0), None),
    # the production pass-1 / pass-2 kernels at the score sets of tests/test_sw_score_sets.py (SCORE_SETS below)
    "scores_unit": ("stress_100bp_unal", _score_opts("unit"), dict(_score_fields("unit"), sam_unaligned=1), None),
    "scores_swapped": ("stress_100bp_unal", _score_opts("swapped"), dict(_score_fields("swapped"), sam_unaligned=1), None),
    "scores_large": ("stress_100bp_unal", _score_opts("large"), dict(_score_fields("large"), sam_unaligned=1), None),
    "scores_linear": ("stress_60bp", _score_opts("linear"), _score_fields("linear"), None),
    "pairs_scores_swapped": ("stress_pairs_2x100", _score_opts("swapped"), _score_fields("swapped"), None),
}
# the option sets above that exist for their scores: the reference's output for each maps at least half of the reads and holds at least 20 records with an indel
SCORE_CASE_TAGS = ["scores_unit", "scores_swapped", "scores_large", "scores_linear", "pairs_scores_swapped", "cs_scores_swapped", "cs_gate_under", "cs_gate_over"]


# paired match modes (tools/make_golden.py OPTION_CASES pairs_n3 ... cfg5_n2): tag -> (base pair golden, oracle option string, gm_pair_opts_t fields)
#   -n 3: a region marked once counts when the mate has hits within reach (use_mp_region_counts 2; 3 with --no-half-paired), hit list mode 3 (mapping.c:733-742,1080-1093,1153-1157)
#   -n 2: no region counts at all, a window per anchor (gmapper.c:2652-2673)
PAIR_MODE_CASES = {
    "pairs_n3": ("stress_pairs_2x100", "mp-match-mode=3", dict(match_mode=3)),
    "pairs_n3_nhp": ("stress_pairs_2x100", "mp-match-mode=3;half-paired=0", dict(match_mode=3, half_paired=0)),
    "cfg5_n3": ("cfg5s_2x150_1Mbp", "mp-match-mode=3", dict(match_mode=3)),
    "cfg5_n3_nhp": ("cfg5s_2x150_1Mbp", "mp-match-mode=3;half-paired=0", dict(match_mode=3, half_paired=0)),
    "pairs_n2": ("stress_pairs_2x100", "mp-match-mode=2", dict(match_mode=2)),
    # ("param_" fields go to gm_params_t)
    "pairs_hashed_n3": ("stress_pairs_2x100", "hash-spaced-kmers=1;mp-match-mode=3", dict(match_mode=3, param_hash_seeds=1)),
    "pairs_local_n3_nhp": ("stress_pairs_2x100", "local=1;mp-match-mode=3;half-paired=0", dict(match_mode=3, half_paired=0, param_local_alignment=1)),
    "cfg5_n2": ("cfg5s_2x150_1Mbp", "mp-match-mode=2", dict(match_mode=2)),
}

# colour-space option sets (tools/make_golden.py CS_OPTION_CASES: gmapper-cs with these options on a committed colour-space golden's inputs):
# tag -> (base golden, oracle option string, product gm_params_t fields, sam_unaligned)
CS_OPTION_CASES = {
    "cs_local": ("cfg4s_50col_2Mbp", "colour=1;local=1", dict(local_alignment=1), False),
    "cs_local_unal": ("stress_cs_60col_unal", "colour=1;local=1", dict(local_alignment=1, sam_unaligned=1), True),
    "cs_ungapped": ("cfg4s_50col_2Mbp", "colour=1;local=1;ungapped=1", dict(local_alignment=1, ungapped=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255, hash_filter_calls=0), False),
    "cs_ungapped_unal": ("stress_cs_60col_unal", "colour=1;local=1;ungapped=1;full-threshold=40",
                         dict(local_alignment=1, ungapped=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255, hash_filter_calls=0, sw_full_threshold=40.0, sam_unaligned=1), True),
    "cs_tiebreak_off": ("stress_cs_60col_unal", "colour=1;tiebreak-off=1", dict(tiebreak_rev=0, sam_unaligned=1), True),
    "cs_xover_taboo": ("stress_cs_60col_unal", "colour=1;crossover=-25;indel-taboo-len=3;pr-xover=0.05",
                       dict(crossover_score=-25, indel_taboo_len=3, pr_xover=0.05, sam_unaligned=1), True),
    "cs_no_mapq": ("cfg4s_50col_2Mbp", "colour=1;no-mapping-qualities=1", dict(no_mapping_qualities=1), False),
    "cs_single_best": ("stress_cs_60col_unal", "colour=1;single-best-mapping=1", dict(single_best_mapping=1, sam_unaligned=1), True),
    # the production colour-space kernels at other scores.  Pass 2 has two implementations, chosen by gm_launch_pass2_cs: int16_t carry rows while
    # reach = (read_len + window_len) * big < 16000, big = max(|match|, |mismatch|, a open + ext, b open + ext) + |crossover|; else int.  60 colours, windows of 84: 144 moves.
    "cs_scores_swapped": ("stress_cs_60col_unal", "colour=1;" + _score_opts("swapped", True), dict(_score_fields("swapped", True), sam_unaligned=1), True),   # reach 144 * (54 + 20) = 10656: int16_t
    # large gap and crossover penalties on either side of the gate: big = 71 + 40 = 111 and 72 + 40 = 112
    "cs_gate_under": ("stress_cs_60col_unal", "colour=1;crossover=-40;open-r=-60;ext-r=-11;open-q=-55;ext-q=-10",
                      dict(crossover_score=-40, a_gap_open_score=-60, a_gap_extend_score=-11, b_gap_open_score=-55, b_gap_extend_score=-10, sam_unaligned=1), True),   # reach 144 * 111 = 15984: int16_t
    "cs_gate_over": ("stress_cs_60col_unal", "colour=1;crossover=-40;open-r=-60;ext-r=-12;open-q=-55;ext-q=-10",
                     dict(crossover_score=-40, a_gap_open_score=-60, a_gap_extend_score=-12, b_gap_open_score=-55, b_gap_extend_score=-10, sam_unaligned=1), True),    # reach 144 * 112 = 16128: int
}


# colour-space pairs with options (tools/make_golden.py CS_PAIR_OPTION_CASES): tag -> (base pair golden, oracle option string, product gm_params_t fields)
CS_PAIR_OPTION_CASES = {
    "cs_pairs_local": ("cs_pairs_50col_opp-in", "colour=1;local=1", dict(local_alignment=1)),
    "cs_pairs_local_colbw": ("cs_pairs_50col_col-bw", "colour=1;local=1", dict(local_alignment=1)),
    # paired match modes in colour space ("pair_" fields go to gm_pair_opts_t)
    "cs_pairs_n3": ("cs_pairs_50col_opp-in", "colour=1;mp-match-mode=3", dict(pair_match_mode=3)),
    "cs_pairs_n3_colbw_nhp": ("cs_pairs_50col_col-bw", "colour=1;mp-match-mode=3;half-paired=0", dict(pair_match_mode=3, pair_half_paired=0)),
    "cs_pairs_n2": ("cs_pairs_50col_opp-in", "colour=1;mp-match-mode=2", dict(pair_match_mode=2)),
}


# -M mirna (gmapper.c:1497-1517 + gmapper-defaults.h:230-238): (oracle option string, gm_params_t fields, seeds)
MIRNA_SEEDS = ["00111111001111111100", "00111111110011111100", "00111111111100111100", "00111111111111001100", "00111111111111110000"]
MIRNA_MODE = ("hash-spaced-kmers=1;seeds=%s;local=1;ungapped=1;cmw-mode=1;match-window=100" % ",".join(MIRNA_SEEDS),
              dict(hash_seeds=1, ungapped=1, local_alignment=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255, hash_filter_calls=0, match_mode=1,
                   window_len=100.0), MIRNA_SEEDS)


# the optional tail of the SAM records (--extra-sam-fields, --read-group, --sam-r2; output.c:452-465,729-756): host formatting pinned on the product directly against the
# reference's output -- the oracle does not restate it.  tag -> (base golden, gm_params_t fields, colour space, pairs)
SAM_TAIL_CASES = {
    "extra_fields": ("cfg2s_100bp_2Mbp", dict(extra_sam_fields=1), False, False),
    "extra_fields_rg_unal": ("n1_noisy_70bp", dict(extra_sam_fields=1, read_group=b"grp1", sam_unaligned=1), False, False),
    "rg_unal": ("stress_100bp_unal", dict(read_group=b"grp1", sam_unaligned=1), False, False),
    "pairs_r2_rg_extra": ("cfg5s_2x150_1Mbp", dict(sam_r2=1, read_group=b"grp1", extra_sam_fields=1), False, True),
    "pairs_r2_rg": ("stress_pairs_2x100", dict(sam_r2=1, read_group=b"grp1"), False, True),
    "cs_extra_rg": ("cfg4s_50col_2Mbp", dict(extra_sam_fields=1, read_group=b"grp1", sam_unaligned=1), True, False),
    "cs_pairs_r2_extra": ("cs_pairs_50col_col-bw", dict(sam_r2=1, extra_sam_fields=1, sam_unaligned=1), True, True),
}


# Seed sets beyond the ones the option cases use (tools/make_golden.py --seeds-only, tests/test_seed_sets.py): name -> (seed strings, -H).
# ref_*: the four non-default rows of the reference's table of default seeds by weight (gmapper-defaults.h:216-227; weights 16 and 18 are the ones its README gives
# for long reads with -H: spans up to 30, four words of eight positions under the hashed key).  The rest: the library's limits (span 32, weight 14 without -H,
# 16 seeds) and the shapes next to them, drawn once and fixed here.
SEED_SETS = {
    "ref_w10": (["111110011111", "111100110001111", "111100100100100111", "111001000100001001111"], False),
    "ref_w11": (["1111001111111", "1111100110001111", "11110010010001001111", "11100110010000100100111"], False),
    "ref_w16H": (["111111101110111111", "1111100101101101011111", "11110011001010100011011111", "111101001100000100110011010111"], True),
    "ref_w18H": (["11111011111110111111", "11110111011010111011111", "11111100110101101001011111", "11111010101100100010011101111"], True),
    "span32": (["10000000001000000010001111101111"], False),                                    # weight 12: every bit of the 64-bit mask in use
    "span32H": (["11101101110010000101100011101001"], True),                                   # weight 17
    "span32_14": (["10000000001000000010001111101111", "11110111101111"], False),              # mixed spans share one max_seed_span
    "span31_25H": (["1010011011100100111110111111001", "1001111111110010010100011"], True),    # weights 20 and 15
    "one": (["11110111101111"], False),                                                        # the default's first seed alone
    "sixteen": (["110111111111", "1010111111111", "11101010111111", "1110011011101011", "11110110011100101", "111010110011010011", "11011010011110100001",
                 "100001011110010011101", "1100100011110001011001", "111010011101000010000011", "1010100011101000000110011", "11100100000100011110100001",
                 "1001000010101011010000010101", "10000001100001000000011111011", "110001100111000001000000001011", "10001001100001010010001010010001"], False),   # GM_MAX_SEEDS, weight 11, spans 12 .. 32
    "w13": (["11101111111100011", "1110110000111001100111"], False),
    "w14": (["10111111101011000111"], False),                                                  # MAX_SEED_WEIGHT: 4^14 lists
    "contiguous": (["111111111111"], False),
}
# the runs of every set: tag suffix -> (input golden, reads taken from its front (None: all), colour space, -n 1)
SEED_RUNS = {
    "": ("stress_100bp_unal", None, False, False),
    "_n1": ("n1_noisy_70bp", 1500, False, True),
    "_def": ("n1_noisy_70bp", 1500, False, False),
    "_cs": ("stress_cs_60col_unal", 600, True, False),
}
SEED_RUNS_NO_EXTRA = ("",)                          # the reference does not return from --extra-sam-fields on stress_100bp_unal (an N in a reversed edit string): stored without them
SEED_RUNS_W14 = ("", "_def")                       # w14 runs on the two default-mode letter-space inputs only
# the index fixtures of the seed sets (tests/golden/<name>/, tools/make_golden.py seed_index_cases): name -> (seed strings, -H)
SEED_INDEX_CASES = {
    "idxfix_h30": (SEED_SETS["ref_w16H"][0], True),                                            # four mask words in the reference's -S files
    "idxfix_s32": (["10101000010010000010000010000001", "110110111"], False),                 # span 32 at weight 8 (4^8 lists keep the files small)
}


def seed_runs(name):
    return [r for r in SEED_RUNS if name != "w14" or r in SEED_RUNS_W14]


def seed_oracle_opts(seeds, hashed, colour=False, n1=False):
    """the oracle's option string of a seed set"""
    return ("colour=1;" if colour else "") + ("hash-spaced-kmers=1;" if hashed else "") + ("cmw-mode=1;" if n1 else "") + "seeds=" + ",".join(seeds)


def load_seed_sam(name, run):
    """the reference's records (no header, no @PG) of seed set `name` on run `run` of SEED_RUNS, written with --extra-sam-fields --sam-unaligned"""
    base = SEED_RUNS[run][0]
    tag = {"": "", "_n1": "_n1", "_def": "", "_cs": ""}[run]
    return load_option_sam(base, "seeds_%s%s" % (name, tag))


def load_option_sam(base, tag):
    with gzip.open(os.path.join(ROOT, "tests", "golden", "%s@%s.sam.gz" % (base, tag)), "rb") as f:
        return f.read()


# Window and anchor-band geometry off the defaults (tools/make_golden.py --geometry-only, tests/test_window_geometry.py): -a anchor width (-1: no anchor band, the
# threshold band in every full alignment), -w window length, -l window overlap, -r window generation threshold (a trailing % in the reference's options: of the read
# length / the window / the best score; without it an absolute count -- a negative value in the oracle's options and in gm_params_t), -h / -v the full and the vector
# threshold (letter space takes -h for both, gmapper.c), -z the list cutoff.  The inputs are committed ones, cut to their first GEOMETRY_READS reads or pairs; only the
# reference's records are stored, as <input>@geo_<tag>.sam.gz.
GEOMETRY_READS = {"stress_60bp": 1500, "stress_100bp_unal": 1500, "stress_cs_60col_unal": 600, "stress_pairs_2x100": 600, "pair_edges_opp-in": 378, "pair_edges_col-bw": 378}
# (on the first 1 500 reads -h 437 moves 4 records only, on the whole input 6; -w 300% moves 2 records of the first 600 colour-space reads, 5 of the first 1 400)
# -w 170 -l 30 moves the records of one pair among the first 600, of two among the first 900
GEOMETRY_READS_OF = {"stress_60bp:h437abs": 3000, "stress_cs_60col_unal:w300": 1400, "stress_pairs_2x100:w170abs_l30abs": 900}
GEOMETRY_UNAL = ("stress_100bp_unal", "stress_cs_60col_unal")      # inputs whose goldens are made with --sam-unaligned
_W100 = (["-w", "100%"], "match-window=100", dict(window_len=100.0))
_GEO_SETS = {      # what -> (the reference's options, the oracle's, gm_params_t fields; "pair_" fields go to gm_pair_opts_t)
    "a-1": (["-a", "-1"], "anchor-width=-1", dict(anchor_width=-1)),
    "a0": (["-a", "0"], "anchor-width=0", dict(anchor_width=0)),
    "a1": (["-a", "1"], "anchor-width=1", dict(anchor_width=1)),
    "a99": (["-a", "99"], "anchor-width=99", dict(anchor_width=99)),
    "w100": _W100,
    "w250": (["-w", "250%"], "match-window=250", dict(window_len=250.0)),
    "w300": (["-w", "300%"], "match-window=300", dict(window_len=300.0)),
    "w131abs": (["-w", "131"], "match-window=-131", dict(window_len=-131.0)),
    "w61abs": (["-w", "61"], "match-window=-61", dict(window_len=-61.0)),
    "w60abs": (["-w", "60"], "match-window=-60", dict(window_len=-60.0)),
    "w50abs": (["-w", "50"], "match-window=-50", dict(window_len=-50.0)),                      # a window shorter than the read
    "l20abs": (["-l", "20"], "cmw-overlap=-20", dict(window_overlap=-20.0)),
    "l100": (["-l", "100%"], "cmw-overlap=100", dict(window_overlap=100.0)),
    "l10": (["-l", "10%"], "cmw-overlap=10", dict(window_overlap=10.0)),
    "r250abs": (["-r", "250"], "cmw-threshold=-250", dict(window_gen_threshold=-250.0)),
    "r90": (["-r", "90%"], "cmw-threshold=90", dict(window_gen_threshold=90.0)),
    "h437abs": (["-h", "437"], "full-threshold=-437;vec-threshold=-437", dict(sw_full_threshold=-437.0, sw_vect_threshold=-437.0)),
    "z5": (["-z", "5"], "cutoff=5", dict(list_cutoff=5)),
    "v40_h80": (["-v", "40%", "-h", "80%"], "vec-threshold=40;full-threshold=80", dict(sw_vect_threshold=40.0, sw_full_threshold=80.0)),
    "local_a-1": (["--local", "-a", "-1"], "local=1;anchor-width=-1", dict(local_alignment=1, anchor_width=-1)),
    "w100_a-1": (["-w", "100%", "-a", "-1"], "match-window=100;anchor-width=-1", dict(window_len=100.0, anchor_width=-1)),
    "w100_n1": (["-w", "100%", "-n", "1"], "match-window=100;cmw-mode=1", dict(window_len=100.0, match_mode=1)),
    "w170abs_l30abs": (["-w", "170", "-l", "30"], "match-window=-170;cmw-overlap=-30", dict(window_len=-170.0, window_overlap=-30.0)),
    "w100_nhp": (["-w", "100%", "--no-half-paired"], "match-window=100;half-paired=0", dict(window_len=100.0, pair_half_paired=0)),
    "w250_n3": (["-w", "250%", "-n", "3"], "match-window=250;mp-match-mode=3", dict(window_len=250.0, pair_match_mode=3)),
}
_GEO_ON = {
    "stress_60bp": ["a-1", "a0", "a1", "a99", "w100", "w300", "w131abs", "w60abs", "w61abs", "w50abs", "l20abs", "l100", "l10", "r250abs", "r90", "h437abs", "z5",
                    "local_a-1", "w100_a-1", "w100_n1"],
    "stress_100bp_unal": ["a-1", "a0", "a1", "a99", "w100", "w300", "l20abs", "r90", "z5", "local_a-1"],      # w300: windows of 300 > 256 columns under one stripe
    "stress_cs_60col_unal": ["a-1", "a0", "w100", "w300", "v40_h80", "local_a-1"],
    "stress_pairs_2x100": ["w100", "w250", "a-1", "a0", "w170abs_l30abs", "w100_nhp", "w250_n3"],
    "pair_edges_opp-in": ["w100"],      # mates of 40 and 60 bases: window_len - read_len is 0 for both, the four delta_g_off formulas of the mate ranges collapse
    "pair_edges_col-bw": ["w100"],
}
# tag -> (input, the reference's options, the oracle's options, gm_params_t / pair_ fields)
GEOMETRY_CASES = {"%s:%s" % (base, what): (base,) + _GEO_SETS[what] for base, whats in _GEO_ON.items() for what in whats}
GEOMETRY_MIN_DISTANCE = 5      # records of a golden that are not in its input's default golden; and of -a -1 / -a 99 that are not in -a 0
# ... but for colour space -a -1: there the threshold band and the default band of width 8 give the same records on this input, and its distance from -a 0 stands alone
GEOMETRY_SAME_AS_DEFAULT = ("stress_cs_60col_unal:a-1",)


def geometry_kind(base):
    """'cs', 'pairs' or 'ls'"""
    return "cs" if "_cs_" in base else ("pairs" if "pairs" in base or base.startswith("pair_") else "ls")


def geometry_file(tag):
    base, what = tag.split(":")
    return "%s@geo_%s.sam.gz" % (base, what)


def load_geometry_sam(tag):
    """the reference's records (no header) of a geometry case"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", geometry_file(tag)), "rb") as f:
        return f.read()


def geometry_reads(tag):
    """reads / pairs of its input a geometry case runs on, from the input's front"""
    return GEOMETRY_READS_OF.get(tag, GEOMETRY_READS[tag.split(":")[0]])


def geometry_default_records(base, n=None):
    """the records of the input's default golden that belong to its first n (GEOMETRY_READS) reads / pairs, header dropped (the goldens are written in read order)"""
    n = n or GEOMETRY_READS[base]
    if geometry_kind(base) == "pairs":
        g = load_golden_pairs(base); keep = {x[:-2] for x in g["names1"][:n]}; sam = g["sam"]      # (the mates' names without their /1, :1)
    else:
        keep = {b"r%d" % i for i in range(n)}; sam = load_golden(base)[2]
    return b"".join(l + b"\n" for l in sam.split(b"\n") if l and not l.startswith(b"@") and l.split(b"\t", 1)[0] in keep)


def sam_distance(body, other):
    """records of `body` that are not records of `other`"""
    have = set(other.split(b"\n"))
    return sum(1 for l in body.split(b"\n") if l and l not in have)


# Reads of 128 to 1 000 bases and colours (tools/make_golden.py --long-only, tests/test_long_reads.py).  One genome for all of them, stored once as long_genome.npz
# (long_stress_genome of the generator: contig0, contig1 and `repeat`, the bounds of contig 0's repeat part); an input is long_<name>.npz (reads, or mates1 / mates2 /
# names1 / names2 / mode / ins) and names the genome; the reference's body under an option set is long_<name>@<set>.sam.gz ("default" for none), made with --sam-unaligned.
GM_SWF_LDS_LIMIT = 160 * 1024


def gm_pass2_g4_lds(ng, read_len, window_len):
    """shrimp_amd/csrc/gm_pass2_sizes.h restated (tests/host/pass2_sizes_main.cpp holds the two together)"""
    r16 = (read_len + 15) & ~15; w16 = (window_len + 15) & ~15
    return ng * r16 + ng * w16 + ng * window_len * 3 * (2 if ng == 8 else 4) + 64


def gm_pass2_cs_lds(ng, read_len, window_len):
    q16 = (read_len + 15) & ~15; w16 = (window_len + 15) & ~15
    return ng * 5 * q16 + ng * w16 + ng * window_len * 12 * (2 if ng == 8 else 4) + 64


def gm_pass2_max_window(colour, local, read_len):
    lds = (lambda W: gm_pass2_g4_lds(4, read_len, W)) if not colour else (lambda W: gm_pass2_cs_lds(4 if local else 1, read_len, W))
    lo, hi = 0, 65535
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if lds(mid) <= GM_SWF_LDS_LIMIT: lo = mid
        else: hi = mid - 1
    return lo


def default_window(read_len):
    """window_len_of at -w 140 %"""
    return int(read_len * (140.0 / 100.0)) & 0xFFFF


def pass2_kernel(colour, read_len, local=False, big=None):
    """the kernel gm_launch_pass2 / gm_launch_pass2_cs choose for reads of read_len under default windows and scores (big: the largest change of the score a move can
    make, 40 + 20 at the colour-space defaults), as gm_last_pass2_kernel() names it"""
    W = default_window(read_len)
    if not colour: return "k_pass2_g4<16,int>"
    reach = (read_len + W) * (big or 60)
    if reach < 16000 and gm_pass2_cs_lds(8, read_len, W) <= 64 * 1024: return "k_pass2_cs_g4<8,int16_t>"
    if gm_pass2_cs_lds(4, read_len, W) <= GM_SWF_LDS_LIMIT: return "k_pass2_cs_g4<16,int>"
    assert not local
    return "k_pass2_cs"


def _last_true(pred, lo, hi):
    """the largest L in [lo, hi] with pred(L), pred true at lo and monotone"""
    assert pred(lo)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if pred(mid): lo = mid
        else: hi = mid - 1
    return lo


# the last read length the four-window colour-space kernel takes at default windows, and the last one colour-space --local is admitted at (check_read_len)
LONG_CS_G4_LAST = _last_true(lambda L: gm_pass2_cs_lds(4, L, default_window(L)) <= GM_SWF_LDS_LIMIT, 100, 1000)
LONG_CS_LOCAL_LAST = _last_true(lambda L: L * (140.0 / 100.0) <= gm_pass2_max_window(1, 1, L), 100, 1000)

_W16H = SEED_SETS["ref_w16H"][0]
_LONG_SETS = {      # set -> (the reference's options, the oracle's, gm_params_t fields ("pair_": gm_pair_opts_t), seed strings or None)
    "default": ([], "", {}, None),
    "local": (["--local"], "local=1", dict(local_alignment=1), None),
    "n1": (["-n", "1"], "cmw-mode=1", dict(match_mode=1), None),
    "w16H": (["-H", "-s", ",".join(_W16H)], "hash-spaced-kmers=1;seeds=" + ",".join(_W16H), dict(hash_seeds=1), _W16H),
    "extra": (["--extra-sam-fields"], "extra-sam-fields=1", dict(extra_sam_fields=1), None),
    "w110": (["-w", "110%"], "match-window=110", dict(window_len=110.0), None),
    "o5_strata": (["-o", "5", "--strata"], "report=5;strata=1", dict(num_outputs=5, num_tmp_outputs=25, strata=1), None),
    "ungapped": (["--local", "-U"], "local=1;ungapped=1", dict(local_alignment=1, ungapped=1, anchor_width=0, a_gap_open_score=-255, b_gap_open_score=-255, hash_filter_calls=0), None),
    # (colour space at unit scores: a move changes the score by 3 at the most, so `reach` stays far below 16 000 and the eight-window kernel's 64 KB decide at 204 / 205)
    "unit": (["-m", "1", "-i", "-1", "-g", "-1", "-e", "-1", "-q", "-1", "-f", "-1", "-x", "-1"], _score_opts("unit", True), _score_fields("unit", True), None),
    # FASTQ input with PHRED+33 qualities (letter space: --qv-offset 33; csfastq is PHRED+33 by default): the QUAL strings come with the input, not with the options
    "fq": (["--qv-offset", "33"], "", {}, None),
    "csfq": ([], "", {}, None),
    "nhp": (["--no-half-paired"], "half-paired=0", dict(pair_half_paired=0), None),
    "n3": (["-n", "3"], "mp-match-mode=3", dict(pair_match_mode=3), None),
}


def long_reads_of(length):
    """reads of an unpaired input: 200 up to 257 bases or colours, 100 up to 557, 60 at 700, 40 letter-space or 30 colour-space reads at 1 000 (long_inputs)"""
    return 200 if length <= 257 else (100 if length <= max(557, LONG_CS_G4_LAST + 1) else (60 if length < 1000 else 40))


def _long_inputs():
    """name -> dict(kind, length(s), n, seed, sets, and for pairs mode and ins)"""
    d = {}
    ls = {128: [], 129: ["local", "extra"], 183: [], 184: ["n1"], 256: [], 257: ["w16H", "extra"], 385: [], 400: ["local", "n1", "o5_strata"], 700: ["extra"], 1000: ["local", "w16H", "w110"]}
    for k, (L, more) in enumerate(sorted(ls.items())):
        d["ls_%d" % L] = dict(kind="ls", len=L, n=long_reads_of(L), seed=4117 if L == 1000 else 4100 + k, sets=["default"] + more, clean="extra" in more)
    cs = {129: ["local"], 204: ["unit"], 205: ["unit"], LONG_CS_G4_LAST: [], LONG_CS_G4_LAST + 1: [], 400: ["local", "ungapped"], 1000: []}
    for k, (L, more) in enumerate(sorted(cs.items())):
        d["cs_%d" % L] = dict(kind="cs", len=L, n=30 if L == 1000 else long_reads_of(L), seed=4200 + k, sets=["default"] + more)
    # FASTQ at 400 bases (QUAL lines of that length), csfastq at 200 colours (per-position crossover rows of that length)
    d["ls_400q"] = dict(kind="ls", len=400, n=100, seed=4150, sets=["fq"], fq=33)
    d["cs_200q"] = dict(kind="cs", len=200, n=200, seed=4250, sets=["csfq"], fq=33)
    d["cs_%d" % LONG_CS_LOCAL_LAST] = dict(kind="cs", len=LONG_CS_LOCAL_LAST, n=60, seed=4290, sets=["local"])
    pr = [("pairs_2x250_opp-in", (250, 250), 100, "opp-in", (200, 1200), ["default", "nhp", "n3"]),
          ("pairs_400_100_col-fw", (400, 100), 100, "col-fw", (200, 1500), ["default", "nhp"]),
          ("pairs_400_100_col-bw", (400, 100), 100, "col-bw", (200, 1500), ["default", "nhp"]),
          ("pairs_2x250_opp-out", (250, 250), 100, "opp-out", (200, 1200), ["default", "nhp"]),
          ("pairs_2x700_opp-in", (700, 700), 40, "opp-in", (700, 3000), ["default", "nhp"]),
          ("cs_pairs_2x150_opp-in", (150, 150), 100, "opp-in", (200, 1200), ["default", "nhp"])]
    # (share: of the pairs drawn from the repeat part.  Under --no-half-paired the reference loses a quarter of the 400 + 100 pairs that lie in unique sequence and none of
    # those in the repeats; with half of the pairs there fewer than 90 % of the mates keep a record, with four fifths they do -- on one draw of the col-bw pairs in eight: 83 to 87 of 100 pairs stay paired on the others, 91 on seed 4312)
    for k, (name, lens, n, mode, ins, sets) in enumerate(pr):
        d[name] = dict(kind="cs_pairs" if name.startswith("cs_") else "pairs", len=lens, n=n, seed=4312 if mode == "col-bw" else 4300 + k, sets=sets, mode=mode, ins=ins, share=0.8 if lens == (400, 100) else 0.5)
    return d


LONG_INPUTS = _long_inputs()
# tag "<input>:<set>" -> (input, the reference's options, the oracle's options, fields, seeds)
LONG_CASES = {"%s:%s" % (name, st): (name,) + _LONG_SETS[st] for name, inp in LONG_INPUTS.items() for st in inp["sets"]}
# (-U aligns without gaps: no record of it can hold an I or a D)
LONG_NO_INDELS = ("cs_400:ungapped",)
# (--strata prints the mappings of a read's best score alone: a read has a second record only where two places tie, which 3 % substitutions leave to a few reads)
LONG_NO_MULTI = ("ls_400:o5_strata",)
# what every fixture holds at the least (tools/make_golden.py asserts it when it writes them, tests/test_long_reads.py on the committed files): shares of the reads with a
# mapped record and with more than one, of the records on the reverse strand and with an I or a D in the CIGAR; pairs: the properly paired share of the pairs and, with
# half-paired mappings allowed, the share of the records that are half-paired or unpaired
LONG_MIN = dict(mapped=0.90, multi=0.10, reverse=0.30, indel=0.50, proper=0.60, loose=0.05)


def long_file(tag):
    name, st = tag.split(":")
    return "long_%s@%s.sam.gz" % (name, st)


def load_long_sam(tag):
    with gzip.open(os.path.join(ROOT, "tests", "golden", long_file(tag)), "rb") as f:
        return f.read()


_long_genome = []
def load_long_genome():
    """(contigs, (lo, hi) of the repeat part of contig 0)"""
    if not _long_genome:
        z = np.load(os.path.join(ROOT, "tests", "golden", "long_genome.npz"))
        _long_genome.append(([z["contig0"], z["contig1"]], tuple(int(x) for x in z["repeat"])))
    return _long_genome[0]


def load_long_input(name):
    """the genome's contigs beside an input's arrays: reads, or m1 / m2 / names1 / names2 / mode / ins"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "long_%s.npz" % name))
    assert str(z["genome"]) == "long_genome"
    g = dict(contigs=load_long_genome()[0], contig_names=[b"contig1", b"contig2"])
    if "reads" in z.files:
        g["reads"] = z["reads"]
        if "quals" in z.files: g["quals"] = [bytes(q) for q in z["quals"]]; g["qual_delta"] = int(z["qual_delta"])
    else: g.update(m1=z["mates1"], m2=z["mates2"], names1=[bytes(x) for x in z["names1"]], names2=[bytes(x) for x in z["names2"]], mode=str(z["mode"]), ins=tuple(int(x) for x in z["ins"]))
    return g


def long_counts(body, n, pairs=False):
    """the counts LONG_MIN speaks of, from a SAM body without header lines: n reads (pairs: n pairs, a mate a read)"""
    per = {}; recs = rev = indel = loose = 0; proper = set()
    for l in body.split(b"\n"):
        if not l or l.startswith(b"@"): continue
        t = l.split(b"\t"); fl = int(t[1])
        if fl & 4: continue
        key = (t[0], fl & 0xC0); per[key] = per.get(key, 0) + 1
        recs += 1; rev += bool(fl & 16); indel += (b"I" in t[5] or b"D" in t[5])
        if pairs:
            if fl & 2: proper.add(t[0])
            else: loose += 1
    reads = 2 * n if pairs else n
    d = dict(reads=reads, records=recs, mapped=len(per), multi=sum(1 for v in per.values() if v > 1), reverse=rev, indel=indel)
    if pairs: d.update(pairs=n, proper=len(proper), loose=loose)
    return d


def long_conditions(tag, c):
    """the conditions of LONG_MIN a fixture with the counts c misses (an empty list: none)"""
    m = LONG_MIN; bad = []
    if c["mapped"] < m["mapped"] * c["reads"]: bad.append("mapped")
    if tag not in LONG_NO_MULTI and c["multi"] < m["multi"] * c["reads"]: bad.append("multi")
    if c["reverse"] < m["reverse"] * c["records"]: bad.append("reverse")
    if tag not in LONG_NO_INDELS and c["indel"] < m["indel"] * c["records"]: bad.append("indel")
    if "pairs" in c:
        if c["proper"] < m["proper"] * c["pairs"]: bad.append("proper")
        if not tag.endswith(":nhp") and c["loose"] < m["loose"] * c["records"]: bad.append("loose")
    return bad


def load_kat_anchors(colour=False):
    """the known answers of the full alignments at other anchor widths than 8 (oracle/ref_kat.cpp / ref_kat_cs.cpp, mode "anchors"): (name, setup, records) a width as
    load_kat_scores gives them; the setup tuple ends with the width.  Letter space: F records (global, threshold 0), and G / L records in the L records' layout (global /
    local at a threshold of half the read, with the box and without); colour space: S and L records."""
    sets = []
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sw_kat_cs_anchors.txt.gz" if colour else "sw_kat_anchors.txt.gz"), "rb" if colour else "rt") as f:
        for line in f:
            t = line.split()
            if t[0] in ("P", b"P"): sets.append((t[1].decode() if colour else t[1], tuple(int(x) for x in t[2:]), []))
            elif colour: sets[-1][2].append(_kat_cs_record(t))
            elif t[0] == "G": sets[-1][2].append(("G",) + _kat_ls_record(["L"] + t[1:]))
            else: sets[-1][2].append(_kat_ls_record(t))
    return sets


def load_kat_local():
    """sw_full_ls in local mode (Gflag off), with an anchor box and without, from the reference's own function (oracle/ref_kat.cpp local)"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sw_kat_local.txt.gz"), "rt") as f:
        for line in f:
            t = line.split()
            if t[0] != "L": continue
            yield _kat_ls_record(t)


def _kat_cs_record(t):
    """one line of a colour-space known-answer file (oracle/ref_kat_cs.cpp), split at blanks (bytes)"""
    words = lambda t: np.array([int(x, 16) for x in t.split(b",")], dtype=np.uint32)
    if t[0] == b"C":
        return ("C", int(t[1]), int(t[2]), int(t[3]), int(t[4]), words(t[5]), words(t[6]), words(t[7]), int(t[8]))
    if t[0] in (b"X", b"Y"):      # per-position crossover scores behind the read words (X: global, Y: local mode)
        return (t[0].decode(), [int(x) for x in t[1:11]], words(t[11]), words(t[12]), [int(x) for x in t[14:24]],
                b"" if t[24] == b"-" else t[24], b"" if t[25] == b"-" else t[25], np.array([int(x) for x in t[13].split(b",")], dtype=np.int32))
    return (t[0].decode(), [int(x) for x in t[1:11]], words(t[11]), words(t[12]), [int(x) for x in t[13:23]],
            b"" if t[23] == b"-" else t[23], b"" if t[24] == b"-" else t[24])


def load_kat_cs(name="sw_kat_cs.txt.gz"):
    """colour-space known answers produced by the reference's own sw_vector(use_colours) / sw_full_cs (oracle/ref_kat_cs.cpp); sw_kat_cs_local.txt.gz: "L" records, sw_full_cs in local mode"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", name), "rb") as f:
        return [_kat_cs_record(line.split()) for line in f]


def load_kat_scores(colour=False):
    """the known answers under other score sets than the defaults (oracle/ref_kat.cpp / ref_kat_cs.cpp, mode "scores"): a list of (name, setup, records), one entry a set.
    setup = dblen, qrlen, a_open, a_ext, b_open, b_ext, match, mismatch (colour space: + crossover, indel_taboo_len) -- the setups' arguments in their order.
    Letter space: records as load_kat gives them ("V", "F") and as load_kat_local does (the L records: their first field is a tuple);
    colour space: records as load_kat_cs gives them (C, S, L, X, Y)."""
    sets = []
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sw_kat_cs_scores.txt.gz" if colour else "sw_kat_scores.txt.gz"), "rb" if colour else "rt") as f:
        for line in f:
            t = line.split()
            if t[0] in ("P", b"P"):
                sets.append((t[1].decode() if colour else t[1], tuple(int(x) for x in t[2:]), []))
            else:
                sets[-1][2].append(_kat_cs_record(t) if colour else _kat_ls_record(t))
    return sets


def score_array(setup, anchor_width=8):
    """the _p entry points' score argument from a setup tuple of load_kat_scores: match, mismatch, a_open, a_ext, b_open, b_ext (, crossover, indel_taboo_len), and
    the anchor width behind them"""
    s = list(setup[2:])
    return (C.c_int * 9)(*([s[4], s[5], s[0], s[1], s[2], s[3]] + (s[6:8] if len(s) > 6 else [0, 0]) + [anchor_width]))


# RNA fixtures (tools/make_golden.py rna_cases): tag -> (colour space?, genome file, read files, oracle options, pairing)
RNA_CASES = {
    "rna_ls": (False, "rna_genome.fa.gz", ["rna_reads_ls.fa.gz"], None, None),
    "rna_ls_pairs": (False, "rna_genome.fa.gz", ["rna_pairs_1.fa.gz", "rna_pairs_2.fa.gz"], None, ("opp-in", 100, 500)),
    "rna_ls_last_dna": (False, "rna_genome_last_dna.fa.gz", ["rna_reads_ls.fa.gz"], None, None),
    "rna_cs": (True, "rna_genome.fa.gz", ["rna_reads_cs.fa.gz"], None, None),
    "rna_cs_fq": (True, "rna_genome.fa.gz", ["rna_reads_cs.fq.gz"], None, None),
    "rna_cs_last_dna": (True, "rna_genome_last_dna.fa.gz", ["rna_reads_cs.fa.gz"], None, None),
    "rna_cs_last_rna": (True, "rna_genome_last_rna.fa.gz", ["rna_reads_cs.fa.gz"], None, None),
    "rna_cs_ungapped": (True, "rna_genome.fa.gz", ["rna_reads_cs.fa.gz"], "local=1;ungapped=1", None),
}
_LS_CODE = {c: i for i, c in enumerate(b"ACGTUMRWSYKVHDBN")}


def read_fastx(name, colour=False):
    """names, n x L code matrix (colour space: primer letter code first, then colours, 15 for '.'), QUAL strings or None -- of a fixed-length FASTA/FASTQ fixture"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", name), "rb") as f:
        lines = [l for l in f.read().split(b"\n") if l]
    fq = lines[0][:1] == b"@"
    step = 4 if fq else 2
    names = [lines[i][1:] for i in range(0, len(lines), step)]
    seqs = [lines[i + 1] for i in range(0, len(lines), step)]
    quals = [lines[i + 3] for i in range(0, len(lines), step)] if fq else None
    if colour:
        codes = np.array([[_LS_CODE[s[0]]] + [c - 48 if 48 <= c <= 51 else 15 for c in s[1:]] for s in seqs], dtype=np.uint8)
    else:
        codes = np.array([[_LS_CODE[c] for c in s.upper()] for s in seqs], dtype=np.uint8)
    return names, codes, quals


def read_genome_fixture(name):
    """contig names and code arrays of a FASTA genome fixture"""
    with gzip.open(os.path.join(ROOT, "tests", "golden", name), "rb") as f:
        text = f.read()
    names, contigs = [], []
    for block in text.split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        names.append(head.strip())
        contigs.append(np.array([_LS_CODE[c] for c in body.replace(b"\n", b"").upper()], dtype=np.uint8))
    return names, contigs


def load_rna_case(tag):
    colour, gname, rfiles, opts, pairing = RNA_CASES[tag]
    cn, contigs = read_genome_fixture(gname)
    with gzip.open(os.path.join(ROOT, "tests", "golden", tag + ".sam.gz"), "rb") as f:
        sam = f.read()
    return dict(colour=colour, contig_names=cn, contigs=contigs, reads=[read_fastx(r, colour) for r in rfiles], files=rfiles, opts=opts, pairing=pairing, sam=sam)
