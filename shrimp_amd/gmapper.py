"""Python host mirror of the gmapper hot path on MI355X (ctypes over libgmapper_hip.so).

Mirrors the reference's call surface for this path (names, argument meaning, error behaviour):
    load_genome / genomemap globals   -> Index            (ref: gmapper/genome.c:1012-1182)
    sw_vector_setup / sw_vector       -> sw_vector_*      (ref: common/sw-vector.c:388-515)
    sw_full_ls_setup / sw_full_ls     -> sw_full_ls       (ref: common/sw-full-ls.c:568-683)
    handle_read + SAM emission        -> Session.map_reads (ref: gmapper/mapping.c:1773-1868, gmapper/output.c:227-774)
All compute happens in the HIP library; there is no Python/CPU fallback: importing works without
a GPU (so that symbol checks can run), every compute call fails loudly without one.
"""
from __future__ import annotations

import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GM_LIB_PATH") or os.path.join(_HERE, "libgmapper_hip.so")   # GM_LIB_PATH: an experimental build of the same ABI


class GmError(RuntimeError):
    pass


class Params(C.Structure):   # gm_params_t (include/gmapper_hip.h)
    _fields_ = [("match_score", C.c_int), ("mismatch_score", C.c_int),
                ("a_gap_open_score", C.c_int), ("a_gap_extend_score", C.c_int),
                ("b_gap_open_score", C.c_int), ("b_gap_extend_score", C.c_int),
                ("window_len", C.c_double), ("window_overlap", C.c_double), ("window_gen_threshold", C.c_double),
                ("sw_vect_threshold", C.c_double), ("sw_full_threshold", C.c_double),
                ("match_mode", C.c_int), ("num_outputs", C.c_int), ("num_tmp_outputs", C.c_int), ("anchor_width", C.c_int),
                ("region_bits", C.c_int), ("region_overlap", C.c_int), ("list_cutoff", C.c_uint32),
                ("hash_filter_calls", C.c_int), ("tiebreak_rev", C.c_int), ("sam_unaligned", C.c_int), ("longest_read_len", C.c_int),
                ("strata", C.c_int), ("max_alignments", C.c_int),
                ("colour_space", C.c_int), ("crossover_score", C.c_int), ("indel_taboo_len", C.c_int), ("pr_xover", C.c_double),
                ("local_alignment", C.c_int), ("ungapped", C.c_int), ("hash_seeds", C.c_int), ("output_format", C.c_int), ("print_read_seq", C.c_int), ("strand_only", C.c_int),
                ("single_best_mapping", C.c_int), ("all_contigs", C.c_int), ("no_mapping_qualities", C.c_int), ("no_improper_mappings", C.c_int),
                ("extra_sam_fields", C.c_int), ("sam_r2", C.c_int), ("read_group", C.c_char * 64),
                ("trim_front", C.c_int), ("trim_end", C.c_int), ("trim_first", C.c_int), ("trim_second", C.c_int), ("trim_illumina", C.c_int),
                ("min_avg_qv", C.c_int), ("ignore_qvs", C.c_int), ("no_qv_check", C.c_int)]


class MapStats(C.Structure):   # gm_map_stats_t
    _fields_ = [(n, C.c_uint64) for n in ("reads", "reads_matched", "sam_records", "lookups", "list_entries", "list_bytes",
                                          "survivors", "anchors", "windows", "vec_calls", "vec_cells", "vec_bypassed",
                                          "full_calls", "full_cells", "exact_order_reads", "retries", "survivors_pruned", "mp_unfiltered", "post_sw_host_redo")] + \
               [(n, C.c_double) for n in ("ms_lookup", "ms_anchors", "ms_pass1", "ms_select", "ms_pass2", "ms_host")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


PAIR_MODES = {"opp-in": 1, "opp-out": 2, "col-fw": 3, "col-bw": 4}   # ref: gmapper-definitions.h:42-46, -p option gmapper.c:1583-1600


class PairOpts(C.Structure):    # gm_pair_opts_t
    _fields_ = [("pair_mode", C.c_int), ("min_insert_size", C.c_int), ("max_insert_size", C.c_int),
                ("insert_size_mean", C.c_double), ("insert_size_stddev", C.c_double), ("half_paired", C.c_int), ("match_mode", C.c_int)]

    @staticmethod
    def default(mode="opp-in", min_insert=0, max_insert=1000):
        o = PairOpts(); lib().gm_pair_opts_default(C.byref(o))
        o.pair_mode = PAIR_MODES[mode] if isinstance(mode, str) else int(mode)
        o.min_insert_size = int(min_insert); o.max_insert_size = int(max_insert)
        return o


class MergeOptions(C.Structure):   # gm_merge_options_t (mergesam's options of the same names, ref: mergesam/mergesam.c:216-243)
    _fields_ = [(n, C.c_int) for n in ("max_outputs", "max_alignments", "strata", "half_paired", "sam_unaligned", "single_best", "all_contigs",
                                       "no_mapping_qualities", "leave_mapq", "no_improper_mappings", "min_mapq", "fastq", "threads", "output",
                                       "header_given")] + [("command_line", C.c_char_p)]


MERGE_OUT = {"sam": 0, "un": 1, "al": 2}


def merge_sam(reads_text: bytes, sam_texts, command_line=None, output="sam", **options) -> bytes:
    """mergesam (ref: mergesam/mergesam.c): SAM texts of several runs -> one, in the order of the reads text, mapping qualities recomputed from
    the Z fields.  options: the fields of gm_merge_options_t (max_outputs, strata, single_best, all_contigs, sam_unaligned, ...)."""
    L = lib(); o = MergeOptions(); L.gm_merge_options_default(C.byref(o))
    for k, v in options.items():
        if not hasattr(o, k):
            raise TypeError("merge_sam: unknown option %r" % k)
        setattr(o, k, int(v))
    o.output = MERGE_OUT[output] if isinstance(output, str) else int(output)
    if command_line is not None:
        o.command_line = command_line if isinstance(command_line, bytes) else command_line.encode()
    texts = [bytes(t) for t in sam_texts]
    arr = (C.c_char_p * len(texts))(*texts); lens = (C.c_size_t * len(texts))(*[len(t) for t in texts])
    out = C.c_void_p(); ol = C.c_size_t()
    _check(L.gm_merge_sam(C.byref(o), reads_text, len(reads_text), len(texts), arr, lens, C.byref(out), C.byref(ol)), "gm_merge_sam")
    res = C.string_at(out, ol.value) if out.value else b""
    if out.value: L.gm_free(out)
    return res


class Anchor(C.Structure):      # struct gm_anchor == the reference's struct anchor (gmapper-definitions.h:66-74)
    _fields_ = [("x", C.c_longlong), ("y", C.c_longlong), ("length", C.c_int), ("width", C.c_int),
                ("weight", C.c_int), ("cn", C.c_int), ("score", C.c_int)]


class SwFullResults(C.Structure):   # struct gm_sw_full_results == the reference's struct sw_full_results (sw-full-common.h:13-48)
    _fields_ = [(n, C.c_int) for n in ("read_start", "rmapped", "genome_start", "gmapped", "matches", "mismatches",
                                       "insertions", "deletions", "score", "posterior_score", "pct_posterior_score")] + \
               [("dbalign", C.c_void_p), ("qralign", C.c_void_p), ("qual", C.c_void_p), ("posterior", C.c_double), ("mqv", C.c_int)] + \
               [(n, C.c_double) for n in ("z0", "z1", "z2", "z3", "pr_top_random_at_location", "pr_missed_mp", "insert_size_denom")] + \
               [("crossovers", C.c_int), ("dup", C.c_bool), ("in_use", C.c_bool)]


class SwFullRec(C.Structure):       # gm_sw_full_rec_t: one alignment of gm_sw_full_ls_batch / gm_sw_full_cs_batch (checked against gm_abi_sizeof(4))
    _fields_ = [(n, C.c_int) for n in ("score", "read_start", "rmapped", "gmapped", "matches", "mismatches", "insertions", "deletions", "crossovers", "status")] + \
               [("genome_start", C.c_int64), ("ops_off", C.c_uint64), ("n_ops", C.c_uint32)]


class PostRec(C.Structure):         # gm_post_rec_t: one answer of gm_post_sw_batch (checked against gm_abi_sizeof(5))
    _fields_ = [("posterior", C.c_double), ("matches", C.c_int), ("mismatches", C.c_int), ("crossovers", C.c_int), ("status", C.c_int), ("by_host", C.c_int),
                ("qual_len", C.c_uint32), ("qual_off", C.c_uint64)]


class ReadWindow(C.Structure):      # gm_read_window_t: one candidate window of gm_read_windows (checked against gm_read_window_size())
    _fields_ = [("read", C.c_int32), ("st", C.c_int32), ("cn", C.c_int32), ("g_off", C.c_uint32), ("w_len", C.c_int32), ("score_window_gen", C.c_int32), ("matches", C.c_int32),
                ("ax", C.c_int32), ("ay", C.c_int32), ("alen", C.c_int32), ("awidth", C.c_int32), ("reserved", C.c_int32)]


class Pass1Hit(C.Structure):        # gm_pass1_hit_t: one selected hit of gm_select_pass1 (checked against gm_pass1_hit_size())
    _fields_ = [("read", C.c_int32), ("st", C.c_int32), ("win", C.c_int32), ("cn", C.c_int32), ("gen_st", C.c_int32), ("g_off", C.c_uint32), ("w_len", C.c_int32),
                ("score_vector", C.c_int32), ("pct_score_vector", C.c_int32), ("score_max", C.c_int32), ("matches", C.c_int32), ("score_window_gen", C.c_int32),
                ("ax", C.c_int32), ("ay", C.c_int32), ("alen", C.c_int32), ("awidth", C.c_int32)]


class Mapping(C.Structure):         # gm_mapping_t: one final mapping of gm_select_pass2 (checked against gm_mapping_size())
    _fields_ = [("read", C.c_int32), ("hit", C.c_int32), ("score_full", C.c_int32), ("pct_score_full", C.c_int32), ("mqv", C.c_int32), ("flags", C.c_int32),
                ("posterior", C.c_double), ("z0", C.c_double), ("z1", C.c_double)]


class SAM_INPUT(C.Structure):       # gm_sam_input_t: what gm_sam_records takes (checked against gm_sam_input_size())
    _fields_ = [("n_reads", C.c_int), ("read_len", C.c_int), ("reads_packed", C.c_void_p), ("initbp", C.c_void_p), ("names", C.c_char_p), ("seqs", C.c_char_p),
                ("quals", C.c_char_p), ("qual_delta", C.c_int), ("n_hits", C.c_uint64), ("hits", C.c_void_p), ("recs", C.c_void_p), ("score_vector", C.c_void_p),
                ("post", C.c_void_p), ("post_quals", C.c_char_p), ("post_quals_len", C.c_uint64), ("qralign", C.c_char_p), ("ops_len", C.c_uint64),
                ("cigar", C.c_char_p), ("cigar_off", C.c_void_p), ("edit", C.c_char_p), ("edit_off", C.c_void_p), ("n_maps", C.c_uint64), ("maps", C.c_void_p),
                ("map_off", C.c_void_p)]


class ReadMappingsResult(C.Structure):   # gm_read_mappings_t: what gm_read_mappings fills (checked against gm_read_mappings_size())
    _fields_ = [("n_reads", C.c_int32), ("has_edit", C.c_int32), ("n_hits", C.c_uint64), ("n_maps", C.c_uint64), ("cigar_len", C.c_uint64), ("edit_len", C.c_uint64),
                ("ops_len", C.c_uint64), ("hits", C.c_void_p), ("hit_off", C.c_void_p), ("score_vector", C.c_void_p), ("recs", C.c_void_p), ("maps", C.c_void_p),
                ("map_off", C.c_void_p), ("cigar", C.c_void_p), ("cigar_off", C.c_void_p), ("edit", C.c_void_p), ("edit_off", C.c_void_p), ("ops", C.c_void_p)]


class ReadMappingsCsResult(C.Structure):   # gm_read_mappings_cs_t: ReadMappingsResult's fields, then what colour space adds (checked against gm_read_mappings_cs_size())
    _fields_ = ReadMappingsResult._fields_ + [("post_quals_len", C.c_uint64), ("post", C.c_void_p), ("post_quals", C.c_void_p), ("qralign", C.c_void_p)]


class PairMapping(C.Structure):     # gm_pair_mapping_t: one paired mapping of gm_pair_mappings (checked against gm_pair_mapping_size())
    _fields_ = [("pair", C.c_int32), ("hit", C.c_int32 * 2), ("score", C.c_int32), ("pct_score", C.c_int32), ("key", C.c_int32), ("insert_size", C.c_int32),
                ("mapq", C.c_int32 * 2), ("as", C.c_int32 * 2), ("improper", C.c_int32), ("z", (C.c_double * 4) * 2)]


class PairMappingsResult(C.Structure):   # gm_pair_mappings_t: what gm_pair_mappings fills (checked against gm_pair_mappings_size())
    _fields_ = [("n_pairs", C.c_int32), ("has_edit", C.c_int32), ("n_hits", C.c_uint64 * 2), ("n_pmaps", C.c_uint64), ("n_umaps", C.c_uint64 * 2), ("cigar_len", C.c_uint64 * 2),
                ("edit_len", C.c_uint64 * 2), ("ops_len", C.c_uint64 * 2), ("hits", C.c_void_p * 2), ("hit_off", C.c_void_p * 2), ("hit_kind", C.c_void_p * 2),
                ("recs", C.c_void_p * 2), ("pmaps", C.c_void_p), ("pmap_off", C.c_void_p), ("umaps", C.c_void_p * 2), ("umap_off", C.c_void_p * 2), ("umap_z45", C.c_void_p * 2),
                ("cigar", C.c_void_p * 2), ("cigar_off", C.c_void_p * 2), ("edit", C.c_void_p * 2), ("edit_off", C.c_void_p * 2), ("ops", C.c_void_p * 2)]


SW_FULL_REC_DTYPE = np.dtype(SwFullRec)      # the structured numpy view of an array of them
POST_REC_DTYPE = np.dtype(PostRec)
ANCHOR_DTYPE = np.dtype(Anchor)
READ_WINDOW_DTYPE = np.dtype(ReadWindow)
PASS1_HIT_DTYPE = np.dtype(Pass1Hit)
MAPPING_DTYPE = np.dtype(Mapping)
PAIR_MAPPING_DTYPE = np.dtype(PairMapping)
# one row of ReadMappings.table(): a mapping as a SAM record states it
MAPPING_TABLE_DTYPE = np.dtype([("read", np.int32), ("contig", np.int32), ("strand", np.int32), ("pos", np.uint32), ("mapq", np.int32), ("as", np.int32), ("nm", np.int32),
                                ("hit", np.int32)])


def gm_mqv_on(p):
    """a session under these parameters runs post_sw / prints mapping qualities (neither local_alignment nor no_mapping_qualities)"""
    return not p.local_alignment and not p.no_mapping_qualities


def mapping_positions(hits, recs, contig_len, hit_index):
    """POS of the mappings on the hits `hit_index`, as gm_sam_records prints it (ref: gmapper/output.c:626-634): forward strand genome_start + 1; strand 1
    (contig_len - genome_start) - (rmapped - 1 - deletions + insertions); the low 32 bits, unsigned.  numpy only, no loop."""
    k = np.asarray(hit_index, dtype=np.int64)
    h, r = hits[k], recs[k]
    gs = r["genome_start"].astype(np.int64)
    fw = gs + 1
    rv = (np.asarray(contig_len, dtype=np.int64)[h["cn"]] - gs) - (r["rmapped"].astype(np.int64) - 1 - r["deletions"] + r["insertions"])
    return (np.where(h["gen_st"] == 0, fw, rv) & 0xFFFFFFFF).astype(np.uint32)


class ReadMappings:
    """What Session.read_mappings returns: the arrays of gm_read_mappings_t as numpy arrays of the existing dtypes.
    hits (PASS1_HIT_DTYPE), hit_off; score_vector (ZV of every hit); recs (SW_FULL_REC_DTYPE); maps (MAPPING_DTYPE), map_off; cigar_buf / cigar_off and, where the
    session prints them, edit_buf / edit_off; ops (want_ops only, else None).  cigar(i) / edit(i): the text of hit i (empty for a hit that is no mapping).  The object
    goes into Session.sam_records in place of its first array."""
    def __init__(self, hits, hit_off, score_vector, recs, maps, map_off, cigar_buf, cigar_off, edit_buf, edit_off, ops, contig_len):
        self.hits, self.hit_off, self.score_vector, self.recs, self.maps, self.map_off = hits, hit_off, score_vector, recs, maps, map_off
        self.cigar_buf, self.cigar_off, self.edit_buf, self.edit_off, self.ops, self.contig_len = cigar_buf, cigar_off, edit_buf, edit_off, ops, contig_len

    def cigar(self, i): return self.cigar_buf[int(self.cigar_off[i]):int(self.cigar_off[i + 1])]

    def edit(self, i):
        if self.edit_off is None: raise GmError("read_mappings: the session prints no edit strings (extra_sam_fields)")
        return self.edit_buf[int(self.edit_off[i]):int(self.edit_off[i + 1])]

    def table(self):
        """One MAPPING_TABLE_DTYPE row per mapping, in maps order: read, contig, strand, POS (1-based, as SAM prints it), MAPQ, AS, NM, hit"""
        m = self.maps; k = m["hit"].astype(np.int64)
        t = np.zeros(len(m), dtype=MAPPING_TABLE_DTYPE)
        if not len(m): return t
        h, r = self.hits[k], self.recs[k]
        t["read"], t["contig"], t["strand"], t["hit"] = m["read"], h["cn"], h["gen_st"], m["hit"]
        t["pos"] = mapping_positions(self.hits, self.recs, self.contig_len, k)
        t["mapq"], t["as"] = m["mqv"], m["score_full"]
        t["nm"] = r["mismatches"] + r["deletions"] + r["insertions"]
        return t


class ReadMappingsCs(ReadMappings):
    """What Session.read_mappings_cs returns: ReadMappings (score_vector: pass 1's score; clip "H") and what colour space adds -- post (POST_REC_DTYPE per hit, None
    where the session has no post_sw), post_quals (bytes; post[i]'s slice at qual_off, qual_len) and qralign (bytes, hit i's slice at recs[i].ops_off, n_ops).
    Session.sam_records picks the three from it."""
    def __init__(self, *base, post, post_quals, qralign):
        ReadMappings.__init__(self, *base)
        self.post, self.post_quals, self.qralign = post, post_quals, qralign

    def qralign_of(self, i):
        a = int(self.recs["ops_off"][i]); return self.qralign[a:a + int(self.recs["n_ops"][i])]

    def quals_of(self, i):
        if self.post is None: return b""
        a = int(self.post["qual_off"][i]); return self.post_quals[a:a + int(self.post["qual_len"][i])]


class PairMappings:
    """What Session.pair_mappings returns: the arrays of gm_pair_mappings_t as numpy arrays.  Per mate m (0 / 1), as lists of two: hits (PASS1_HIT_DTYPE), hit_off,
    hit_kind (0 a hit of the paired pass, 1 of the half-paired rescue), recs (SW_FULL_REC_DTYPE), umaps (MAPPING_DTYPE; hit: the index in hits[m]), umap_off, umap_z45
    ([n, 2]: the Z4 and Z5 values), cigar_buf / cigar_off, edit_buf / edit_off (None unless the session prints edit strings), ops (want_ops only, else None).  For the
    pair: pmaps (PAIR_MAPPING_DTYPE; hit[m]: the index within the pair's own slice of hits[m]), pmap_off."""
    def __init__(self, n_pairs, hits, hit_off, hit_kind, recs, pmaps, pmap_off, umaps, umap_off, umap_z45, cigar_buf, cigar_off, edit_buf, edit_off, ops, contig_len):
        self.n_pairs, self.hits, self.hit_off, self.hit_kind, self.recs, self.pmaps, self.pmap_off = n_pairs, hits, hit_off, hit_kind, recs, pmaps, pmap_off
        self.umaps, self.umap_off, self.umap_z45, self.cigar_buf, self.cigar_off, self.edit_buf, self.edit_off = umaps, umap_off, umap_z45, cigar_buf, cigar_off, edit_buf, edit_off
        self.ops, self.contig_len = ops, contig_len

    def cigar(self, m, i): return self.cigar_buf[m][int(self.cigar_off[m][i]):int(self.cigar_off[m][i + 1])]

    def edit(self, m, i):
        if self.edit_off[m] is None: raise GmError("pair_mappings: the session prints no edit strings (extra_sam_fields)")
        return self.edit_buf[m][int(self.edit_off[m][i]):int(self.edit_off[m][i + 1])]

    def pair_hit(self, m, k):
        """the index in hits[m] / recs[m] of mate m's hit of paired mapping k"""
        return int(self.hit_off[m][int(self.pmaps["pair"][k])]) + int(self.pmaps["hit"][k][m])

    def positions(self, m, hit_index):
        """POS of mate m's mappings on the hits `hit_index`, as the SAM records print it"""
        return mapping_positions(self.hits[m], self.recs[m], self.contig_len, hit_index)


# every entry point include/gmapper_hip.h declares
EXPORTS = ["gm_map_pairs_file", "gm_map_reads_file_cb", "gm_map_pairs_file_cb", "gm_preprocess_read_text", "gm_map_pairs_cs_fastq", "gm_map_reads_file", "gm_merge_options_default", "gm_merge_sam", "gm_release_cache", "gm_map_pairs_cs", "gm_last_error", "gm_device_count", "gm_params_default", "gm_params_default_cs", "gm_index_build", "gm_index_build_fasta", "gm_index_n_contigs", "gm_index_contig", "gm_sam_header", "gm_index_build_timing", "gm_index_free", "gm_index_list_cutoff",
           "gm_index_save", "gm_index_load", "gm_index_bytes", "gm_index_n_slabs", "gm_index_has_buckets", "gm_index_get_list", "gm_index_device_array", "gm_index_meta", "gm_index_alloc_like",
           "sw_vector_setup", "sw_vector", "sw_vector_stats", "sw_vector_cleanup", "gm_sw_vector_batch", "gm_sw_vector_batch_bounded",
           "sw_gapless_setup", "sw_gapless", "sw_gapless_stats", "gm_sw_gapless_batch",
           "sw_full_ls_setup", "sw_full_ls", "sw_full_ls_cleanup", "sw_full_ls_stats",
           "sw_full_cs_setup", "sw_full_cs", "sw_full_cs_cleanup", "sw_full_cs_stats", "gm_sw_vector_batch_cs",
           "gm_sw_full_ls_batch", "gm_sw_full_cs_batch", "gm_sw_full_batch_strings",
           "post_sw_setup", "post_sw", "post_sw_cleanup", "post_sw_stats", "gm_post_sw_batch", "gm_post_sw_batch_last_plan",
           "gm_index_genome_is_rna", "gm_index_get_windows", "gm_sw_vector_batch_ix", "gm_sw_vector_batch_bounded_ix", "gm_sw_gapless_batch_ix", "gm_sw_full_ls_batch_ix", "gm_sw_full_cs_batch_ix",
           "gm_post_sw_batch_ix", "gm_sw_full_batch_text", "gm_sw_full_batch_text_ix",
           "gm_session_create", "gm_session_free", "gm_sequence_to_bitfield", "gm_map_reads_text", "gm_map_reads", "gm_map_reads_fastq", "gm_map_reads_cs", "gm_map_reads_cs_fastq", "gm_map_reads_device", "gm_free", "gm_debug_tophits", "gm_debug_tophits_cs",
           "gm_read_windows", "gm_read_window_size", "gm_select_pass1", "gm_pass1_hit_size", "gm_select_pass2", "gm_mapping_size", "gm_score_windows", "gm_select_pass1_f1", "gm_read_hits", "gm_sam_records", "gm_sam_input_size", "gm_read_mappings", "gm_read_mappings_free", "gm_read_mappings_size",
           "gm_read_mappings_cs", "gm_read_mappings_cs_free", "gm_read_mappings_cs_size",
           "gm_pair_opts_default", "gm_map_pairs", "gm_map_pairs_fastq",
           "gm_pair_mappings", "gm_pair_mappings_free", "gm_pair_mappings_size", "gm_pair_mapping_size", "gm_debug_pair_select",
           "gm_last_lookup_timing", "gm_last_lookup_kernel", "gm_last_pass2_kernel", "gm_abi_sizeof"]

_lib = None


def lib():
    """The HIP library.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GmError(f"{LIB_PATH} is missing: build it with `make -C shrimp_amd/csrc` (or __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    u32p, vp = C.POINTER(C.c_uint32), C.c_void_p
    L.gm_last_error.restype = C.c_char_p
    L.gm_last_lookup_kernel.restype = C.c_char_p
    L.gm_last_pass2_kernel.restype = C.c_char_p
    L.gm_device_count.restype = C.c_int
    L.gm_params_default.argtypes = [C.POINTER(Params)]
    L.gm_params_default_cs.argtypes = [C.POINTER(Params)]
    L.gm_index_build.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(u32p), u32p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.POINTER(Params)]
    L.gm_index_build_fasta.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_char_p), C.POINTER(Params)]
    L.gm_index_n_contigs.argtypes = [vp]; L.gm_index_n_contigs.restype = C.c_int
    L.gm_index_contig.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), u32p]
    L.gm_sam_header.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.gm_index_build_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.gm_index_free.argtypes = [vp]
    L.gm_index_save.argtypes = [vp, C.c_char_p]
    L.gm_index_load.argtypes = [C.POINTER(vp), C.c_int, C.c_char_p, C.POINTER(Params)]
    L.gm_index_list_cutoff.argtypes = [vp]; L.gm_index_list_cutoff.restype = C.c_uint32
    L.gm_index_bytes.argtypes = [vp]; L.gm_index_bytes.restype = C.c_uint64
    L.gm_index_n_slabs.argtypes = [vp]; L.gm_index_n_slabs.restype = C.c_int
    L.gm_index_has_buckets.argtypes = [vp]; L.gm_index_has_buckets.restype = C.c_int
    L.gm_index_get_list.argtypes = [vp, C.c_int, C.c_uint32, u32p, u32p, C.c_uint32]
    L.gm_index_device_array.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.gm_index_meta.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    L.gm_index_alloc_like.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_uint64]
    L.sw_vector_setup.argtypes = [C.c_int] * 9 + [C.c_bool]
    L.sw_vector.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, u32p, C.c_int, C.c_bool]
    L.gm_sw_vector_batch.argtypes = [C.c_int, u32p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int), u32p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gm_sw_vector_batch_bounded.argtypes = [C.c_int, u32p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int), u32p, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int),
                                             C.POINTER(C.c_uint8)]
    L.sw_gapless_setup.argtypes = [C.c_int, C.c_int, C.c_bool]
    L.sw_gapless.argtypes = [u32p, C.c_int, u32p, C.c_int, C.c_int, C.c_int, u32p, C.c_int, C.c_bool]
    L.gm_sw_gapless_batch.argtypes = [C.c_int, u32p, u32p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int), u32p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.sw_full_ls_setup.argtypes = [C.c_int] * 8 + [C.c_bool, C.c_int]
    L.sw_full_ls.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.POINTER(SwFullResults), C.c_bool, C.POINTER(Anchor), C.c_int, C.c_int]
    L.sw_full_ls.restype = None
    L.sw_full_cs_setup.argtypes = [C.c_int] * 9 + [C.c_bool, C.c_int, C.c_int]
    L.sw_full_cs.argtypes = [u32p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_int, C.POINTER(SwFullResults), C.c_bool, C.c_bool, C.POINTER(Anchor), C.c_int, C.c_int, vp]
    L.sw_full_cs.restype = None
    L.gm_sw_vector_batch_cs.argtypes = [C.c_int, u32p, u32p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int), u32p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gm_sw_full_ls_batch.argtypes = [C.c_int, u32p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int), u32p, C.c_int, C.POINTER(C.c_int), vp, vp, C.POINTER(C.c_int), vp,
                                      C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.gm_sw_full_cs_batch.argtypes = [C.c_int, u32p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int), u32p, C.c_int, C.POINTER(C.c_int), vp, vp, vp, C.POINTER(C.c_int), vp,
                                      C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.gm_sw_full_batch_strings.argtypes = [C.c_int, vp, vp, C.c_uint64, u32p, C.c_uint64, u32p, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.post_sw_setup.argtypes = [C.c_int] + [C.c_double] * 6 + [C.c_bool, C.c_bool, C.c_int, C.c_int, C.c_bool]
    L.post_sw.argtypes = [u32p, C.c_int, C.c_char_p, C.POINTER(SwFullResults)]; L.post_sw.restype = None
    L.gm_post_sw_batch.argtypes = [C.c_int, vp, vp, C.c_uint64, u32p, C.c_uint64, u32p, C.c_int, C.POINTER(C.c_int), vp, vp, C.c_int, vp, C.POINTER(vp), C.POINTER(vp),
                                   C.POINTER(C.c_uint64)]
    L.gm_post_sw_batch_last_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    ipt, i64p, u8p = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    win = [vp, C.c_int, ipt, u8p, i64p, ipt]      # ix, n, cn, gen_st, g_off, glen
    L.gm_index_genome_is_rna.argtypes = [vp]
    L.gm_index_get_windows.argtypes = win + [C.c_int, u32p, C.c_int]
    L.gm_sw_vector_batch_ix.argtypes = win + [u32p, C.c_int, ipt, ipt, C.c_int, ipt]
    L.gm_sw_vector_batch_bounded_ix.argtypes = win + [u32p, C.c_int, ipt, C.c_int, ipt, u8p]
    L.gm_sw_gapless_batch_ix.argtypes = [vp, C.c_int, ipt, u8p, C.c_int, u32p, C.c_int, ipt, ipt, ipt, ipt, C.c_int, ipt]
    L.gm_sw_full_ls_batch_ix.argtypes = win + [u32p, C.c_int, ipt, vp, vp, ipt, vp, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.gm_sw_full_cs_batch_ix.argtypes = win + [u32p, C.c_int, ipt, vp, vp, vp, ipt, vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.gm_post_sw_batch_ix.argtypes = [vp, C.c_int, ipt, u8p, vp, vp, C.c_uint64, u32p, C.c_int, ipt, vp, vp, C.c_int, vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]
    text = [vp, vp, C.c_uint64]                                                              # recs, ops, ops_len
    text_tail = [u32p, C.c_int, ipt, vp, C.c_int, vp, vp, C.c_int, ipt, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.gm_sw_full_batch_text.argtypes = [C.c_int, C.c_int, C.c_int] + text + [u32p, C.c_uint64] + text_tail
    L.gm_sw_full_batch_text_ix.argtypes = [vp, C.c_int, C.c_int, C.c_int, ipt, u8p] + text + text_tail
    L.gm_abi_sizeof.argtypes = [C.c_int]; L.gm_abi_sizeof.restype = C.c_int
    L.gm_session_create.argtypes = [C.POINTER(vp), vp, C.POINTER(Params), C.c_int]
    L.gm_session_free.argtypes = [vp]
    L.gm_map_reads.argtypes = [vp, C.c_int, C.c_int, u32p, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_map_reads_fastq.argtypes = [vp, C.c_int, C.c_int, u32p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_map_reads_cs.argtypes = [vp, C.c_int, C.c_int, u32p, C.POINTER(C.c_uint8), C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_map_reads_cs_fastq.argtypes = [vp, C.c_int, C.c_int, u32p, C.POINTER(C.c_uint8), C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_map_reads_device.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_free.argtypes = [vp]
    L.gm_pair_opts_default.argtypes = [C.POINTER(PairOpts)]
    L.gm_map_pairs_fastq.argtypes = [vp, C.c_int, C.c_int, u32p, C.c_int, u32p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(PairOpts),
                                     C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_map_pairs.argtypes = [vp, C.c_int, C.c_int, u32p, C.c_int, u32p, C.c_char_p, C.c_char_p, C.POINTER(PairOpts),
                               C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_map_pairs_cs_fastq.argtypes = [vp, C.c_int, C.c_int, u32p, C.POINTER(C.c_uint8), C.c_int, u32p, C.POINTER(C.c_uint8), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int,
                                        C.POINTER(PairOpts), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_map_pairs_file.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(PairOpts), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_map_reads_file.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_merge_options_default.argtypes = [C.POINTER(MergeOptions)]
    L.gm_merge_sam.argtypes = [C.POINTER(MergeOptions), C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.gm_map_pairs_cs.argtypes = [vp, C.c_int, C.c_int, u32p, C.POINTER(C.c_uint8), C.c_int, u32p, C.POINTER(C.c_uint8), C.c_char_p, C.c_char_p, C.POINTER(PairOpts),
                                  C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(MapStats)]
    L.gm_debug_tophits.argtypes = [vp, C.c_int, C.c_int, u32p, C.POINTER(C.c_longlong), C.c_long, C.POINTER(C.c_long)]
    L.gm_debug_tophits_cs.argtypes = [vp, C.c_int, C.c_int, u32p, C.POINTER(C.c_uint8), C.POINTER(C.c_longlong), C.c_long, C.POINTER(C.c_long)]
    L.gm_last_lookup_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.gm_read_window_size.argtypes = []; L.gm_read_window_size.restype = C.c_int
    L.gm_read_windows.argtypes = [vp, C.c_int, C.c_int, u32p, u8p, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(MapStats)]
    if L.gm_read_window_size() != READ_WINDOW_DTYPE.itemsize:
        raise GmError("gm_read_window_t is %d bytes in the library, %d in READ_WINDOW_DTYPE" % (L.gm_read_window_size(), READ_WINDOW_DTYPE.itemsize))
    u64p = C.POINTER(C.c_uint64)
    L.gm_pass1_hit_size.argtypes = []; L.gm_pass1_hit_size.restype = C.c_int
    L.gm_mapping_size.argtypes = []; L.gm_mapping_size.restype = C.c_int
    L.gm_select_pass1.argtypes = [vp, C.c_int, C.c_int, vp, C.c_uint64, u64p, ipt, C.POINTER(vp), u64p, u64p]
    L.gm_select_pass2.argtypes = [vp, C.c_int, u64p, vp, vp, vp, C.POINTER(vp), u64p, u64p]
    L.gm_score_windows.argtypes = [vp, C.c_int, C.c_int, u32p, u8p, vp, C.c_uint64, u64p, ipt, u32p]
    L.gm_select_pass1_f1.argtypes = [vp, C.c_int, C.c_int, vp, C.c_uint64, u64p, ipt, u32p, C.POINTER(vp), u64p, u64p, u64p]
    L.gm_read_hits.argtypes = [vp, C.c_int, C.c_int, u32p, u8p, C.POINTER(vp), u64p, u64p, C.POINTER(vp), u64p, u64p, C.POINTER(vp), C.POINTER(MapStats)]
    for fn, dt, what in ((L.gm_pass1_hit_size, PASS1_HIT_DTYPE, "gm_pass1_hit_t"), (L.gm_mapping_size, MAPPING_DTYPE, "gm_mapping_t")):
        if fn() != dt.itemsize:
            raise GmError("%s is %d bytes in the library, %d in its numpy dtype" % (what, fn(), dt.itemsize))
    L.gm_sam_input_size.argtypes = []; L.gm_sam_input_size.restype = C.c_int
    L.gm_sam_records.argtypes = [vp, C.POINTER(SAM_INPUT), C.POINTER(vp), C.POINTER(C.c_size_t), u64p]
    if L.gm_sam_input_size() != C.sizeof(SAM_INPUT):
        raise GmError("gm_sam_input_t is %d bytes in the library, %d in SAM_INPUT" % (L.gm_sam_input_size(), C.sizeof(SAM_INPUT)))
    L.gm_read_mappings_size.argtypes = []; L.gm_read_mappings_size.restype = C.c_int
    L.gm_read_mappings.argtypes = [vp, C.c_int, C.c_int, u32p, u8p, C.c_int, C.POINTER(ReadMappingsResult), C.POINTER(MapStats)]
    L.gm_read_mappings_free.argtypes = [C.POINTER(ReadMappingsResult)]; L.gm_read_mappings_free.restype = None
    if L.gm_read_mappings_size() != C.sizeof(ReadMappingsResult):
        raise GmError("gm_read_mappings_t is %d bytes in the library, %d in ReadMappingsResult" % (L.gm_read_mappings_size(), C.sizeof(ReadMappingsResult)))
    L.gm_pair_mapping_size.argtypes = []; L.gm_pair_mapping_size.restype = C.c_int
    L.gm_pair_mappings_size.argtypes = []; L.gm_pair_mappings_size.restype = C.c_int
    L.gm_pair_mappings.argtypes = [vp, C.c_int, C.c_int, u32p, C.c_int, u32p, C.POINTER(PairOpts), C.c_int, C.POINTER(PairMappingsResult), C.POINTER(MapStats)]
    L.gm_pair_mappings_free.argtypes = [C.POINTER(PairMappingsResult)]; L.gm_pair_mappings_free.restype = None
    L.gm_debug_pair_select.argtypes = [vp, C.c_int, C.c_int, u32p, C.POINTER(C.c_int32), u32p, C.POINTER(C.c_int32), u32p, u32p, u32p, u32p, u32p, u32p]
    for fn, size, what in ((L.gm_pair_mapping_size, PAIR_MAPPING_DTYPE.itemsize, "gm_pair_mapping_t"), (L.gm_pair_mappings_size, C.sizeof(PairMappingsResult), "gm_pair_mappings_t")):
        if fn() != size:
            raise GmError("%s is %d bytes in the library, %d in its Python mirror" % (what, fn(), size))
    L.gm_read_mappings_cs_size.argtypes = []; L.gm_read_mappings_cs_size.restype = C.c_int
    L.gm_read_mappings_cs.argtypes = [vp, C.c_int, C.c_int, u32p, u8p, C.c_char_p, C.c_int, C.c_int, C.POINTER(ReadMappingsCsResult), C.POINTER(MapStats)]
    L.gm_read_mappings_cs_free.argtypes = [C.POINTER(ReadMappingsCsResult)]; L.gm_read_mappings_cs_free.restype = None
    if L.gm_read_mappings_cs_size() != C.sizeof(ReadMappingsCsResult):
        raise GmError("gm_read_mappings_cs_t is %d bytes in the library, %d in ReadMappingsCsResult" % (L.gm_read_mappings_cs_size(), C.sizeof(ReadMappingsCsResult)))
    _lib = L
    return L


def _check(rc, what):
    if rc != 0:
        raise GmError(f"{what} failed ({rc}): {lib().gm_last_error().decode()}")


def default_params() -> Params:
    p = Params()
    lib().gm_params_default(C.byref(p))
    return p


def default_params_cs() -> Params:
    """the gmapper-cs binary's defaults (colour space; ref: gmapper.c:1748-1755)"""
    p = Params()
    lib().gm_params_default_cs(C.byref(p))
    return p


def pack_codes(codes: np.ndarray) -> np.ndarray:
    """4-bit codes -> the reference's bitfield (8 bases per uint32; ref: common/util.h:41)."""
    from .synth import pack_nibbles
    return pack_nibbles(np.asarray(codes, dtype=np.uint8))


class Index:
    """Device-resident seed index + genome (the reference's genomemap/genome_contigs globals)."""

    def __init__(self, contigs, names=None, seeds=None, params: Params | None = None, device: int = 0):
        L = lib()
        self.params = params or default_params()
        self._packed = [np.ascontiguousarray(pack_codes(c)) for c in contigs]
        n = len(contigs)
        self.contig_len = [int(len(c)) for c in contigs]
        ptrs = (C.POINTER(C.c_uint32) * n)(*[p.ctypes.data_as(C.POINTER(C.c_uint32)) for p in self._packed])
        lens = (C.c_uint32 * n)(*self.contig_len)
        cn = None
        if names is not None:
            cn = (C.c_char_p * n)(*[s.encode() if isinstance(s, str) else s for s in names])
        sd = None
        ns = 0
        if seeds:
            ns = len(seeds); sd = (C.c_char_p * ns)(*[s.encode() for s in seeds])
        self.h = C.c_void_p()
        _check(L.gm_index_build(C.byref(self.h), device, n, ptrs, lens, cn, ns, sd, C.byref(self.params)), "gm_index_build")
        self.device = device

    @classmethod
    def load(cls, prefix: str, params: "Params | None" = None, device: int = 0) -> "Index":
        """the reference's -L: <prefix>.genome + <prefix>.seed.<n> as written by stock gmapper -S (or by save())"""
        self = cls.__new__(cls)
        self.params = params or default_params()
        self.h = C.c_void_p(); self.device = device; self._packed = []; self.contig_len = []
        _check(lib().gm_index_load(C.byref(self.h), device, prefix.encode(), C.byref(self.params)), "gm_index_load")
        return self

    @classmethod
    def from_fasta(cls, paths, seeds=None, params: "Params | None" = None, device: int = 0) -> "Index":
        """load_genome(files, nfiles): the genome FASTA files (plain or gzip, in this order) packed on the device and indexed"""
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        self = cls.__new__(cls)
        self.params = params or default_params()
        self.h = C.c_void_p(); self.device = device; self._packed = []; self.contig_len = []
        ps = [os.fsencode(p) for p in paths]
        arr = (C.c_char_p * len(ps))(*ps)
        sd = None; ns = 0
        if seeds:
            ns = len(seeds); sd = (C.c_char_p * ns)(*[s.encode() for s in seeds])
        _check(lib().gm_index_build_fasta(C.byref(self.h), device, len(ps), arr, ns, sd, C.byref(self.params)), "gm_index_build_fasta")
        self.contig_len = [n for _, n in self.contigs()]
        return self

    def contigs(self):
        """[(name, length)] of the index's contigs"""
        L = lib(); out = []
        for c in range(L.gm_index_n_contigs(self.h)):
            nm = C.c_char_p(); ln = C.c_uint32()
            _check(L.gm_index_contig(self.h, c, C.byref(nm), C.byref(ln)), "gm_index_contig")
            out.append((nm.value, ln.value))
        return out

    def sam_header(self, rg_id=None, rg_sample=None, command_line=None) -> bytes:
        """the header gmapper prints before its records: @HD, one @SQ per contig, @RG when rg_id is given, @PG when command_line is given"""
        L = lib(); out = C.c_void_p(); n = C.c_size_t()
        enc = lambda x: None if x is None else (x if isinstance(x, bytes) else str(x).encode())
        _check(L.gm_sam_header(self.h, enc(rg_id), enc(rg_sample), enc(command_line), C.byref(out), C.byref(n)), "gm_sam_header")
        text = C.string_at(out, n.value)
        L.gm_free(out)
        return text

    def save(self, prefix: str) -> None:
        """the reference's -S: files stock gmapper can load with -L"""
        _check(lib().gm_index_save(self.h, prefix.encode()), "gm_index_save")

    @property
    def list_cutoff(self): return lib().gm_index_list_cutoff(self.h)
    @property
    def nbytes(self): return lib().gm_index_bytes(self.h)
    @property
    def n_slabs(self): return lib().gm_index_n_slabs(self.h)
    @property
    def has_buckets(self): return bool(lib().gm_index_has_buckets(self.h))

    def get_list(self, sn: int, mapidx: int) -> np.ndarray:
        L = lib(); n = C.c_uint32()
        _check(L.gm_index_get_list(self.h, sn, mapidx, C.byref(n), None, 0), "gm_index_get_list")
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            _check(L.gm_index_get_list(self.h, sn, mapidx, C.byref(n), out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value), "gm_index_get_list")
        return out

    def device_arrays(self):
        """(device pointer, nbytes) of every resident array, for the start-up broadcast."""
        L = lib(); out = []
        kind = 0
        while True:
            p = C.c_void_p(); b = C.c_uint64()
            if L.gm_index_device_array(self.h, kind, C.byref(p), C.byref(b)) != 0:
                break
            out.append((p.value, b.value)); kind += 1
        return out

    def meta(self) -> bytes:
        L = lib(); nb = C.c_uint64(0)
        L.gm_index_meta(self.h, None, C.byref(nb))
        buf = C.create_string_buffer(nb.value)
        L.gm_index_meta(self.h, buf, C.byref(nb))
        return buf.raw

    @classmethod
    def alloc_like(cls, meta: bytes, device: int = 0) -> "Index":
        self = cls.__new__(cls)
        self.h = C.c_void_p(); self.device = device; self.params = default_params()
        _check(lib().gm_index_alloc_like(C.byref(self.h), device, meta, len(meta)), "gm_index_alloc_like")
        return self

    # ---- the batch seams on the resident genome (gm_*_ix): window i = glen[i] positions from offset g_off[i] of contig cn[i] on strand gen_st[i] ----
    def contig_lengths(self) -> np.ndarray:
        return np.array([ln for _, ln in self.contigs()], dtype=np.int64)

    @staticmethod
    def strand_offset(clen, g_off, glen):
        """the offset of a window on the other strand of its contig: forward offset <-> offset on the reverse-complement contig (its own inverse)"""
        return np.asarray(clen, dtype=np.int64) - np.asarray(g_off, dtype=np.int64) - np.asarray(glen, dtype=np.int64)

    @staticmethod
    def _win(cn, gen_st, g_off=None, glen=None):
        c = np.ascontiguousarray(cn, dtype=np.int32); n = c.shape[0]
        st = np.ascontiguousarray(gen_st, dtype=np.uint8)
        go = None if g_off is None else np.ascontiguousarray(g_off, dtype=np.int64); gn = None if glen is None else np.ascontiguousarray(glen, dtype=np.int32)
        if any(a is not None and a.shape != (n,) for a in (st, go, gn)): raise GmError("cn, gen_st, g_off, glen have n entries each")
        ipt, i64p, u8p = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        args = [c.ctypes.data_as(ipt), st.ctypes.data_as(u8p)]
        if go is not None: args += [go.ctypes.data_as(i64p), gn.ctypes.data_as(ipt)]
        return n, args, (c, st, go, gn)

    @staticmethod
    def _reads(reads_words, n):
        r = np.ascontiguousarray(reads_words, dtype=np.uint32)
        if r.ndim != 2 or r.shape[0] != n: raise GmError("reads_words is (n, read_words)")
        return r

    def get_windows(self, cn, gen_st, g_off, glen, colours=False) -> np.ndarray:
        """gm_index_get_windows: (n, stride) uint32 -- window i as a bitfield of its own (position 0 in nibble 0): letters, or the colour translation of the strand's contig"""
        n, wargs, keep = self._win(cn, gen_st, g_off, glen)
        stride = max(1, (int(keep[3].max()) + 7) // 8) if n else 1
        out = np.zeros((n, stride), dtype=np.uint32)
        _check(lib().gm_index_get_windows(self.h, n, *wargs, 1 if colours else 0, out.ctypes.data_as(C.POINTER(C.c_uint32)), stride), "gm_index_get_windows")
        return out

    def sw_vector_batch(self, cn, gen_st, g_off, glen, reads_words, rlen, initbp=None, is_rna=-1) -> np.ndarray:
        """gm_sw_vector_batch_ix (letter or colour space as sw_vector_setup's use_colours chose; colour space: initbp per read)"""
        n, wargs, keep = self._win(cn, gen_st, g_off, glen)
        r = self._reads(reads_words, n); rl = np.ascontiguousarray(rlen, dtype=np.int32)
        ib = None if initbp is None else np.ascontiguousarray(initbp, dtype=np.int32)
        out = np.zeros(n, dtype=np.int32); ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
        _check(lib().gm_sw_vector_batch_ix(self.h, n, *wargs, r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[1], ip(rl), ip(ib), int(is_rna), ip(out)), "gm_sw_vector_batch_ix")
        return out

    def sw_vector_batch_bounded(self, cn, gen_st, g_off, glen, reads_words, rlen, threshold: int):
        """gm_sw_vector_batch_bounded_ix: (scores, stopped) as the module-level sw_vector_batch_bounded"""
        n, wargs, keep = self._win(cn, gen_st, g_off, glen)
        r = self._reads(reads_words, n); rl = np.ascontiguousarray(rlen, dtype=np.int32)
        out = np.zeros(n, dtype=np.int32); stopped = np.zeros(n, dtype=np.uint8); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _check(lib().gm_sw_vector_batch_bounded_ix(self.h, n, *wargs, r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[1], ip(rl), int(threshold), ip(out),
                                                   stopped.ctypes.data_as(C.POINTER(C.c_uint8))), "gm_sw_vector_batch_bounded_ix")
        return out, stopped

    def sw_gapless_batch(self, cn, gen_st, reads_words, rlen, g_idx, r_idx, initbp=None, colour_space=False, is_rna=-1) -> np.ndarray:
        """gm_sw_gapless_batch_ix: the ungapped filter against the whole contig of the strand; g_idx is a position of that strand's contig"""
        n, wargs, keep = self._win(cn, gen_st)
        r = self._reads(reads_words, n)
        rl, gi, ri = (np.ascontiguousarray(a, dtype=np.int32) for a in (rlen, g_idx, r_idx))
        ib = None if initbp is None else np.ascontiguousarray(initbp, dtype=np.int32)
        out = np.zeros(n, dtype=np.int32); ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
        _check(lib().gm_sw_gapless_batch_ix(self.h, n, *wargs, 1 if colour_space else 0, r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[1], ip(rl), ip(gi), ip(ri), ip(ib),
                                            int(is_rna), ip(out)), "gm_sw_gapless_batch_ix")
        return out

    def _full_finish(self, colour, recs, ops_p, ops_len, keep, r, rl, initbp, is_rna):
        ops = np.ctypeslib.as_array(C.cast(ops_p, C.POINTER(C.c_uint8)), shape=(ops_len.value,)).copy() if ops_len.value else np.zeros(0, dtype=np.uint8)
        lib().gm_free(ops_p)
        c, st, go, gn = keep
        wins = {}
        def strings(i):      # item i's window fetched from the index (one small call; strings.prefetch() fetches those of all items in one), the record moved onto it
            w = wins["all"][i] if "all" in wins else self.get_windows(c[i:i + 1], st[i:i + 1], go[i:i + 1], gn[i:i + 1])[0]
            rna = (colour and self.genome_is_rna()) if is_rna < 0 else bool(is_rna)
            rec = recs[i].copy(); rec["genome_start"] -= go[i]
            return sw_full_batch_strings(colour, rec, ops, w, r[i], 0 if initbp is None else int(initbp[i]), rna, rlen=int(rl[i]))
        def prefetch():
            ok = recs["status"] == 0                                     # (a refused item may have no window to fetch)
            if "all" not in wins and ok.any():
                got = self.get_windows(c[ok], st[ok], go[ok], gn[ok]); full = np.zeros((len(recs), got.shape[1]), dtype=np.uint32); full[ok] = got; wins["all"] = full
        strings.prefetch = prefetch
        return recs, ops, strings

    def genome_is_rna(self) -> bool:
        """gm_index_genome_is_rna: the flag of the last contig, what is_rna = -1 stands for in the _ix entries"""
        rc = lib().gm_index_genome_is_rna(self.h)
        if rc < 0: _check(rc, "gm_index_genome_is_rna")
        return bool(rc)

    def sw_full_ls_batch(self, cn, gen_st, g_off, glen, reads_words, rlen, anchors=None, revcmpl=None, threshscore=None, maxscore=None, local_alignment=False):
        """gm_sw_full_ls_batch_ix: (records, ops, strings) as the module-level sw_full_ls_batch; genome_start is counted on the strand's contig.  strings(i) fetches
        item i's window with one gm_index_get_windows call; a caller who wants the strings of many items calls strings.prefetch() first (one call for all windows)."""
        n, wargs, keep = self._win(cn, gen_st, g_off, glen)
        r = self._reads(reads_words, n); rl = np.ascontiguousarray(rlen, dtype=np.int32)
        th = np.ascontiguousarray(threshscore if threshscore is not None else np.zeros(n), dtype=np.int32)
        mx = None if maxscore is None else np.ascontiguousarray(maxscore, dtype=np.int32)
        rv = None if revcmpl is None else np.ascontiguousarray(revcmpl, dtype=np.uint8)
        an = None if anchors is None else _anchor_array(anchors, n)
        recs = np.zeros(n, dtype=SW_FULL_REC_DTYPE); ops_p = C.c_void_p(); ops_len = C.c_uint64(0)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)); dp = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        _check(lib().gm_sw_full_ls_batch_ix(self.h, n, *wargs, r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[1], ip(rl), dp(an), dp(rv), ip(th), dp(mx),
                                            1 if local_alignment else 0, dp(recs), C.byref(ops_p), C.byref(ops_len)), "gm_sw_full_ls_batch_ix")
        return self._full_finish(False, recs, ops_p, ops_len, keep, r, rl, None, 0)

    def sw_full_cs_batch(self, cn, gen_st, g_off, glen, reads_words, rlen, initbp, anchors, revcmpl=None, threshscore=None, xover=None, is_rna=-1, local_alignment=False):
        """gm_sw_full_cs_batch_ix: (records, ops, strings) as the module-level sw_full_cs_batch"""
        n, wargs, keep = self._win(cn, gen_st, g_off, glen)
        r = self._reads(reads_words, n); rl = np.ascontiguousarray(rlen, dtype=np.int32)
        ib = np.ascontiguousarray(initbp, dtype=np.uint8)
        th = np.ascontiguousarray(threshscore if threshscore is not None else np.zeros(n), dtype=np.int32)
        rv = None if revcmpl is None else np.ascontiguousarray(revcmpl, dtype=np.uint8)
        an = _anchor_array(anchors, n)
        xs = None if xover is None else np.ascontiguousarray(xover, dtype=np.int32)
        if xs is not None and (xs.ndim != 2 or xs.shape[0] != n): raise GmError("sw_full_cs_batch: xover is (n, row length)")
        recs = np.zeros(n, dtype=SW_FULL_REC_DTYPE); ops_p = C.c_void_p(); ops_len = C.c_uint64(0)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)); dp = lambda a: None if a is None or a.size == 0 else a.ctypes.data
        _check(lib().gm_sw_full_cs_batch_ix(self.h, n, *wargs, r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[1], ip(rl), dp(ib), dp(an), dp(rv), ip(th), dp(xs),
                                            0 if xs is None else xs.shape[1], int(is_rna), 1 if local_alignment else 0, dp(recs), C.byref(ops_p), C.byref(ops_len)),
               "gm_sw_full_cs_batch_ix")
        return self._full_finish(True, recs, ops_p, ops_len, keep, r, rl, ib, int(is_rna))

    def post_sw_batch(self, cn, gen_st, recs, ops, reads_words, rlen, initbp, quals=None, is_rna=-1):
        """gm_post_sw_batch_ix: (post, qralign, qual) as the module-level post_sw_batch, on the records of Index.sw_full_cs_batch"""
        n, wargs, keep = self._win(cn, gen_st)
        rc_ = np.ascontiguousarray(recs, dtype=SW_FULL_REC_DTYPE); o = np.ascontiguousarray(ops, dtype=np.uint8)
        r = self._reads(reads_words, n)
        rl = np.ascontiguousarray(rlen, dtype=np.int32); ib = np.ascontiguousarray(initbp, dtype=np.uint8)
        if rc_.shape[0] != n or rl.shape[0] != n or ib.shape[0] != n or (quals is not None and len(quals) != n): raise GmError("post_sw_batch: every per-item array has n entries")
        qp = None if quals is None else (C.c_char_p * max(n, 1))(*[None if q is None else (q if isinstance(q, bytes) else q.encode()) for q in quals])
        post = np.zeros(n, dtype=POST_REC_DTYPE); qa_p, qo_p, qo_len = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        dp = lambda a: None if a.size == 0 else a.ctypes.data
        _check(lib().gm_post_sw_batch_ix(self.h, n, *wargs, dp(rc_), dp(o), o.size, r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[1], rl.ctypes.data_as(C.POINTER(C.c_int)),
                                         dp(ib), qp, int(is_rna), dp(post), C.byref(qa_p), C.byref(qo_p), C.byref(qo_len)), "gm_post_sw_batch_ix")
        qa = C.string_at(qa_p.value, o.size) if qa_p.value else b""
        qo = C.string_at(qo_p.value, qo_len.value) if qo_p.value else b""
        lib().gm_free(qa_p); lib().gm_free(qo_p)
        def qralign(i):
            return qa[int(rc_[i]["ops_off"]):int(rc_[i]["ops_off"]) + int(rc_[i]["n_ops"])].decode() if post[i]["status"] == 0 and rc_[i]["score"] > 0 else None
        def qual(i):
            return qo[int(post[i]["qual_off"]):int(post[i]["qual_off"]) + int(post[i]["qual_len"])].decode()
        qralign.buffer = qa                                                  # the whole buffer (ops.size bytes): what sw_full_batch_text takes as qralign
        qual.buffer = qo                                                     # ... and the base qualities end to end: what sam_records takes as post_quals
        return post, qralign, qual

    def sw_full_batch_text(self, cn, gen_st, recs, ops, reads_words, rlen, initbp=None, is_rna=-1, qralign=None, reverse=None, clip="S", what=("align", "cigar", "edit"),
                           colour_space=None):
        """gm_sw_full_batch_text_ix: (status, dbalign, qralign, cigar, edit) as the module-level sw_full_batch_text, on the records of Index.sw_full_ls_batch /
        sw_full_cs_batch with the cn / gen_st they were given.  colour_space: default -- colour space iff initbp is given."""
        n, wargs, keep = self._win(cn, gen_st)
        colour = (initbp is not None) if colour_space is None else bool(colour_space)
        return _batch_text(lambda *a: lib().gm_sw_full_batch_text_ix(self.h, *a[:3], *wargs, *a[3:]), "gm_sw_full_batch_text_ix", colour, n, recs, ops, [],
                           reads_words, rlen, initbp, int(is_rna), qralign, reverse, clip, what)

    def close(self):
        if getattr(self, "h", None):
            lib().gm_index_free(self.h); self.h = None

    def __del__(self):
        try: self.close()
        except Exception: pass


class Session:
    """One mapping stream on one GPU (the reference's per-thread state)."""

    def __init__(self, index: Index, params: Params | None = None, max_batch_reads: int = 131072):
        self.index = index
        self.h = C.c_void_p()
        self.params = params or index.params
        _check(lib().gm_session_create(C.byref(self.h), index.h, C.byref(self.params), max_batch_reads), "gm_session_create")
        self.stats = None

    def map_reads(self, reads_codes: np.ndarray, names=None) -> bytes:
        """reads_codes: [n, L] uint8 4-bit codes -> SAM records (bytes), input order."""
        from .synth import pack_reads
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        n, Lr = reads_codes.shape
        packed = np.ascontiguousarray(pack_reads(reads_codes))
        return self.map_packed(packed, n, Lr, names)

    def map_reads_fastq(self, reads_codes: np.ndarray, quals, qual_delta: int = 64, names=None) -> bytes:
        """FASTQ reads: quals = one QUAL string (bytes) per read, as in the file; qual_delta = the file's offset (--qv-offset)."""
        from .synth import pack_reads
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        n, Lr = reads_codes.shape
        packed = np.ascontiguousarray(pack_reads(reads_codes))
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        nm = None if names is None else b"\n".join(x if isinstance(x, bytes) else x.encode() for x in names)
        _check(L.gm_map_reads_fastq(self.h, n, Lr, packed.ctypes.data_as(C.POINTER(C.c_uint32)), nm, b"\n".join(quals), int(qual_delta),
                                    C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads_fastq")
        out = C.string_at(sam, sl.value) if sam.value else b""
        L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_reads_cs_fastq(self, reads_codes: np.ndarray, quals, qual_delta: int = 33, names=None) -> bytes:
        """csfastq reads: reads_codes as for map_reads_cs; quals = one QV string (bytes, one character per colour) per read."""
        from .synth import pack_reads
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        n, L1 = reads_codes.shape
        initbp = np.ascontiguousarray(reads_codes[:, 0])
        packed = np.ascontiguousarray(pack_reads(np.ascontiguousarray(reads_codes[:, 1:])))
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        nm = None if names is None else b"\n".join(x if isinstance(x, bytes) else x.encode() for x in names)
        _check(L.gm_map_reads_cs_fastq(self.h, n, L1 - 1, packed.ctypes.data_as(C.POINTER(C.c_uint32)), initbp.ctypes.data_as(C.POINTER(C.c_uint8)), nm,
                                       b"\n".join(quals), int(qual_delta), C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads_cs_fastq")
        out = C.string_at(sam, sl.value) if sam.value else b""
        L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_reads_cs(self, reads_codes: np.ndarray, names=None) -> bytes:
        """Colour-space reads: reads_codes [n, 1 + colours] uint8, column 0 the primer letter code (A0 C1 G2 T3), then colours
        (0-3, 15 = skipped cycle) -- csfasta without the text.  Needs an index / session made with default_params_cs()."""
        from .synth import pack_reads
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        n, L1 = reads_codes.shape
        initbp = np.ascontiguousarray(reads_codes[:, 0])
        packed = np.ascontiguousarray(pack_reads(np.ascontiguousarray(reads_codes[:, 1:])))
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        nm = None
        if names is not None:
            nm = b"\n".join(x if isinstance(x, bytes) else x.encode() for x in names)
        _check(L.gm_map_reads_cs(self.h, n, L1 - 1, packed.ctypes.data_as(C.POINTER(C.c_uint32)), initbp.ctypes.data_as(C.POINTER(C.c_uint8)), nm,
                                 C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads_cs")
        out = C.string_at(sam, sl.value) if sam.value else b""
        L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_reads_file(self, path, fastq=-1, qual_delta=None) -> bytes:
        """A reads file as the reference's reader takes it: FASTA / FASTQ, plain or gzip, any mix of read lengths (gm_map_reads_file)."""
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        qd = qual_delta if qual_delta is not None else (33 if self.params.colour_space else 64)      # gmapper-defaults.h:41-42
        _check(L.gm_map_reads_file(self.h, os.fsencode(path), int(fastq), int(qd), C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads_file")
        out = C.string_at(sam, sl.value) if sam.value else b""
        if sam.value: L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_reads_file_chunks(self, path, chunk_reads=0, fastq=-1, qual_delta=None, collect=True):
        """gm_map_reads_file_cb: the file in chunks of at most chunk_reads reads; returns the list of texts the write function received (one per chunk; with
        collect=False their lengths only: the form a timed loop uses)."""
        L = lib(); st = MapStats(); parts = []
        qd = qual_delta if qual_delta is not None else (33 if self.params.colour_space else 64)
        WRITE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
        cb = WRITE((lambda ctx, p, n: (parts.append(C.string_at(p, n)), 0)[1]) if collect else (lambda ctx, p, n: (parts.append(n), 0)[1]))
        _check(L.gm_map_reads_file_cb(self.h, os.fsencode(path), int(fastq), int(qd), C.c_size_t(int(chunk_reads)), cb, None, C.byref(st)), "gm_map_reads_file_cb")
        self.stats = st.as_dict()
        return parts

    def map_pairs_file_chunks(self, path1, path2=None, chunk_pairs=0, fastq=-1, qual_delta=None, mode="opp-in", min_insert=0, max_insert=1000, opts: "PairOpts | None" = None):
        """gm_map_pairs_file_cb: at most chunk_pairs pairs at a time; returns the texts the write function received."""
        L = lib(); st = MapStats(); parts = []
        qd = qual_delta if qual_delta is not None else (33 if self.params.colour_space else 64)
        o = opts if opts is not None else PairOpts.default(mode, min_insert, max_insert)
        WRITE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
        cb = WRITE(lambda ctx, p, n: (parts.append(C.string_at(p, n)), 0)[1])
        _check(L.gm_map_pairs_file_cb(self.h, os.fsencode(path1), None if path2 is None else os.fsencode(path2), int(fastq), int(qd), C.byref(o), C.c_size_t(int(chunk_pairs)),
                                      cb, None, C.byref(st)), "gm_map_pairs_file_cb")
        self.stats = st.as_dict()
        return parts

    def map_pairs_file(self, path1, path2=None, fastq=-1, qual_delta=None, mode="opp-in", min_insert=0, max_insert=1000, opts: "PairOpts | None" = None) -> bytes:
        """Pairs from one file (mates adjacent) or two (-1 / -2): FASTA / FASTQ, plain or gzip, any mix of lengths (gm_map_pairs_file)."""
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        qd = qual_delta if qual_delta is not None else (33 if self.params.colour_space else 64)
        o = opts if opts is not None else PairOpts.default(mode, min_insert, max_insert)
        _check(L.gm_map_pairs_file(self.h, os.fsencode(path1), None if path2 is None else os.fsencode(path2), int(fastq), int(qd), C.byref(o),
                                   C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_pairs_file")
        out = C.string_at(sam, sl.value) if sam.value else b""
        if sam.value: L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_pairs_cs(self, mates1: np.ndarray, mates2: np.ndarray, names1=None, names2=None, mode="opp-in", min_insert=0, max_insert=1000,
                     opts: "PairOpts | None" = None, quals1=None, quals2=None, qual_delta=33) -> bytes:
        """Colour-space pairs (gmapper-cs -p opp-in): mates as for map_reads_cs ([n, 1 + colours], column 0 the primer letter code)."""
        from .synth import pack_reads
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        m1 = np.ascontiguousarray(mates1, dtype=np.uint8); m2 = np.ascontiguousarray(mates2, dtype=np.uint8)
        if m1.shape[0] != m2.shape[0]:
            raise ValueError("mates1 and mates2 must hold the same number of reads")
        ib1 = np.ascontiguousarray(m1[:, 0]); ib2 = np.ascontiguousarray(m2[:, 0])
        p1 = np.ascontiguousarray(pack_reads(np.ascontiguousarray(m1[:, 1:]))); p2 = np.ascontiguousarray(pack_reads(np.ascontiguousarray(m2[:, 1:])))
        join = lambda names: None if names is None else b"\n".join(x if isinstance(x, bytes) else x.encode() for x in names)
        o = opts if opts is not None else PairOpts.default(mode, min_insert, max_insert)
        u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        if quals1 is not None:
            jq = lambda q: b"\n".join(bytes(np.ascontiguousarray(r, dtype=np.uint8)) for r in q)
            _check(L.gm_map_pairs_cs_fastq(self.h, m1.shape[0], m1.shape[1] - 1, p1.ctypes.data_as(u32p), ib1.ctypes.data_as(u8p), m2.shape[1] - 1, p2.ctypes.data_as(u32p),
                                           ib2.ctypes.data_as(u8p), join(names1), join(names2), jq(quals1), jq(quals2), int(qual_delta), C.byref(o), C.byref(sam), C.byref(sl),
                                           C.byref(st)), "gm_map_pairs_cs_fastq")
        else:
            _check(L.gm_map_pairs_cs(self.h, m1.shape[0], m1.shape[1] - 1, p1.ctypes.data_as(u32p), ib1.ctypes.data_as(u8p), m2.shape[1] - 1, p2.ctypes.data_as(u32p),
                                     ib2.ctypes.data_as(u8p), join(names1), join(names2), C.byref(o), C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_pairs_cs")
        out = C.string_at(sam, sl.value) if sam.value else b""
        if sam.value: L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_cs_packed(self, packed: np.ndarray, initbp: np.ndarray, n: int, n_colours: int, return_bytes: bool = True):
        """Colour-space reads already packed (pack_reads of the colours, one primer byte per read): the form a timed loop uses.
        With return_bytes=False the SAM text stays in the library's buffer and its length is returned."""
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        _check(L.gm_map_reads_cs(self.h, n, n_colours, packed.ctypes.data_as(C.POINTER(C.c_uint32)), initbp.ctypes.data_as(C.POINTER(C.c_uint8)), None,
                                 C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads_cs")
        out = sl.value
        if return_bytes: out = C.string_at(sam, sl.value) if sam.value else b""
        if sam.value: L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_pairs_packed(self, p1: np.ndarray, p2: np.ndarray, n: int, len1: int, len2: int, opts: "PairOpts", return_bytes: bool = True):
        """Paired mode on packed mates (pack_reads of each mate set)."""
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        _check(L.gm_map_pairs(self.h, n, len1, p1.ctypes.data_as(C.POINTER(C.c_uint32)), len2, p2.ctypes.data_as(C.POINTER(C.c_uint32)),
                              None, None, C.byref(opts), C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_pairs")
        out = sl.value
        if return_bytes: out = C.string_at(sam, sl.value) if sam.value else b""
        if sam.value: L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_reads_text(self, seqs, names=None, quals=None, qual_delta: int = 64) -> bytes:
        """Reads as text lines of one length (letters; or primer + colours in a colour-space session), packed inside the library."""
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        seqs = [x if isinstance(x, bytes) else x.encode() for x in seqs]
        n = len(seqs); read_len = len(seqs[0]) - (1 if self.params.colour_space else 0) if n else 1
        join = lambda v: None if v is None else b"\n".join(x if isinstance(x, bytes) else x.encode() for x in v)
        _check(L.gm_map_reads_text(self.h, n, read_len, b"\n".join(seqs), join(names), join(quals), int(qual_delta), C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads_text")
        out = C.string_at(sam, sl.value) if sam.value else b""
        if sam.value: L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_text_buffer(self, seq_buf: bytes, n: int, read_len: int, names_buf: "bytes | None" = None, return_bytes: bool = True):
        """gm_map_reads_text on a ready-made buffer (n lines of read_len letters, '\\n' between them; names likewise): the form a timed loop uses -- parsing, packing and
        the upload all happen inside the call.  With return_bytes=False the SAM text stays in the library's buffer and its length is returned."""
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        _check(L.gm_map_reads_text(self.h, n, read_len, seq_buf, names_buf, None, 64, C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads_text")
        out = sl.value
        if return_bytes: out = C.string_at(sam, sl.value) if sam.value else b""
        if sam.value: L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_packed(self, packed: np.ndarray, n: int, read_len: int, names=None) -> bytes:
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        nm = None
        if names is not None:
            nm = b"\n".join(x if isinstance(x, bytes) else x.encode() for x in names)
        _check(L.gm_map_reads(self.h, n, read_len, packed.ctypes.data_as(C.POINTER(C.c_uint32)), nm, C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads")
        out = C.string_at(sam, sl.value) if sam.value else b""
        L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_pairs(self, mates1: np.ndarray, mates2: np.ndarray, names1=None, names2=None, mode="opp-in", min_insert=0, max_insert=1000,
                  opts: "PairOpts | None" = None) -> bytes:
        """Paired mode (-p mode -I min,max): mates1 [n, L1], mates2 [n, L2] uint8 codes -> SAM records of every pair, input order."""
        from .synth import pack_reads
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        m1 = np.ascontiguousarray(mates1, dtype=np.uint8); m2 = np.ascontiguousarray(mates2, dtype=np.uint8)
        if m1.shape[0] != m2.shape[0]:
            raise ValueError("mates1 and mates2 must hold the same number of reads")
        p1 = np.ascontiguousarray(pack_reads(m1)); p2 = np.ascontiguousarray(pack_reads(m2))
        join = lambda names: None if names is None else b"\n".join(x if isinstance(x, bytes) else x.encode() for x in names)
        o = opts if opts is not None else PairOpts.default(mode, min_insert, max_insert)
        _check(L.gm_map_pairs(self.h, m1.shape[0], m1.shape[1], p1.ctypes.data_as(C.POINTER(C.c_uint32)), m2.shape[1], p2.ctypes.data_as(C.POINTER(C.c_uint32)),
                              join(names1), join(names2), C.byref(o), C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_pairs")
        out = C.string_at(sam, sl.value) if sam.value else b""
        L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_pairs_fastq(self, mates1: np.ndarray, mates2: np.ndarray, quals1, quals2, qual_delta: int = 64, names1=None, names2=None,
                        mode="opp-in", min_insert=0, max_insert=1000, opts: "PairOpts | None" = None) -> bytes:
        """Paired FASTQ: as map_pairs plus one QUAL string (bytes) per mate and the file's quality offset."""
        from .synth import pack_reads
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        m1 = np.ascontiguousarray(mates1, dtype=np.uint8); m2 = np.ascontiguousarray(mates2, dtype=np.uint8)
        p1 = np.ascontiguousarray(pack_reads(m1)); p2 = np.ascontiguousarray(pack_reads(m2))
        join = lambda names: None if names is None else b"\n".join(x if isinstance(x, bytes) else x.encode() for x in names)
        o = opts if opts is not None else PairOpts.default(mode, min_insert, max_insert)
        _check(L.gm_map_pairs_fastq(self.h, m1.shape[0], m1.shape[1], p1.ctypes.data_as(C.POINTER(C.c_uint32)), m2.shape[1], p2.ctypes.data_as(C.POINTER(C.c_uint32)),
                                    join(names1), join(names2), b"\n".join(quals1), b"\n".join(quals2), int(qual_delta), C.byref(o),
                                    C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_pairs_fastq")
        out = C.string_at(sam, sl.value) if sam.value else b""
        L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def map_device(self, dev_ptr: int, n: int, read_len: int, emit_sam: bool = True, return_bytes: bool = True):
        """Reads already resident in HBM (packed layout).  With return_bytes=False the SAM text is produced
        in the library's buffer and released without a Python-side copy (returns its length)."""
        L = lib(); sam = C.c_void_p(); sl = C.c_size_t(); st = MapStats()
        _check(L.gm_map_reads_device(self.h, n, read_len, C.c_void_p(dev_ptr), int(emit_sam), C.byref(sam), C.byref(sl), C.byref(st)), "gm_map_reads_device")
        out = sl.value
        if return_bytes:
            out = C.string_at(sam, sl.value) if sam.value else b""
        if sam.value: L.gm_free(sam)
        self.stats = st.as_dict()
        return out

    def tophits(self, reads_codes: np.ndarray, initbp=None) -> np.ndarray:
        """initbp (colour space): the reads' primer letters, one per row of colours (gm_debug_tophits_cs)"""
        from .synth import pack_reads
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        n, Lr = reads_codes.shape
        packed = np.ascontiguousarray(pack_reads(reads_codes))
        rows = np.zeros((n * 30, 12), dtype=np.int64); nr = C.c_long()
        if initbp is not None:
            ib = np.ascontiguousarray(initbp, dtype=np.uint8)
            if ib.shape != (n,): raise GmError("tophits: one primer letter per read")
            _check(lib().gm_debug_tophits_cs(self.h, n, Lr, packed.ctypes.data_as(C.POINTER(C.c_uint32)), ib.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             rows.ctypes.data_as(C.POINTER(C.c_longlong)), n * 30, C.byref(nr)), "gm_debug_tophits_cs")
            return rows[:nr.value]
        _check(lib().gm_debug_tophits(self.h, n, Lr, packed.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      rows.ctypes.data_as(C.POINTER(C.c_longlong)), n * 30, C.byref(nr)), "gm_debug_tophits")
        return rows[:nr.value]

    def read_windows(self, reads_codes: np.ndarray, initbp=None):
        """The candidate windows of every read on both strands, before pass 1 (gm_read_windows): -> (wins, off).  wins: structured array of READ_WINDOW_DTYPE;
        off: uint64[2 n + 1], the windows of read r on strand st are wins[off[2 r + st]:off[2 r + st + 1]], ascending (cn, g_off).  As an `_ix` window: strand 0 is
        (cn, 0, g_off, w_len), strand 1 is (cn, 1, Index.strand_offset(contig_len, g_off, w_len), w_len), both with the read as given.
        initbp (colour space): the reads' primer letters, one per row of colours.  The stage counters of the call are left in self.stats."""
        from .synth import pack_reads
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        if reads_codes.ndim != 2: raise GmError("read_windows: reads_codes is [n, L]")
        n, Lr = reads_codes.shape
        packed = np.ascontiguousarray(pack_reads(reads_codes), dtype=np.uint32) if n else np.zeros(1, dtype=np.uint32)
        ib = None
        if initbp is not None:
            ib = np.ascontiguousarray(initbp, dtype=np.uint8)
            if ib.shape != (n,): raise GmError("read_windows: one primer letter per read")
        L = lib(); out = C.c_void_p(); nw = C.c_uint64(0); st = MapStats()
        off = np.zeros(2 * n + 1, dtype=np.uint64)
        _check(L.gm_read_windows(self.h, n, Lr, packed.ctypes.data_as(C.POINTER(C.c_uint32)), None if ib is None else ib.ctypes.data_as(C.POINTER(C.c_uint8)),
                                 C.byref(out), C.byref(nw), off.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st)), "gm_read_windows")
        wins = np.zeros(nw.value, dtype=READ_WINDOW_DTYPE)
        if nw.value: C.memmove(wins.ctypes.data, out, nw.value * READ_WINDOW_DTYPE.itemsize)
        if out.value: L.gm_free(out)
        self.stats = st.as_dict(); self._windows_read_len = Lr
        return wins, off

    def _reads_args(self, who, reads_codes, initbp):
        """[n, L] codes and the primer letters as the read entries take them: -> (n, L, packed, initbp array or None)"""
        from .synth import pack_reads
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        if reads_codes.ndim != 2: raise GmError("%s: reads_codes is [n, L]" % who)
        n, Lr = reads_codes.shape
        packed = np.ascontiguousarray(pack_reads(reads_codes), dtype=np.uint32) if n else np.zeros(1, dtype=np.uint32)
        ib = None
        if initbp is not None:
            ib = np.ascontiguousarray(initbp, dtype=np.uint8)
            if ib.shape != (n,): raise GmError("%s: one primer letter per read" % who)
        return n, Lr, packed, ib

    def score_windows(self, reads_codes, wins, off, initbp=None):
        """The score pass 1 gives every window and its f1 cache slot (gm_score_windows): -> (scores int32[n_wins], slots uint32[n_wins]).  reads_codes / initbp: the batch
        as read_windows takes it (nothing is gathered per window or turned by the caller); wins / off: read_windows', or the caller's own."""
        n, Lr, packed, ib = self._reads_args("score_windows", reads_codes, initbp)
        wins = np.ascontiguousarray(wins, dtype=READ_WINDOW_DTYPE); off = np.ascontiguousarray(off, dtype=np.uint64)
        if off.shape != (2 * n + 1,): raise GmError("score_windows: off has 2 n + 1 entries")
        scores = np.zeros(len(wins), dtype=np.int32); slots = np.zeros(len(wins), dtype=np.uint32)
        _check(lib().gm_score_windows(self.h, n, Lr, packed.ctypes.data_as(C.POINTER(C.c_uint32)), None if ib is None else ib.ctypes.data_as(C.POINTER(C.c_uint8)),
                                      wins.ctypes.data_as(C.c_void_p), len(wins), off.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_int)),
                                      slots.ctypes.data_as(C.POINTER(C.c_uint32))), "gm_score_windows")
        return scores, slots

    def select_pass1(self, wins, off, scores, read_len=None, slots=None, want_bypassed=False):
        """Pass 1's selection (gm_select_pass1) over the windows of read_windows and their vector scores: -> (hits, hit_off).  hits: structured array of
        PASS1_HIT_DTYPE, read r's at hits[hit_off[r]:hit_off[r + 1]] in the heap's array order, strand-1 hits already turned by reverse_hit: (cn, gen_st, g_off, w_len)
        and the box (ax, ay, alen, awidth) go to Index.sw_full_ls_batch / sw_full_cs_batch as they are.  read_len: the reads' length (colours in colour space);
        None: that of this session's last read_windows call.
        slots (score_windows'): the selection with the reference's f1 call cache (gm_select_pass1_f1), its default; None: without it (the reference under -Z).
        want_bypassed: -> (hits, hit_off, bypassed), the number of calls the cache bypassed."""
        if read_len is None: read_len = getattr(self, "_windows_read_len", None)
        if read_len is None: raise GmError("select_pass1: read_len is needed (no read_windows call on this session yet)")
        wins = np.ascontiguousarray(wins, dtype=READ_WINDOW_DTYPE); off = np.ascontiguousarray(off, dtype=np.uint64)
        scores = np.ascontiguousarray(scores, dtype=np.int32)
        if off.ndim != 1 or len(off) < 1 or len(off) % 2 != 1: raise GmError("select_pass1: off has 2 n + 1 entries")
        if scores.shape != (len(wins),): raise GmError("select_pass1: one score per window")
        n = (len(off) - 1) // 2
        L = lib(); out = C.c_void_p(); nh = C.c_uint64(0); byp = C.c_uint64(0)
        hit_off = np.zeros(n + 1, dtype=np.uint64)
        if slots is None and not want_bypassed:
            _check(L.gm_select_pass1(self.h, n, int(read_len), wins.ctypes.data_as(C.c_void_p), len(wins), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                     scores.ctypes.data_as(C.POINTER(C.c_int)), C.byref(out), C.byref(nh), hit_off.ctypes.data_as(C.POINTER(C.c_uint64))), "gm_select_pass1")
        else:
            sl = None
            if slots is not None:
                sl = np.ascontiguousarray(slots, dtype=np.uint32)
                if sl.shape != (len(wins),): raise GmError("select_pass1: one slot per window")
                if len(sl) == 0: sl = np.zeros(1, dtype=np.uint32)   # (an empty array still means: with the cache)
            _check(L.gm_select_pass1_f1(self.h, n, int(read_len), wins.ctypes.data_as(C.c_void_p), len(wins), off.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        scores.ctypes.data_as(C.POINTER(C.c_int)), None if sl is None else sl.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(out), C.byref(nh),
                                        hit_off.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(byp)), "gm_select_pass1_f1")
        hits = np.zeros(nh.value, dtype=PASS1_HIT_DTYPE)
        if nh.value: C.memmove(hits.ctypes.data, out, nh.value * PASS1_HIT_DTYPE.itemsize)
        if out.value: L.gm_free(out)
        return (hits, hit_off, int(byp.value)) if want_bypassed else (hits, hit_off)

    def read_hits(self, reads_codes, initbp=None, want_windows=False):
        """Reads to pass-1 hits in one call (gm_read_hits: read_windows -> score_windows -> select_pass1 with the cache rule iff the session's hash_filter_calls is set):
        -> (hits, hit_off), or with want_windows (hits, hit_off, wins, off, scores) -- the windows as read_windows returns them and their OWN scores.  The stage
        counters of the call are left in self.stats."""
        n, Lr, packed, ib = self._reads_args("read_hits", reads_codes, initbp)
        L = lib(); out = C.c_void_p(); nh = C.c_uint64(0); st = MapStats()
        hit_off = np.zeros(n + 1, dtype=np.uint64)
        wout = C.c_void_p(); sout = C.c_void_p(); nw = C.c_uint64(0); off = np.zeros(2 * n + 1, dtype=np.uint64)
        _check(L.gm_read_hits(self.h, n, Lr, packed.ctypes.data_as(C.POINTER(C.c_uint32)), None if ib is None else ib.ctypes.data_as(C.POINTER(C.c_uint8)),
                              C.byref(out), C.byref(nh), hit_off.ctypes.data_as(C.POINTER(C.c_uint64)),
                              C.byref(wout) if want_windows else None, C.byref(nw) if want_windows else None,
                              off.ctypes.data_as(C.POINTER(C.c_uint64)) if want_windows else None, C.byref(sout) if want_windows else None, C.byref(st)), "gm_read_hits")
        hits = np.zeros(nh.value, dtype=PASS1_HIT_DTYPE)
        if nh.value: C.memmove(hits.ctypes.data, out, nh.value * PASS1_HIT_DTYPE.itemsize)
        if out.value: L.gm_free(out)
        self.stats = st.as_dict(); self._windows_read_len = Lr
        if not want_windows: return hits, hit_off
        wins = np.zeros(nw.value, dtype=READ_WINDOW_DTYPE); scores = np.zeros(nw.value, dtype=np.int32)
        if nw.value:
            C.memmove(wins.ctypes.data, wout, nw.value * READ_WINDOW_DTYPE.itemsize); C.memmove(scores.ctypes.data, sout, nw.value * 4)
        if wout.value: L.gm_free(wout)
        if sout.value: L.gm_free(sout)
        return hits, hit_off, wins, off, scores

    def read_mappings(self, reads_codes, want_ops=False):
        """Reads to mappings in one call (gm_read_mappings: read_hits, then per hit the second vector score, the full alignment at or above the threshold, select_pass2
        and the text of the mappings, on arrays that stay on the device): -> ReadMappings.  Letter space, unpaired.  want_ops: the edit operations of the records come
        down too.  The stage counters of the call are left in self.stats."""
        n, Lr, packed, _ = self._reads_args("read_mappings", reads_codes, None)
        L = lib(); R = ReadMappingsResult(); st = MapStats()
        _check(L.gm_read_mappings(self.h, n, Lr, packed.ctypes.data_as(C.POINTER(C.c_uint32)), None, 1 if want_ops else 0, C.byref(R), C.byref(st)), "gm_read_mappings")
        try:
            def take(p, count, dtype):
                a = np.zeros(count, dtype=dtype)
                if count and p: C.memmove(a.ctypes.data, p, count * a.dtype.itemsize)
                return a
            nh, nm = int(R.n_hits), int(R.n_maps)
            res = ReadMappings(take(R.hits, nh, PASS1_HIT_DTYPE), take(R.hit_off, n + 1, np.uint64), take(R.score_vector, nh, np.int32), take(R.recs, nh, SW_FULL_REC_DTYPE),
                               take(R.maps, nm, MAPPING_DTYPE), take(R.map_off, n + 1, np.uint64),
                               C.string_at(R.cigar, int(R.cigar_len)) if R.cigar else b"", take(R.cigar_off, nh + 1, np.uint64),
                               (C.string_at(R.edit, int(R.edit_len)) if R.edit else b"") if R.has_edit else None, take(R.edit_off, nh + 1, np.uint64) if R.has_edit else None,
                               take(R.ops, int(R.ops_len), np.uint8) if want_ops else None, self.index.contig_lengths())
        finally:
            L.gm_read_mappings_free(C.byref(R))
        self.stats = st.as_dict(); self._windows_read_len = Lr
        return res

    def pair_mappings(self, mates1, mates2, opts=None, want_ops=False):
        """A chunk of read pairs to mapping arrays in one call (gm_pair_mappings: the pipeline of map_pairs with the pair selection on the device and arrays in place
        of SAM text): mates1 [n, L1], mates2 [n, L2] uint8 codes, opts a PairOpts (None: the defaults) -> PairMappings.  Letter space; match_mode 4 and 3.  want_ops: the
        edit operations of the records come down too.  The stage counters of the call are left in self.stats."""
        from .synth import pack_reads
        m1 = np.ascontiguousarray(mates1, dtype=np.uint8); m2 = np.ascontiguousarray(mates2, dtype=np.uint8)
        if m1.ndim != 2 or m2.ndim != 2 or m1.shape[0] != m2.shape[0]:
            raise ValueError("pair_mappings: mates1 [n, L1] and mates2 [n, L2] must hold the same number of reads")
        n = m1.shape[0]
        p1 = np.ascontiguousarray(pack_reads(m1)); p2 = np.ascontiguousarray(pack_reads(m2))
        o = opts if opts is not None else PairOpts.default()
        L = lib(); R = PairMappingsResult(); st = MapStats(); u32p = C.POINTER(C.c_uint32)
        _check(L.gm_pair_mappings(self.h, n, m1.shape[1], p1.ctypes.data_as(u32p), m2.shape[1], p2.ctypes.data_as(u32p), C.byref(o), 1 if want_ops else 0, C.byref(R), C.byref(st)),
               "gm_pair_mappings")
        try:
            def take(p, count, dtype):
                a = np.zeros(count, dtype=dtype)
                if count and p: C.memmove(a.ctypes.data, p, count * a.dtype.itemsize)
                return a
            text = lambda p, k: C.string_at(p, int(k)) if p else b""
            nh = [int(R.n_hits[m]) for m in (0, 1)]; nu = [int(R.n_umaps[m]) for m in (0, 1)]
            res = PairMappings(n, [take(R.hits[m], nh[m], PASS1_HIT_DTYPE) for m in (0, 1)], [take(R.hit_off[m], n + 1, np.uint64) for m in (0, 1)],
                               [take(R.hit_kind[m], nh[m], np.uint8) for m in (0, 1)], [take(R.recs[m], nh[m], SW_FULL_REC_DTYPE) for m in (0, 1)],
                               take(R.pmaps, int(R.n_pmaps), PAIR_MAPPING_DTYPE), take(R.pmap_off, n + 1, np.uint64),
                               [take(R.umaps[m], nu[m], MAPPING_DTYPE) for m in (0, 1)], [take(R.umap_off[m], n + 1, np.uint64) for m in (0, 1)],
                               [take(R.umap_z45[m], 2 * nu[m], np.float64).reshape(nu[m], 2) for m in (0, 1)],
                               [text(R.cigar[m], R.cigar_len[m]) for m in (0, 1)], [take(R.cigar_off[m], nh[m] + 1, np.uint64) for m in (0, 1)],
                               [text(R.edit[m], R.edit_len[m]) if R.has_edit else None for m in (0, 1)],
                               [take(R.edit_off[m], nh[m] + 1, np.uint64) if R.has_edit else None for m in (0, 1)],
                               [take(R.ops[m], int(R.ops_len[m]), np.uint8) if want_ops else None for m in (0, 1)], self.index.contig_lengths())
        finally:
            L.gm_pair_mappings_free(C.byref(R))
        self.stats = st.as_dict()
        return res

    def debug_pair_select(self, pair_mode, cnt0, wins0, cnt1, wins1, plist, pcnt):
        """Test hook (gm_debug_pair_select): the device pair selection of pair_mappings beside the host loop of map_pairs on hand-made candidate lists, under this
        session's num_outputs, strata, max_alignments and sw_full_threshold.  wins0 / wins1: [sum(cnt), 9] int32 rows (cn, gen_st, genome_start, rmapped, deletions,
        insertions, score_full, score_max, sort_idx); plist [n, 64] uint32 candidates (a << 8) | b, pcnt [n].  -> (device pairs per pair, host pairs per pair), each a list
        of lists of (a, b)."""
        cnt0 = np.ascontiguousarray(cnt0, dtype=np.uint32); cnt1 = np.ascontiguousarray(cnt1, dtype=np.uint32); pcnt = np.ascontiguousarray(pcnt, dtype=np.uint32)
        wins0 = np.ascontiguousarray(wins0, dtype=np.int32).reshape(-1, 9); wins1 = np.ascontiguousarray(wins1, dtype=np.int32).reshape(-1, 9)
        plist = np.ascontiguousarray(plist, dtype=np.uint32)
        n = cnt0.shape[0]
        if cnt1.shape[0] != n or pcnt.shape[0] != n or plist.shape != (n, 64) or wins0.shape[0] != int(cnt0.sum()) or wins1.shape[0] != int(cnt1.sum()):
            raise ValueError("debug_pair_select: the arrays do not agree")
        out = [np.zeros((n, 64), dtype=np.uint32) for _ in range(2)]; oc = [np.zeros(n, dtype=np.uint32) for _ in range(2)]
        u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
        _check(lib().gm_debug_pair_select(self.h, int(pair_mode), n, cnt0.ctypes.data_as(u32p), wins0.ctypes.data_as(i32p), cnt1.ctypes.data_as(u32p), wins1.ctypes.data_as(i32p),
                                          plist.ctypes.data_as(u32p), pcnt.ctypes.data_as(u32p), out[0].ctypes.data_as(u32p), oc[0].ctypes.data_as(u32p),
                                          out[1].ctypes.data_as(u32p), oc[1].ctypes.data_as(u32p)), "gm_debug_pair_select")
        return tuple([[(int(v) >> 8, int(v) & 0xff) for v in out[k][pr, :int(oc[k][pr])]] for pr in range(n)] for k in range(2))

    def read_mappings_cs(self, reads_codes, initbp=None, quals=None, qual_delta=33, want_ops=False):
        """Colour reads to mappings in one call (gm_read_mappings_cs: read_hits, then per hit sw_full_cs, post_sw under the session's constants with the host re-dos and
        the rounding guard inside, select_pass2 and the text of the mappings with clip "H", on arrays that stay on the device): -> ReadMappingsCs.
        reads_codes: [n, colours] with initbp, or (initbp None) [n, 1 + colours] with the primer letter code in column 0 as map_reads_cs takes them; quals: None or one
        QV string (bytes, a character a colour) per read, as map_reads_cs_fastq takes them.  The stage counters of the call are left in self.stats."""
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        if initbp is None and reads_codes.ndim == 2 and reads_codes.shape[1] >= 1:
            initbp = np.ascontiguousarray(reads_codes[:, 0]); reads_codes = np.ascontiguousarray(reads_codes[:, 1:])
        n, Lr, packed, ib = self._reads_args("read_mappings_cs", reads_codes, initbp)
        q = None
        if quals is not None:
            quals = [x if isinstance(x, bytes) else x.encode() for x in quals]
            if len(quals) != n: raise GmError("read_mappings_cs: one QV string per read")
            q = b"\n".join(quals)
        L = lib(); R = ReadMappingsCsResult(); st = MapStats()
        _check(L.gm_read_mappings_cs(self.h, n, Lr, packed.ctypes.data_as(C.POINTER(C.c_uint32)), None if ib is None else ib.ctypes.data_as(C.POINTER(C.c_uint8)), q, int(qual_delta),
                                     1 if want_ops else 0, C.byref(R), C.byref(st)), "gm_read_mappings_cs")
        try:
            def take(p, count, dtype):
                a = np.zeros(count, dtype=dtype)
                if count and p: C.memmove(a.ctypes.data, p, count * a.dtype.itemsize)
                return a
            nh, nm = int(R.n_hits), int(R.n_maps)
            res = ReadMappingsCs(take(R.hits, nh, PASS1_HIT_DTYPE), take(R.hit_off, n + 1, np.uint64), take(R.score_vector, nh, np.int32), take(R.recs, nh, SW_FULL_REC_DTYPE),
                                 take(R.maps, nm, MAPPING_DTYPE), take(R.map_off, n + 1, np.uint64),
                                 C.string_at(R.cigar, int(R.cigar_len)) if R.cigar else b"", take(R.cigar_off, nh + 1, np.uint64),
                                 (C.string_at(R.edit, int(R.edit_len)) if R.edit else b"") if R.has_edit else None, take(R.edit_off, nh + 1, np.uint64) if R.has_edit else None,
                                 take(R.ops, int(R.ops_len), np.uint8) if want_ops else None, self.index.contig_lengths(),
                                 post=take(R.post, nh, POST_REC_DTYPE) if gm_mqv_on(self.params) else None,
                                 post_quals=C.string_at(R.post_quals, int(R.post_quals_len)) if R.post_quals else b"",
                                 qralign=C.string_at(R.qralign, int(R.ops_len)) if R.qralign else b"")
        finally:
            L.gm_read_mappings_cs_free(C.byref(R))
        self.stats = st.as_dict(); self._windows_read_len = Lr
        return res

    def select_pass2(self, hits, hit_off, recs, post=None):
        """Pass 2's selection and the mapping qualities (gm_select_pass2) over the records of ONE full batch call on the hits of select_pass1: -> (maps, map_off).
        maps: structured array of MAPPING_DTYPE in the reference's output order, read r's at maps[map_off[r]:map_off[r + 1]]; post: the POST_REC_DTYPE answers of
        post_sw_batch, required in colour space with mapping qualities on.  flags bit 0: see include/gmapper_hip.h."""
        hits = np.ascontiguousarray(hits, dtype=PASS1_HIT_DTYPE); hit_off = np.ascontiguousarray(hit_off, dtype=np.uint64)
        recs = np.ascontiguousarray(recs, dtype=SW_FULL_REC_DTYPE)
        if hit_off.ndim != 1 or len(hit_off) < 1: raise GmError("select_pass2: hit_off has n + 1 entries")
        if len(recs) != len(hits): raise GmError("select_pass2: one record per hit")
        if post is not None:
            post = np.ascontiguousarray(post, dtype=POST_REC_DTYPE)
            if len(post) != len(hits): raise GmError("select_pass2: one post record per hit")
        n = len(hit_off) - 1
        if int(hit_off[-1]) != len(hits): raise GmError("select_pass2: hit_off ends at %d, there are %d hits" % (int(hit_off[-1]), len(hits)))
        L = lib(); out = C.c_void_p(); nm = C.c_uint64(0)
        map_off = np.zeros(n + 1, dtype=np.uint64)
        _check(L.gm_select_pass2(self.h, n, hit_off.ctypes.data_as(C.POINTER(C.c_uint64)), hits.ctypes.data_as(C.c_void_p), recs.ctypes.data_as(C.c_void_p),
                                 None if post is None else post.ctypes.data_as(C.c_void_p), C.byref(out), C.byref(nm), map_off.ctypes.data_as(C.POINTER(C.c_uint64))),
               "gm_select_pass2")
        maps = np.zeros(nm.value, dtype=MAPPING_DTYPE)
        if nm.value: C.memmove(maps.ctypes.data, out, nm.value * MAPPING_DTYPE.itemsize)
        if out.value: L.gm_free(out)
        return maps, map_off

    def sam_records(self, reads_codes, hits, recs=None, maps=None, map_off=None, cigar=None, *, initbp=None, names=None, seqs=None, quals=None, qual_delta=33, score_vector=None, post=None,
                    post_quals=None, qralign=None, edit=None):
        """The SAM text of a chunk's mappings (gm_sam_records): -> (bytes, read_off), read r's records at bytes[read_off[r]:read_off[r + 1]].
        reads_codes: [n, L] uint8 codes (colour space: the colours, with initbp); hits / recs / maps / map_off: select_pass1's hits, the records of the ONE full batch
        call over them, select_pass2's answer; cigar / edit: what Index.sw_full_batch_text returned for ALL hits (reverse = gen_st; clip "S" letter / "H" colour), or a
        (buffer, offsets) pair; qralign / post_quals: what post_sw_batch returned (the text call's qralign where there is no post_sw), or the whole buffers; names /
        seqs / quals: None or one bytes a read; score_vector: ZV of every hit (None: hits["score_vector"]).  The rules: include/gmapper_hip.h."""
        from .synth import pack_reads
        if isinstance(hits, ReadMappings):                                   # read_mappings' answer: its arrays, ZV = its second vector score
            rm = hits
            hits, recs, maps, map_off, cigar = rm.hits, rm.recs, rm.maps, rm.map_off, (rm.cigar_buf, rm.cigar_off)
            if score_vector is None: score_vector = rm.score_vector
            if edit is None and rm.edit_off is not None: edit = (rm.edit_buf, rm.edit_off)
            if isinstance(rm, ReadMappingsCs):                               # colour space: post_sw's answers and the read letters
                if post is None: post = rm.post
                if post_quals is None and rm.post is not None: post_quals = rm.post_quals
                if qralign is None: qralign = rm.qralign
        if recs is None or maps is None or map_off is None or cigar is None: raise GmError("sam_records: recs, maps, map_off and cigar are required beside plain hits")
        reads_codes = np.ascontiguousarray(reads_codes, dtype=np.uint8)
        if reads_codes.ndim != 2: raise GmError("sam_records: reads_codes is (n, read_len)")
        n, Lr = reads_codes.shape
        packed = np.ascontiguousarray(pack_reads(reads_codes), dtype=np.uint32) if n and Lr else np.zeros((n, 1), dtype=np.uint32)
        hits = np.ascontiguousarray(hits, dtype=PASS1_HIT_DTYPE); recs = np.ascontiguousarray(recs, dtype=SW_FULL_REC_DTYPE)
        maps = np.ascontiguousarray(maps, dtype=MAPPING_DTYPE); map_off = np.ascontiguousarray(map_off, dtype=np.uint64)
        if len(recs) != len(hits): raise GmError("sam_records: one record per hit")
        if len(map_off) != n + 1: raise GmError("sam_records: map_off has n + 1 entries")
        keep = []
        def arr(a, dtype, what):
            if a is None: return None
            a = np.ascontiguousarray(a, dtype=dtype); keep.append(a)
            if len(a) != len(hits): raise GmError("sam_records: one %s per hit" % what)
            return a.ctypes.data
        def lines(x):
            if x is None: return None
            return x if isinstance(x, bytes) else b"\n".join(t if isinstance(t, bytes) else t.encode() for t in x)
        def whole(x):                                                        # a buffer, or the accessor a batch call returned
            if x is None: return None
            b = getattr(x, "buffer", x)
            return b if isinstance(b, bytes) else bytes(b)
        def text(x, what):                                                   # (buffer, n_hits + 1 offsets)
            if x is None: return None, None
            b, off = (x.buffer, x.offsets) if hasattr(x, "buffer") else x
            off = np.ascontiguousarray(off, dtype=np.uint64); keep.append(off)
            if len(off) != len(hits) + 1: raise GmError("sam_records: %s has n_hits + 1 offsets" % what)
            return (b if isinstance(b, bytes) else bytes(b)), off.ctypes.data
        ib = None if initbp is None else np.ascontiguousarray(initbp, dtype=np.uint8)
        if ib is not None and len(ib) != n: raise GmError("sam_records: one primer letter per read")
        I = SAM_INPUT(); I.n_reads, I.read_len = n, Lr
        I.reads_packed = packed.ctypes.data; I.initbp = None if ib is None else ib.ctypes.data
        I.names, I.seqs, I.quals, I.qual_delta = lines(names), lines(seqs), lines(quals), int(qual_delta)
        I.n_hits = len(hits); I.hits = hits.ctypes.data if len(hits) else None; I.recs = recs.ctypes.data if len(hits) else None
        I.score_vector = arr(score_vector, np.int32, "vector score"); I.post = arr(post, POST_REC_DTYPE, "post record")
        pq = whole(post_quals); I.post_quals = pq; I.post_quals_len = 0 if pq is None else len(pq)
        qa = whole(qralign); I.qralign = qa; I.ops_len = 0 if qa is None else len(qa)
        I.cigar, I.cigar_off = text(cigar, "cigar"); I.edit, I.edit_off = text(edit, "edit")
        I.n_maps = len(maps); I.maps = maps.ctypes.data if len(maps) else None; I.map_off = map_off.ctypes.data
        L = lib(); out = C.c_void_p(); sl = C.c_size_t(0)
        read_off = np.zeros(n + 1, dtype=np.uint64)
        _check(L.gm_sam_records(self.h, C.byref(I), C.byref(out), C.byref(sl), read_off.ctypes.data_as(C.POINTER(C.c_uint64))), "gm_sam_records")
        sam = C.string_at(out, sl.value) if out.value else b""
        if out.value: L.gm_free(out)
        return sam, read_off

    def lookup_timing(self):
        ms = C.c_double(); b = C.c_uint64(); n = C.c_int()
        lib().gm_last_lookup_timing(self.h, C.byref(ms), C.byref(b), C.byref(n))
        return ms.value, b.value, n.value

    def close(self):
        if getattr(self, "h", None):
            lib().gm_session_free(self.h); self.h = None

    def __del__(self):
        try: self.close()
        except Exception: pass


# ---- S1 / S2 seams ---------------------------------------------------------------------------------
def sw_vector_setup(dblen, qrlen, a_gap_open, a_gap_ext, b_gap_open, b_gap_ext, match, mismatch, use_colours=0, reset_stats=True):
    _check(lib().sw_vector_setup(dblen, qrlen, a_gap_open, a_gap_ext, b_gap_open, b_gap_ext, match, mismatch, use_colours, reset_stats), "sw_vector_setup")


def sw_vector_batch(genome_words: np.ndarray, g_off, glen, reads_words: np.ndarray, rlen) -> np.ndarray:
    L = lib()
    genome_words = np.ascontiguousarray(genome_words, dtype=np.uint32)
    reads_words = np.ascontiguousarray(reads_words, dtype=np.uint32)
    n = reads_words.shape[0]
    g_off = np.ascontiguousarray(g_off, dtype=np.int64); glen = np.ascontiguousarray(glen, dtype=np.int32); rlen = np.ascontiguousarray(rlen, dtype=np.int32)
    out = np.zeros(n, dtype=np.int32)
    _check(L.gm_sw_vector_batch(n, genome_words.ctypes.data_as(C.POINTER(C.c_uint32)), genome_words.size,
                                g_off.ctypes.data_as(C.POINTER(C.c_int64)), glen.ctypes.data_as(C.POINTER(C.c_int)),
                                reads_words.ctypes.data_as(C.POINTER(C.c_uint32)), reads_words.shape[1],
                                rlen.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_int))), "gm_sw_vector_batch")
    return out


def sw_vector_batch_bounded(genome_words: np.ndarray, g_off, glen, reads_words: np.ndarray, rlen, threshold: int):
    """gm_sw_vector_batch with pass 1's early stop against `threshold`: (scores, stopped); where stopped, the score is a lower bound below the threshold"""
    L = lib()
    genome_words = np.ascontiguousarray(genome_words, dtype=np.uint32)
    reads_words = np.ascontiguousarray(reads_words, dtype=np.uint32)
    n = reads_words.shape[0]
    g_off = np.ascontiguousarray(g_off, dtype=np.int64); glen = np.ascontiguousarray(glen, dtype=np.int32); rlen = np.ascontiguousarray(rlen, dtype=np.int32)
    out = np.zeros(n, dtype=np.int32); stopped = np.zeros(n, dtype=np.uint8)
    _check(L.gm_sw_vector_batch_bounded(n, genome_words.ctypes.data_as(C.POINTER(C.c_uint32)), genome_words.size,
                                        g_off.ctypes.data_as(C.POINTER(C.c_int64)), glen.ctypes.data_as(C.POINTER(C.c_int)),
                                        reads_words.ctypes.data_as(C.POINTER(C.c_uint32)), reads_words.shape[1],
                                        rlen.ctypes.data_as(C.POINTER(C.c_int)), int(threshold), out.ctypes.data_as(C.POINTER(C.c_int)),
                                        stopped.ctypes.data_as(C.POINTER(C.c_uint8))), "gm_sw_vector_batch_bounded")
    return out, stopped


def sw_vector(genome_words, goff, glen, read_words, rlen, genome_ls=None, initbp=-1, is_rna=False) -> int:
    g = np.ascontiguousarray(genome_words, dtype=np.uint32); r = np.ascontiguousarray(read_words, dtype=np.uint32)
    gl = None
    if genome_ls is not None:
        gla = np.ascontiguousarray(genome_ls, dtype=np.uint32); gl = gla.ctypes.data_as(C.POINTER(C.c_uint32))
    return lib().sw_vector(g.ctypes.data_as(C.POINTER(C.c_uint32)), goff, glen, r.ctypes.data_as(C.POINTER(C.c_uint32)), rlen, gl, initbp, bool(is_rna))


def sw_gapless_setup(match, mismatch, reset_stats=True):
    _check(lib().sw_gapless_setup(match, mismatch, reset_stats), "sw_gapless_setup")


def sw_gapless_batch(genome_words, genome_woff, glen, reads_words, rlen, g_idx, r_idx, genome_ls=None, initbp=None) -> np.ndarray:
    """n calls of the ungapped filter (ref: sw-gapless.c:57-117): call i's bitfield starts at word genome_woff[i]; colour space: genome_ls + initbp"""
    L = lib()
    g = np.ascontiguousarray(genome_words, dtype=np.uint32); r = np.ascontiguousarray(reads_words, dtype=np.uint32)
    n = r.shape[0]
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    wo = np.ascontiguousarray(genome_woff, dtype=np.int64); out = np.zeros(n, dtype=np.int32)
    gn, rl, gi, ri = (np.ascontiguousarray(a, dtype=np.int32) for a in (glen, rlen, g_idx, r_idx))
    gl = np.ascontiguousarray(genome_ls, dtype=np.uint32) if genome_ls is not None else None
    ib = np.ascontiguousarray(initbp, dtype=np.int32) if initbp is not None else None
    _check(L.gm_sw_gapless_batch(n, u32(g), u32(gl) if gl is not None else None, g.size if gl is None else min(g.size, gl.size), wo.ctypes.data_as(C.POINTER(C.c_int64)), ip(gn),
                                 u32(r), r.shape[1], ip(rl), ip(gi), ip(ri), ip(ib) if ib is not None else None, ip(out)), "gm_sw_gapless_batch")
    return out


def sw_gapless(genome_words, glen, read_words, rlen, g_idx, r_idx, genome_ls=None, init_bp=-1) -> int:
    g = np.ascontiguousarray(genome_words, dtype=np.uint32); r = np.ascontiguousarray(read_words, dtype=np.uint32)
    gl = None
    if genome_ls is not None:
        gla = np.ascontiguousarray(genome_ls, dtype=np.uint32); gl = gla.ctypes.data_as(C.POINTER(C.c_uint32))
    return lib().sw_gapless(g.ctypes.data_as(C.POINTER(C.c_uint32)), glen, r.ctypes.data_as(C.POINTER(C.c_uint32)), rlen, g_idx, r_idx, gl, init_bp, False)


def sw_full_ls_setup(dblen, qrlen, a_gap_open, a_gap_ext, b_gap_open, b_gap_ext, match, mismatch, reset_stats=True, anchor_width=8):
    _check(lib().sw_full_ls_setup(dblen, qrlen, a_gap_open, a_gap_ext, b_gap_open, b_gap_ext, match, mismatch, reset_stats, anchor_width), "sw_full_ls_setup")


def sw_full_ls(genome_words, goff, glen, read_words, rlen, anchor, revcmpl=False, threshscore=0, maxscore=0, local_alignment=False):
    """anchor = (x, y, length, width) or None (the threshold band); returns (fields dict, dbalign, qralign)."""
    L = lib()
    g = np.ascontiguousarray(genome_words, dtype=np.uint32); r = np.ascontiguousarray(read_words, dtype=np.uint32)
    a = Anchor(anchor[0], anchor[1], anchor[2], anchor[3], 1, 0, 0) if anchor is not None else None
    s = SwFullResults()
    L.sw_full_ls(g.ctypes.data_as(C.POINTER(C.c_uint32)), goff, glen, r.ctypes.data_as(C.POINTER(C.c_uint32)), rlen, int(threshscore), int(maxscore),
                 C.byref(s), bool(revcmpl), C.byref(a) if a is not None else None, 1 if a is not None else 0, 1 if local_alignment else 0)
    db = C.string_at(s.dbalign).decode() if s.dbalign else ""
    qr = C.string_at(s.qralign).decode() if s.qralign else ""
    L.gm_free(s.dbalign); L.gm_free(s.qralign)
    return {n: getattr(s, n) for n, _ in SwFullResults._fields_[:9]}, db, qr


def _anchor_array(anchors, n):
    """(n, 4) rows of x, y, length, width (a row with length 0: no box) -> an array of struct gm_anchor"""
    a = np.asarray(anchors, dtype=np.int64).reshape(n, 4)
    out = np.zeros(n, dtype=ANCHOR_DTYPE)
    out["x"] = a[:, 0]; out["y"] = a[:, 1]; out["length"] = a[:, 2]; out["width"] = a[:, 3]; out["weight"] = 1
    return out


def sw_full_batch_strings(colour_space, rec, ops, genome_words, read_words, initbp=0, is_rna=False, rlen=None):
    """gm_sw_full_batch_strings (host only): (dbalign, qralign) of one record as the single seams return them; colour space without alignment: (None, None).
    rlen: the read's length (default: all positions of read_words); the library refuses a record that points outside ops, the genome or the read."""
    L = lib()
    g = np.ascontiguousarray(genome_words, dtype=np.uint32); r = np.ascontiguousarray(read_words, dtype=np.uint32)
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    one = np.ascontiguousarray(np.asarray(rec, dtype=SW_FULL_REC_DTYPE).reshape(1))
    db, qr = C.c_void_p(), C.c_void_p()
    _check(L.gm_sw_full_batch_strings(1 if colour_space else 0, one.ctypes.data, o.ctypes.data if o.size else None, o.size, g.ctypes.data_as(C.POINTER(C.c_uint32)), g.size * 8,
                                      r.ctypes.data_as(C.POINTER(C.c_uint32)), r.size * 8 if rlen is None else int(rlen), int(initbp), 1 if is_rna else 0, C.byref(db), C.byref(qr)), "gm_sw_full_batch_strings")
    out = tuple(None if p.value is None else C.string_at(p.value).decode() for p in (db, qr))
    L.gm_free(db); L.gm_free(qr)
    return out


def _sw_full_batch_finish(colour, recs, ops_p, ops_len, g, r, rl, initbp, is_rna):
    L = lib()
    ops = np.ctypeslib.as_array(C.cast(ops_p, C.POINTER(C.c_uint8)), shape=(ops_len.value,)).copy() if ops_len.value else np.zeros(0, dtype=np.uint8)
    L.gm_free(ops_p)
    def strings(i):
        return sw_full_batch_strings(colour, recs[i], ops, g, r[i], 0 if initbp is None else int(initbp[i]), is_rna, rlen=int(rl[i]))
    return recs, ops, strings


def sw_full_ls_batch(genome_words, g_off, glen, reads_words, rlen, anchors=None, revcmpl=None, threshscore=None, maxscore=None, local_alignment=False):
    """gm_sw_full_ls_batch: n sw_full_ls calls in one.  anchors: (n, 4) rows x, y, length, width (length 0: the threshold band for that item) or None (for all).
    Returns (records: structured array of SW_FULL_REC_DTYPE, ops: uint8 buffer, strings: i -> (dbalign, qralign))."""
    L = lib()
    g = np.ascontiguousarray(genome_words, dtype=np.uint32); r = np.ascontiguousarray(reads_words, dtype=np.uint32)
    if r.ndim != 2: raise GmError("sw_full_ls_batch: reads_words is (n, read_words)")
    n = r.shape[0]
    go = np.ascontiguousarray(g_off, dtype=np.int64); gn = np.ascontiguousarray(glen, dtype=np.int32); rl = np.ascontiguousarray(rlen, dtype=np.int32)
    th = np.ascontiguousarray(threshscore if threshscore is not None else np.zeros(n), dtype=np.int32)
    mx = None if maxscore is None else np.ascontiguousarray(maxscore, dtype=np.int32)
    rv = None if revcmpl is None else np.ascontiguousarray(revcmpl, dtype=np.uint8)
    an = None if anchors is None else _anchor_array(anchors, n)
    if any(a is not None and a.shape[0] != n for a in (go, gn, rl, th, mx, rv)): raise GmError("sw_full_ls_batch: every per-item array has n entries")
    recs = np.zeros(n, dtype=SW_FULL_REC_DTYPE); ops_p = C.c_void_p(); ops_len = C.c_uint64(0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)); dp = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    _check(L.gm_sw_full_ls_batch(n, g.ctypes.data_as(C.POINTER(C.c_uint32)), g.size, go.ctypes.data_as(C.POINTER(C.c_int64)), ip(gn), r.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 r.shape[1], ip(rl), dp(an), dp(rv), ip(th), dp(mx), 1 if local_alignment else 0, dp(recs), C.byref(ops_p), C.byref(ops_len)), "gm_sw_full_ls_batch")
    return _sw_full_batch_finish(False, recs, ops_p, ops_len, g, r, rl, None, False)


def sw_full_cs_batch(genome_ls, g_off, glen, reads_words, rlen, initbp, anchors, revcmpl=None, threshscore=None, xover=None, is_rna=False, local_alignment=False):
    """gm_sw_full_cs_batch: n sw_full_cs calls in one.  anchors: (n, 4) rows x, y, length, width; xover: None or (n, >= max rlen) per-position crossover scores.
    Returns (records, ops, strings) as sw_full_ls_batch; an item the device path refuses has status < 0 (reason: gm_last_error)."""
    L = lib()
    g = np.ascontiguousarray(genome_ls, dtype=np.uint32); r = np.ascontiguousarray(reads_words, dtype=np.uint32)
    if r.ndim != 2: raise GmError("sw_full_cs_batch: reads_words is (n, read_words)")
    n = r.shape[0]
    go = np.ascontiguousarray(g_off, dtype=np.int64); gn = np.ascontiguousarray(glen, dtype=np.int32); rl = np.ascontiguousarray(rlen, dtype=np.int32)
    ib = np.ascontiguousarray(initbp, dtype=np.uint8)
    th = np.ascontiguousarray(threshscore if threshscore is not None else np.zeros(n), dtype=np.int32)
    rv = None if revcmpl is None else np.ascontiguousarray(revcmpl, dtype=np.uint8)
    an = _anchor_array(anchors, n)
    xs = None if xover is None else np.ascontiguousarray(xover, dtype=np.int32)
    if xs is not None and (xs.ndim != 2 or xs.shape[0] != n): raise GmError("sw_full_cs_batch: xover is (n, row length)")
    if any(a is not None and a.shape[0] != n for a in (go, gn, rl, th, ib, rv)): raise GmError("sw_full_cs_batch: every per-item array has n entries")
    recs = np.zeros(n, dtype=SW_FULL_REC_DTYPE); ops_p = C.c_void_p(); ops_len = C.c_uint64(0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int)); dp = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    _check(L.gm_sw_full_cs_batch(n, g.ctypes.data_as(C.POINTER(C.c_uint32)), g.size, go.ctypes.data_as(C.POINTER(C.c_int64)), ip(gn), r.ctypes.data_as(C.POINTER(C.c_uint32)),
                                 r.shape[1], ip(rl), dp(ib), dp(an), dp(rv), ip(th), dp(xs), 0 if xs is None else xs.shape[1], 1 if is_rna else 0,
                                 1 if local_alignment else 0, dp(recs), C.byref(ops_p), C.byref(ops_len)), "gm_sw_full_cs_batch")
    return _sw_full_batch_finish(True, recs, ops_p, ops_len, g, r, rl, ib, is_rna)


# ---- colour space S1/S2/S3 at the kernel seams (the read pipeline is Session.map_reads_cs*) ----
def sw_vector_batch_cs(genome_cs, genome_ls, g_off, glen, reads_words, rlen, initbp):
    """colour-space vector filter: genome_cs / genome_ls = colour and letter bitfields of the same contig; one initial base per read"""
    L = lib()
    gc = np.ascontiguousarray(genome_cs, dtype=np.uint32); gl = np.ascontiguousarray(genome_ls, dtype=np.uint32)
    r = np.ascontiguousarray(reads_words, dtype=np.uint32)
    n = r.shape[0]
    go = np.ascontiguousarray(g_off, dtype=np.int64); gn = np.ascontiguousarray(glen, dtype=np.int32); rl = np.ascontiguousarray(rlen, dtype=np.int32)
    ib = np.ascontiguousarray(initbp, dtype=np.int32); out = np.zeros(n, dtype=np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _check(L.gm_sw_vector_batch_cs(n, gc.ctypes.data_as(C.POINTER(C.c_uint32)), gl.ctypes.data_as(C.POINTER(C.c_uint32)), min(gc.size, gl.size),
                                   go.ctypes.data_as(C.POINTER(C.c_int64)), ip(gn), r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[1], ip(rl), ip(ib), ip(out)),
           "gm_sw_vector_batch_cs")
    return out


def preprocess_read(params, seq: bytes, qual: "bytes | None" = None, qual_delta: int = 64, mate: int = 0):
    """gm_preprocess_read_text (host only): what the file entries do to one read before mapping it -> (seq, qual, dropped)"""
    sb = C.create_string_buffer(seq, len(seq) + 1); qb = None if qual is None else C.create_string_buffer(qual, len(qual) + 1); d = C.c_int(0)
    _check(lib().gm_preprocess_read_text(C.byref(params), int(mate), sb, qb, int(qual_delta), C.byref(d)), "gm_preprocess_read_text")
    return sb.value, (None if qb is None else qb.value), bool(d.value)


def sw_full_cs_setup(dblen, qrlen, a_gap_open, a_gap_ext, b_gap_open, b_gap_ext, match, mismatch, xover, reset_stats=True, anchor_width=8, indel_taboo_len=0):
    _check(lib().sw_full_cs_setup(dblen, qrlen, a_gap_open, a_gap_ext, b_gap_open, b_gap_ext, match, mismatch, xover, reset_stats, anchor_width, indel_taboo_len),
           "sw_full_cs_setup")


def sw_full_cs(genome_ls, goff, glen, read_words, rlen, initbp, thresh, anchor, revcmpl=False, local=False, xover=None, is_rna=False):
    """anchor = (x, y, length, width), or None after a setup with anchor_width -1 (the threshold band); local: the reference's local_alignment argument; xover: the reference's crossover_score argument (one int per read position, what
    gmapper hands over for a read with quality values, ref: mapping.c:375-379) or None; returns (fields dict incl. crossovers, dbalign, qralign)."""
    L = lib()
    g = np.ascontiguousarray(genome_ls, dtype=np.uint32); r = np.ascontiguousarray(read_words, dtype=np.uint32)
    a = None if anchor is None else Anchor(anchor[0], anchor[1], anchor[2], anchor[3], 1, 0, 0)
    s = SwFullResults()
    xs = None if xover is None else np.ascontiguousarray(xover, dtype=np.int32)
    L.sw_full_cs(g.ctypes.data_as(C.POINTER(C.c_uint32)), goff, glen, r.ctypes.data_as(C.POINTER(C.c_uint32)), rlen, initbp, thresh,
                 C.byref(s), bool(revcmpl), bool(is_rna), None if a is None else C.byref(a), 1 if a is not None else 0, 1 if local else 0, None if xs is None else xs.ctypes.data_as(C.POINTER(C.c_int)))
    db = C.string_at(s.dbalign).decode() if s.dbalign else ""
    qr = C.string_at(s.qralign).decode() if s.qralign else ""
    if s.dbalign: L.gm_free(s.dbalign)
    if s.qralign: L.gm_free(s.qralign)
    f = {n: getattr(s, n) for n in ("score", "read_start", "rmapped", "genome_start", "gmapped", "matches", "mismatches", "insertions", "deletions", "crossovers")}
    return f, db, qr


def post_sw_setup(max_len, pr_snp, pr_xover, pr_del_open, pr_del_extend, pr_ins_open, pr_ins_extend, use_read_qvs=False, use_sanger_qvs=True, qual_vector_offset=0,
                  qual_delta=33, reset_stats=True):
    """post_sw_setup (ref: sw-post.c:364-441): this thread's state for post_sw and post_sw_batch.  Host only."""
    lib().post_sw_setup(int(max_len), pr_snp, pr_xover, pr_del_open, pr_del_extend, pr_ins_open, pr_ins_extend, bool(use_read_qvs), bool(use_sanger_qvs), int(qual_vector_offset),
                        int(qual_delta), bool(reset_stats))


def post_sw(read_words, initbp, dbalign, qralign, read_start, qual=None):
    """The single seam post_sw on a struct sw_full_results holding sw_full_cs's dbalign / qralign / read_start (host code, needs post_sw_setup; qual: the read's QV
    string, used when the setup got use_read_qvs).  Returns dict(posterior, matches, mismatches, crossovers, qralign, qual) -- what post_sw leaves in the struct."""
    L = lib()
    r = np.ascontiguousarray(read_words, dtype=np.uint32)
    b = lambda x: x if isinstance(x, bytes) else x.encode()
    db = C.create_string_buffer(b(dbalign)); qr = C.create_string_buffer(b(qralign))
    s = SwFullResults(); s.read_start = int(read_start); s.dbalign = C.addressof(db); s.qralign = C.addressof(qr)
    L.post_sw(r.ctypes.data_as(C.POINTER(C.c_uint32)), int(initbp), None if qual is None else b(qual), C.byref(s))
    q = C.string_at(s.qual).decode() if s.qual else ""
    if s.qual: L.gm_free(s.qual)
    return dict(posterior=s.posterior, matches=s.matches, mismatches=s.mismatches, crossovers=s.crossovers, qralign=qr.value.decode(), qual=q)


def post_sw_batch(recs, ops, genome_ls, reads_words, rlen, initbp, quals=None, is_rna=False):
    """gm_post_sw_batch: post_sw of every record of one sw_full_cs_batch call (recs, ops as it returned them; genome_ls, reads_words, rlen, initbp, is_rna as it was given
    them) in one call.  quals: None or n QV strings (bytes).  Returns (post: structured array of POST_REC_DTYPE, qralign: i -> the re-called qralign of item i,
    qual: i -> its base qualities), both strings as the single seam leaves them; an item that was refused has status < 0 (reason: gm_last_error)."""
    L = lib()
    rc_ = np.ascontiguousarray(recs, dtype=SW_FULL_REC_DTYPE); n = rc_.shape[0]
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    g = np.ascontiguousarray(genome_ls, dtype=np.uint32); r = np.ascontiguousarray(reads_words, dtype=np.uint32)
    if r.ndim != 2 or r.shape[0] != n: raise GmError("post_sw_batch: reads_words is (n, read_words)")
    rl = np.ascontiguousarray(rlen, dtype=np.int32); ib = np.ascontiguousarray(initbp, dtype=np.uint8)
    if rl.shape[0] != n or ib.shape[0] != n or (quals is not None and len(quals) != n): raise GmError("post_sw_batch: every per-item array has n entries")
    qp = None if quals is None else (C.c_char_p * max(n, 1))(*[None if q is None else (q if isinstance(q, bytes) else q.encode()) for q in quals])
    post = np.zeros(n, dtype=POST_REC_DTYPE); qa_p, qo_p, qo_len = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    dp = lambda a: None if a.size == 0 else a.ctypes.data
    _check(L.gm_post_sw_batch(n, dp(rc_), dp(o), o.size, g.ctypes.data_as(C.POINTER(C.c_uint32)), g.size, r.ctypes.data_as(C.POINTER(C.c_uint32)), r.shape[1],
                              rl.ctypes.data_as(C.POINTER(C.c_int)), dp(ib), qp, 1 if is_rna else 0, dp(post), C.byref(qa_p), C.byref(qo_p), C.byref(qo_len)), "gm_post_sw_batch")
    qa = C.string_at(qa_p.value, o.size) if qa_p.value else b""
    qo = C.string_at(qo_p.value, qo_len.value) if qo_p.value else b""
    L.gm_free(qa_p); L.gm_free(qo_p)
    def qralign(i):
        return qa[int(rc_[i]["ops_off"]):int(rc_[i]["ops_off"]) + int(rc_[i]["n_ops"])].decode() if post[i]["status"] == 0 and rc_[i]["score"] > 0 else None
    def qual(i):
        return qo[int(post[i]["qual_off"]):int(post[i]["qual_off"]) + int(post[i]["qual_len"])].decode()
    qralign.buffer = qa                                                  # the whole buffer (ops.size bytes): what sw_full_batch_text takes as qralign
    qual.buffer = qo                                                     # ... and the base qualities end to end: what Session.sam_records takes as post_quals
    return post, qralign, qual


TEXT_KINDS = {"align": 1, "cigar": 2, "edit": 4}      # GM_TEXT_ALIGN / GM_TEXT_CIGAR / GM_TEXT_EDIT


def _batch_text(call, name, colour, n, recs, ops, genome_args, reads_words, rlen, initbp, is_rna, qralign, reverse, clip, what):
    rc_ = np.ascontiguousarray(recs, dtype=SW_FULL_REC_DTYPE); o = np.ascontiguousarray(ops, dtype=np.uint8)
    bits = 0
    for k in ([what] if isinstance(what, str) else what): bits |= TEXT_KINDS[k]
    r = None if reads_words is None else np.ascontiguousarray(reads_words, dtype=np.uint32)
    if r is not None and (r.ndim != 2 or r.shape[0] != n): raise GmError("sw_full_batch_text: reads_words is (n, read_words)")
    rl = np.ascontiguousarray(rlen, dtype=np.int32)
    ib = None if initbp is None else np.ascontiguousarray(initbp, dtype=np.uint8)
    rv = None if reverse is None else np.ascontiguousarray(reverse, dtype=np.uint8)
    if rc_.shape[0] != n or any(a is not None and a.shape[0] != n for a in (rl, ib, rv)): raise GmError("sw_full_batch_text: every per-item array has n entries")
    qin = None
    if qralign is not None:
        qin = bytes(qralign)
        if len(qin) != o.size: raise GmError("sw_full_batch_text: qralign holds ops_len bytes (post_sw_batch's buffer)")
    status = np.zeros(n, dtype=np.int32)
    db_p, qr_p, cg_p, ed_p = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    coff = np.zeros(n + 1, dtype=np.uint64); eoff = np.zeros(n + 1, dtype=np.uint64)
    dp = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    _check(call(1 if colour else 0, bits, n, dp(rc_), dp(o), o.size, *genome_args, None if r is None else r.ctypes.data_as(C.POINTER(C.c_uint32)), 1 if r is None else r.shape[1],
                rl.ctypes.data_as(C.POINTER(C.c_int)), dp(ib), is_rna, qin, dp(rv), ord(clip), status.ctypes.data_as(C.POINTER(C.c_int)),
                C.byref(db_p), C.byref(qr_p), C.byref(cg_p), u64p(coff), C.byref(ed_p), u64p(eoff)), name)
    def take(p, size):
        b = C.string_at(p.value, size) if p.value and size else b""
        lib().gm_free(p)
        return b
    db, qr = take(db_p, o.size), take(qr_p, o.size)
    cg, ed = take(cg_p, int(coff[n])), take(ed_p, int(eoff[n]))
    answered = lambda i: status[i] == 0 and rc_[i]["score"] > 0
    def by_ops(buf): return lambda i: buf[int(rc_[i]["ops_off"]):int(rc_[i]["ops_off"]) + int(rc_[i]["n_ops"])] if answered(i) else b""
    def by_off(buf, off): return lambda i: buf[int(off[i]):int(off[i + 1])]
    fd, fq = (by_ops(db), by_ops(qr)) if bits & 1 else (None, None)
    fc = by_off(cg, coff) if bits & 2 else None
    fe = by_off(ed, eoff) if bits & 4 else None
    for f, buf, off in ((fd, db, None), (fq, qr, None), (fc, cg, coff), (fe, ed, eoff)):
        if f is not None: f.buffer = buf; f.offsets = off                      # the whole buffer and (CIGAR, edit string) its n + 1 offsets
    return status, fd, fq, fc, fe


def sw_full_batch_text(colour_space, recs, ops, genome_words, reads_words, rlen, initbp=None, is_rna=False, qralign=None, reverse=None, clip="S", what=("align", "cigar", "edit")):
    """gm_sw_full_batch_text: the text of every record of one sw_full_ls_batch / sw_full_cs_batch call (recs, ops as it returned them; genome_words, reads_words, rlen,
    initbp, is_rna as it was given them) in one call.  qralign: None or post_sw_batch's whole qralign buffer (ops.size bytes), used in place of the rebuilt one;
    reverse: None or n flags (the item is printed as a reverse-strand mapping); clip: "S" or "H"; what: kinds out of "align", "cigar", "edit".
    Returns (status, dbalign, qralign, cigar, edit): status is an int32 array (< 0: the item was refused, reason: gm_last_error), the others are i -> bytes for the
    kinds asked for (empty for an item without alignment) and None otherwise; each carries the whole buffer as .buffer and, CIGAR and edit string, .offsets."""
    g = np.ascontiguousarray(genome_words, dtype=np.uint32)
    n = np.asarray(recs).shape[0]
    return _batch_text(lib().gm_sw_full_batch_text, "gm_sw_full_batch_text", colour_space, n, recs, ops, [g.ctypes.data_as(C.POINTER(C.c_uint32)), g.size],
                       reads_words, rlen, initbp, 1 if is_rna else 0, qralign, reverse, clip, what)


def post_sw_batch_last_plan():
    """gm_post_sw_batch_last_plan (a diagnostic hook for tests, not stable surface): [(items, thread slots, columns of scratch a slot)] of the launches of this thread's last post_sw_batch call"""
    L = lib(); a, b, c = C.c_int(0), C.c_int(0), C.c_int(0); out = []
    for k in range(L.gm_post_sw_batch_last_plan(-1, None, None, None)):
        L.gm_post_sw_batch_last_plan(k, C.byref(a), C.byref(b), C.byref(c)); out.append((a.value, b.value, c.value))
    return out


def seam_stats(which):
    """(invocations, cells, seconds) of this thread's sw_vector / sw_full_ls / sw_full_cs / post_sw calls (ref: the *_stats functions gmapper.c:734-745 reads)."""
    L = lib()
    if which == "sw_gapless":                                 # (invocations, cells, ns): three integers, as sw-gapless.h:12 declares them
        inv, cells, ticks = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.sw_gapless_stats.restype = None
        L.sw_gapless_stats(C.byref(inv), C.byref(cells), C.byref(ticks))
        return inv.value, cells.value, ticks.value
    inv, cells, secs = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
    fn = getattr(L, {"sw_vector": "sw_vector_stats", "sw_full_ls": "sw_full_ls_stats", "sw_full_cs": "sw_full_cs_stats", "post_sw": "post_sw_stats"}[which])
    fn.restype = None if which != "post_sw" else C.c_int
    fn(C.byref(inv), C.byref(cells), C.byref(secs))
    return inv.value, cells.value, secs.value


def sequence_to_bitfield(text, colour_space: bool = False):
    """fasta_sequence_to_bitfield (ref: common/fasta.c:609-673) through the library: returns (uint32 words, primer letter code or None)."""
    t = text if isinstance(text, bytes) else text.encode()
    n = len(t) - (1 if colour_space else 0)
    words = np.zeros(max(1, (n + 7) // 8), dtype=np.uint32); b = C.c_int(0)
    _check(lib().gm_sequence_to_bitfield(int(colour_space), t, len(t), words.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(b)), "gm_sequence_to_bitfield")
    return words, (b.value if colour_space else None)
