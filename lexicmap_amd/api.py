"""ctypes view of include/lexicmap_hip.h.  No compute happens in Python and there is no fallback: if the HIP library is
missing or no GPU is present the calls raise."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(HERE, "liblexicmap_hip.so")
# LEXICMAP_HIP_LIB=<path>: another build of the same C-ABI (an experiment from experiments/, an A-B build) instead of the in-tree
# library; said on stderr so that no measurement is attributed to the wrong sources
if os.environ.get("LEXICMAP_HIP_LIB"):
    LIB_PATH = os.path.abspath(os.environ["LEXICMAP_HIP_LIB"])
    import sys as _sys
    print("[lexicmap_amd] library override: %s" % LIB_PATH, file=_sys.stderr)


class HipLibraryMissing(RuntimeError):
    pass


class Options(C.Structure):
    _fields_ = [("min_prefix", C.c_int32), ("min_single_prefix", C.c_int32), ("top_n_genomes", C.c_int32),
                ("top_n_chains", C.c_int32), ("max_gap", C.c_double), ("max_distance", C.c_double),
                ("ext_len", C.c_int32), ("ext_len2", C.c_int32), ("min_qcov_per_genome", C.c_double),
                ("max_evalue", C.c_double), ("output_seq", C.c_int32), ("align_max_gap", C.c_int32),
                ("align_band", C.c_int32), ("align_min_match_len", C.c_int32), ("align_min_pident", C.c_double),
                ("min_qcov_per_hsp", C.c_double), ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
                ("total_bases_override", C.c_int64)]


class IndexInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("masks", C.c_int32), ("mask_prefix", C.c_int32), ("anchor_prefix", C.c_int32),
                ("total_bases", C.c_int64), ("genomes", C.c_int64), ("seeds", C.c_int64), ("genome_bases", C.c_int64),
                ("hbm_bytes", C.c_int64), ("seed_bytes", C.c_int64), ("outlier_seeds", C.c_int64),
                ("key_bits", C.c_int32), ("val_bits", C.c_int32), ("partition_bases", C.c_int32), ("pad", C.c_int32)]


class Query(C.Structure):
    _fields_ = [("seq", C.c_char_p), ("len", C.c_uint32)]


class Hsp(C.Structure):
    _fields_ = [("query", C.c_uint32), ("hits", C.c_uint32), ("batch_genome", C.c_uint64), ("qcov_genome", C.c_double),
                ("cls", C.c_int32), ("hsp", C.c_int32), ("seq_idx", C.c_int32), ("nseqs", C.c_int32),
                ("seq_len", C.c_int32), ("nchunks", C.c_int32), ("chunk_idx", C.c_int32), ("rc", C.c_int32),
                ("qcov_hsp", C.c_double), ("aligned_length", C.c_int32), ("pident", C.c_double), ("gaps", C.c_int32),
                ("qbegin", C.c_int32), ("qend", C.c_int32), ("tbegin", C.c_int32), ("tend", C.c_int32),
                ("evalue", C.c_double), ("bitscore", C.c_int32), ("score", C.c_int32), ("matched_bases", C.c_int32),
                ("genome_id", C.c_char_p), ("seq_id", C.c_char_p), ("cigar", C.c_char_p), ("qseq", C.c_char_p),
                ("sseq", C.c_char_p), ("align", C.c_char_p)]


class StageStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("query_bases", "query_kmers", "seed_lookups", "seed_values", "anchors_raw",
                                         "genome_pairs", "anchors_cleared", "chains", "window_bases", "pa_anchors",
                                         "hsps_aligned", "wfa_retries", "rows", "aligned_bases")] + \
               [(n, C.c_double) for n in ("ms_mask", "ms_lookup", "ms_chain", "ms_window", "ms_pseudo", "ms_glue",
                                          "ms_extend_wfa", "ms_finalize", "ms_total")]


class Anchor(C.Structure):
    _fields_ = [("qbegin", C.c_int32), ("tbegin", C.c_int32), ("len", C.c_uint8), ("trc", C.c_uint8),
                ("qrc", C.c_uint8), ("pad", C.c_uint8)]


class Pair(C.Structure):
    _fields_ = [("query", C.c_uint32), ("batch_genome", C.c_uint64), ("raw_off", C.c_int64), ("raw_n", C.c_int64),
                ("clr_off", C.c_int64), ("clr_n", C.c_int64), ("score", C.c_float), ("chain_off", C.c_int64),
                ("chain_n", C.c_int64)]


class Chain2(C.Structure):
    _fields_ = [("qbegin", C.c_int32), ("qend", C.c_int32), ("tbegin", C.c_int32), ("tend", C.c_int32),
                ("nanchors", C.c_int32), ("matched_bases", C.c_int32), ("aligned_bases_q", C.c_int32),
                ("aligned_bases_t", C.c_int32), ("pident", C.c_double)]


LM_ERR_OPTION, LM_ERR_ARG = 3, 7  # lm_status
REFUSED_ARG = (LM_ERR_ARG,)                    # calls without an option check
REFUSED_ARG_OR_OPTION = (LM_ERR_OPTION, LM_ERR_ARG)


def _check(st, text, fmt="liblexicmap_hip error %(status)d: %(text)s", refused=()):
    """The one place a status of the library becomes an exception; returns when st is 0.  text: the library's error text, or a
    callable that fetches it (called only for a failure).  refused: the statuses by which this call refuses the caller's
    argument or option - they raise ValueError with the bare text.  Every other status raises RuntimeError with
    fmt % {"status": st, "text": text}.  The exception carries the status as e.status."""
    if st == 0:
        return
    if callable(text):
        text = text()
    e = ValueError(text) if st in refused else RuntimeError(fmt % {"status": st, "text": text})
    e.status = st
    raise e


def _global_error():
    return lib().lm_last_error(None).decode()


class PaRegion(C.Structure):
    """lm_pa_region: one window of a resident genome for Index.pseudoalign_regions"""
    _fields_ = [("query", C.c_uint32), ("qbegin", C.c_uint32), ("qend", C.c_uint32), ("rc", C.c_int32),
                ("local_genome", C.c_int64), ("tbegin", C.c_int32), ("wlen", C.c_int32)]


class Wfa(C.Structure):
    _fields_ = [("status", C.c_int32), ("score", C.c_int32), ("qbegin", C.c_int32), ("qend", C.c_int32),
                ("tbegin", C.c_int32), ("tend", C.c_int32), ("align_len", C.c_uint32), ("matches", C.c_uint32),
                ("gaps", C.c_uint32), ("gap_regions", C.c_uint32), ("ops_off", C.c_int64), ("nops", C.c_int32)]


class SynthSpec(C.Structure):
    _fields_ = [("k", C.c_int32), ("masks", C.c_int32), ("mask_seed", C.c_int64), ("genomes", C.c_int64),
                ("genome_len", C.c_int32), ("families", C.c_int32), ("max_div", C.c_double), ("seed", C.c_int64),
                ("max_desert", C.c_int32), ("seed_dist", C.c_int32)]


class BuildOpt(C.Structure):
    """lm_build_opt: the settings of `lexicmap index` that Index.from_genomes honours (BuildOpt.default(): its defaults)"""
    _fields_ = [("k", C.c_int32), ("masks", C.c_int32), ("mask_seed", C.c_int64), ("max_desert", C.c_int32),
                ("seed_dist", C.c_int32), ("contig_interval", C.c_int32), ("genome_batch_size", C.c_int32),
                ("max_genome", C.c_int32)]

    @classmethod
    def default(cls, **kw):
        o = cls()
        lib().lm_build_opt_default(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


class Contig(C.Structure):
    _fields_ = [("id", C.c_char_p), ("seq", C.c_char_p), ("len", C.c_uint32)]


GENOMES_AUTO, GENOMES_DEVICE, GENOMES_HOST = 0, 1, 2  # lm_residency.genomes


class Residency(C.Structure):
    """lm_residency: where the 2-bit genomes live (HBM, pinned host memory, or HBM up to a byte budget)"""
    _fields_ = [("genomes", C.c_int32), ("pad", C.c_int32), ("genome_hbm_bytes", C.c_int64)]

    def __init__(self, genomes=GENOMES_AUTO, genome_hbm_bytes=0):
        super().__init__(genomes, 0, genome_hbm_bytes)


class ResidencyInfo(C.Structure):
    _fields_ = [("genomes_device", C.c_int64), ("genomes_host", C.c_int64), ("genome_bytes_device", C.c_int64),
                ("genome_bytes_host", C.c_int64), ("stage_bytes", C.c_int64)]


class SeedDistOpt(C.Structure):
    _fields_ = [("min_dist", C.c_uint32), ("hist_bins", C.c_uint32), ("hist_width", C.c_uint32), ("pad", C.c_uint32)]


class SeedDistRec(C.Structure):
    _fields_ = [("key", C.c_uint64), ("seeds", C.c_int64), ("max_dist", C.c_uint32), ("max_dist_pos", C.c_uint32),
                ("contigs", C.c_int32), ("contigs_without_seeds", C.c_int32)]


class SeedDistRow(C.Structure):
    _fields_ = [("record", C.c_uint32), ("contig", C.c_uint32), ("pos", C.c_uint32), ("pos_in_contig", C.c_uint32),
                ("strand", C.c_uint32), ("dist", C.c_uint32)]


class ScreenOpt(C.Structure):
    _fields_ = [("min_prefix", C.c_int32), ("windows", C.c_int32), ("top_n", C.c_int32), ("details", C.c_int32)]


class GenomeQuery(C.Structure):
    _fields_ = [("id", C.c_char_p), ("contigs", C.POINTER(Contig)), ("ncontigs", C.c_size_t)]


class ScreenRow(C.Structure):
    _fields_ = [("query", C.c_uint32), ("nkeys", C.c_uint32), ("score", C.c_uint64), ("batch_genome", C.c_uint64),
                ("genome_id", C.c_char_p), ("keys_off", C.c_uint64), ("score2", C.c_uint64), ("hit_masks", C.c_uint32),
                ("pad", C.c_uint32), ("hit_kmers", C.c_uint64), ("prefixes_off", C.c_uint64)]


class ScreenStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("query_bases", "windows", "lookups", "tuples", "pieces")] + \
               [(n, C.c_double) for n in ("ms_capture", "ms_lookup", "ms_reduce", "ms_total")]


class PairOpt(C.Structure):
    _fields_ = [("min_prefix", C.c_int32), ("masks", C.c_int32), ("min_mask_fraction", C.c_double)]


class PairRow(C.Structure):
    _fields_ = [("key1", C.c_uint64), ("key2", C.c_uint64), ("genome1", C.c_char_p), ("genome2", C.c_char_p),
                ("n_masks", C.c_uint32), ("sum_prefix", C.c_uint32)]


class PairStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("total_masks", "required", "entries", "tuples", "pieces", "pairs_seen", "rows")] + \
               [(n, C.c_double) for n in ("ms_entries", "ms_emit", "ms_reduce", "ms_total")]


REGION_BY_NAME = (1 << 64) - 1   # LM_REGION_BY_NAME
SUBSEQ_OK, SUBSEQ_NO_GENOME, SUBSEQ_NO_SEQ, SUBSEQ_OUT_OF_RANGE, SUBSEQ_NOT_LOCAL = range(5)


class Region(C.Structure):
    _fields_ = [("key", C.c_uint64), ("genome_id", C.c_char_p), ("seq_id", C.c_char_p), ("seq_idx", C.c_int32),
                ("rc", C.c_int32), ("begin", C.c_int64), ("end", C.c_int64)]


class SubseqOpt(C.Structure):
    _fields_ = [("upstream", C.c_int32), ("downstream", C.c_int32), ("ignore_errors", C.c_int32), ("pad", C.c_int32)]


class SubseqInfo(C.Structure):
    _fields_ = [("key", C.c_uint64), ("seq_idx", C.c_int32), ("status", C.c_int32), ("rc", C.c_int32), ("pad", C.c_int32),
                ("begin", C.c_int64), ("end", C.c_int64), ("off", C.c_int64), ("len", C.c_int64),
                ("genome_id", C.c_char_p), ("seq_id", C.c_char_p)]


class SubseqStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("regions", "answered", "bases", "blob_bytes", "pieces")] + \
               [(n, C.c_double) for n in ("ms_plan", "ms_alloc", "ms_device", "ms_total")]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_int64), ("total_ms", C.c_double), ("bytes", C.c_int64)]


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of the in-tree shared library (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h"))]
    srcs.append(os.path.join(os.path.dirname(HERE), "include", "lexicmap_hip.h"))
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing("lexicmap_amd/liblexicmap_hip.so is missing: run __graft_entry__.build() "
                                "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.lm_options_default.argtypes = [C.POINTER(Options)]
    L.lm_index_open.argtypes = [C.c_char_p, C.POINTER(Options), C.c_int, C.POINTER(vp)]
    L.lm_index_open_ex.argtypes = [C.c_char_p, C.POINTER(Options), C.POINTER(Residency), C.c_int, C.POINTER(vp)]
    L.lm_index_build_synthetic_ex.argtypes = [C.POINTER(SynthSpec), C.POINTER(Options), C.POINTER(Residency), C.c_int,
                                              C.POINTER(vp)]
    L.lm_index_get_residency.argtypes = [vp, C.POINTER(ResidencyInfo)]
    L.lm_build_opt_default.argtypes = [C.POINTER(BuildOpt)]
    L.lm_build_opt_default.restype = None
    L.lm_index_builder_new.argtypes = [C.POINTER(BuildOpt), C.POINTER(Options), C.POINTER(Residency), C.c_int, C.POINTER(vp)]
    L.lm_index_builder_new_masks.argtypes = [C.POINTER(BuildOpt), C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(Options),
                                             C.POINTER(Residency), C.c_int, C.POINTER(vp)]
    L.lm_index_builder_extend.argtypes = [vp, C.POINTER(BuildOpt), C.POINTER(Residency), C.POINTER(vp)]
    L.lm_index_builder_like.argtypes = [vp, C.POINTER(BuildOpt), C.POINTER(Residency), C.POINTER(vp)]
    L.lm_index_builder_add_index.argtypes = [vp, vp, C.POINTER(C.c_uint64), C.c_size_t]
    L.lm_index_builder_add.argtypes = [vp, C.c_char_p, C.POINTER(Contig), C.c_size_t]
    L.lm_index_builder_finish.argtypes = [vp, C.POINTER(vp)]
    L.lm_index_builder_free.argtypes = [vp]
    L.lm_index_builder_free.restype = None
    L.lm_index_builder_last_error.argtypes = [vp]
    L.lm_index_builder_last_error.restype = C.c_char_p
    L.lm_index_close.argtypes = [vp]
    L.lm_index_get_info.argtypes = [vp, C.POINTER(IndexInfo)]
    L.lm_index_masks.argtypes = [vp]
    L.lm_index_masks.restype = C.POINTER(C.c_uint64)
    L.lm_last_error.argtypes = [vp]
    L.lm_last_error.restype = C.c_char_p
    L.lm_qbatch_upload.argtypes = [vp, C.POINTER(Query), C.c_size_t, C.POINTER(vp)]
    L.lm_qbatch_free.argtypes = [vp]
    L.lm_search_resident.argtypes = [vp, vp, C.POINTER(vp)]
    L.lm_search_batch.argtypes = [vp, C.POINTER(Query), C.c_size_t, C.POINTER(vp)]
    L.lm_result_rows.argtypes = [vp, C.POINTER(C.POINTER(Hsp))]
    L.lm_result_rows.restype = C.c_size_t
    L.lm_result_stats.argtypes = [vp, C.POINTER(StageStats)]
    L.lm_result_free.argtypes = [vp]
    L.lm_format_row.argtypes = [C.POINTER(Hsp), C.c_char_p, C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
    L.lm_stage_free.argtypes = [vp]
    L.lm_mask_batch.argtypes = [vp, C.POINTER(Query), C.c_size_t, C.POINTER(vp), C.POINTER(C.POINTER(C.c_uint64)),
                                C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(C.c_int32))]
    L.lm_seed_chain_batch.argtypes = [vp, C.POINTER(Query), C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t),
                                      C.POINTER(C.POINTER(Pair)), C.POINTER(C.POINTER(Anchor)),
                                      C.POINTER(C.POINTER(Anchor)), C.POINTER(C.POINTER(C.c_int64)),
                                      C.POINTER(C.POINTER(C.c_int32))]
    L.lm_pseudoalign_batch.argtypes = [vp, C.POINTER(Query), C.c_size_t, C.POINTER(Query), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(vp),
                                       C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(Chain2))]
    L.lm_pseudoalign_batch_ex.argtypes = L.lm_pseudoalign_batch.argtypes + [C.POINTER(C.POINTER(C.c_int64)),
                                                                            C.POINTER(C.POINTER(Anchor))]
    L.lm_pseudoalign_regions.argtypes = [vp, C.POINTER(Query), C.c_size_t, C.POINTER(PaRegion), C.c_size_t, C.POINTER(vp),
                                         C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(Chain2)),
                                         C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(Anchor))]
    L.lm_wfa_batch.argtypes = [vp, C.POINTER(Query), C.POINTER(Query), C.c_size_t, C.POINTER(vp),
                               C.POINTER(C.POINTER(Wfa)), C.POINTER(C.POINTER(C.c_uint64))]
    L.lm_index_build_synthetic.argtypes = [C.POINTER(SynthSpec), C.POINTER(Options), C.c_int, C.POINTER(vp)]
    L.lm_merge_sharded.argtypes = [vp, C.POINTER(C.POINTER(Hsp)), C.POINTER(C.c_size_t), C.c_int, C.POINTER(vp)]
    L.lm_search_scores.argtypes = [vp, vp, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(C.c_uint32)),
                                   C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_float))]
    L.lm_topn_merge.argtypes = [C.c_int, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint64)),
                                C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_size_t), C.c_int,
                                C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_size_t)]
    L.lm_search_resident_keep.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(vp)]
    L.lm_free.argtypes = [vp]
    L.lm_index_set_genome_filter.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t]
    L.lm_index_mask_seeds.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t,
                                      C.POINTER(C.c_size_t)]
    L.lm_index_seed_positions.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(vp)]
    L.lm_seedpos_get.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_int64)),
                                 C.POINTER(C.POINTER(C.c_uint32))]
    L.lm_seedpos_get.restype = C.c_size_t
    L.lm_seedpos_free.argtypes = [vp]
    L.lm_seedpos_free.restype = None
    L.lm_index_seed_distances.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(SeedDistOpt), C.POINTER(vp)]
    L.lm_seed_dist_records.argtypes = [vp, C.POINTER(C.POINTER(SeedDistRec))]
    L.lm_seed_dist_records.restype = C.c_size_t
    L.lm_seed_dist_hist.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64))]
    L.lm_seed_dist_hist.restype = C.c_size_t
    L.lm_seed_dist_rows.argtypes = [vp, C.POINTER(C.POINTER(SeedDistRow))]
    L.lm_seed_dist_rows.restype = C.c_size_t
    L.lm_seed_dist_free.argtypes = [vp]
    L.lm_seed_dist_free.restype = None
    L.lm_screen_opt_default.argtypes = [C.POINTER(ScreenOpt)]
    L.lm_screen_opt_default.restype = None
    L.lm_index_screen_genomes.argtypes = [vp, C.POINTER(GenomeQuery), C.c_size_t, C.POINTER(ScreenOpt), C.POINTER(vp)]
    L.lm_screen_rows.argtypes = [vp, C.POINTER(C.POINTER(ScreenRow))]
    L.lm_screen_rows.restype = C.c_size_t
    L.lm_screen_keys.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint64))]
    L.lm_screen_keys.restype = C.c_size_t
    L.lm_screen_prefixes.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint8))]
    L.lm_screen_prefixes.restype = C.c_size_t
    L.lm_screen_get_stats.argtypes = [vp, C.POINTER(ScreenStats)]
    L.lm_screen_get_stats.restype = None
    L.lm_screen_free.argtypes = [vp]
    L.lm_screen_free.restype = None
    L.lm_format_screen_row.argtypes = [C.POINTER(ScreenRow), C.POINTER(C.c_uint8), C.c_char_p, C.c_int, C.c_int, C.c_int,
                                       C.c_char_p, C.c_size_t]
    L.lm_screen_header.argtypes = [C.c_int]
    L.lm_screen_header.restype = C.c_char_p
    L.lm_pair_opt_default.argtypes = [C.POINTER(PairOpt)]
    L.lm_pair_opt_default.restype = None
    L.lm_index_genome_pairs.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(PairOpt), C.POINTER(vp)]
    L.lm_pairs_rows.argtypes = [vp, C.POINTER(C.POINTER(PairRow))]
    L.lm_pairs_rows.restype = C.c_size_t
    L.lm_pairs_get_stats.argtypes = [vp, C.POINTER(PairStats)]
    L.lm_pairs_get_stats.restype = None
    L.lm_pairs_free.argtypes = [vp]
    L.lm_pairs_free.restype = None
    L.lm_format_pair_row.argtypes = [C.POINTER(PairRow), C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.lm_pair_header.argtypes = []
    L.lm_pair_header.restype = C.c_char_p
    L.lm_index_pair_seeds.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(PairOpt), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.lm_index_genome_pairs_across.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t,
                                               C.POINTER(PairOpt), C.POINTER(vp)]
    L.lm_pairs_from_rows.argtypes = [C.POINTER(PairRow), C.c_size_t, C.POINTER(PairStats), C.POINTER(vp)]
    L.lm_pairs_merge.argtypes = [C.POINTER(vp), C.c_size_t, C.POINTER(vp)]
    L.lm_subseq_opt_default.argtypes = [C.POINTER(SubseqOpt)]
    L.lm_subseq_opt_default.restype = None
    L.lm_index_subseqs.argtypes = [vp, C.POINTER(Region), C.c_size_t, C.POINTER(SubseqOpt), C.POINTER(vp)]
    L.lm_index_subseq_rows.argtypes = [vp, C.POINTER(Hsp), C.c_size_t, C.POINTER(SubseqOpt), C.POINTER(vp)]
    L.lm_index_genome_seqs.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.lm_subseqs_get.argtypes = [vp, C.POINTER(C.POINTER(SubseqInfo)), C.POINTER(vp)]
    L.lm_subseqs_get.restype = C.c_size_t
    L.lm_subseqs_get_stats.argtypes = [vp, C.POINTER(SubseqStats)]
    L.lm_subseqs_get_stats.restype = None
    L.lm_subseqs_free.argtypes = [vp]
    L.lm_subseqs_free.restype = None
    L.lm_format_subseqs.argtypes = [vp, C.POINTER(Hsp), C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_size_t, C.c_int,
                                    C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.lm_index_screen_structure.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.lm_index_screen_add_structure.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.lm_index_fetch.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, C.c_char_p]
    L.lm_index_save.argtypes = [vp, C.c_char_p, C.c_int]
    L.lm_profile_enable.argtypes = [vp, C.c_int]
    L.lm_profile_reset.argtypes = [vp]
    L.lm_profile_exclusive.argtypes = [vp, C.c_int]
    L.lm_format_rows.argtypes = [C.POINTER(Hsp), C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_size_t, C.c_int,
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.lm_free.argtypes = [vp]
    L.lm_free.restype = None
    L.lm_profile_mark.argtypes = [vp, C.c_int]
    L.lm_profile_mark.restype = None
    L.lm_tuning_reload.argtypes = [vp]
    L.lm_tuning_reload.restype = None
    L.lm_profile_get.argtypes = [vp, C.POINTER(C.POINTER(KernelTime))]
    L.lm_profile_get.restype = C.c_size_t
    L.lm_comm_unique_id.argtypes = [C.c_char_p]
    L.lm_comm_init.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.lm_comm_free.argtypes = [vp]
    L.lm_comm_free.restype = None
    L.lm_comm_rank.argtypes = [vp]
    L.lm_comm_size.argtypes = [vp]
    L.lm_comm_last_error.argtypes = [vp]
    L.lm_comm_last_error.restype = C.c_char_p
    L.lm_gather_rows.argtypes = [vp, C.POINTER(Hsp), C.c_size_t, C.c_int, C.POINTER(C.POINTER(Hsp)), C.POINTER(C.c_size_t)]
    L.lm_gather_merge_rows.argtypes = [vp, vp, C.POINTER(Hsp), C.c_size_t, C.c_int, C.POINTER(C.POINTER(Hsp)), C.POINTER(C.c_size_t)]
    L.lm_merge_sharded_device.argtypes = [vp, vp, vp, C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.POINTER(Hsp)), C.POINTER(C.c_size_t)]
    L.lm_merge_sharded_ex.argtypes = [vp, C.POINTER(C.POINTER(Hsp)), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(vp)]
    L.lm_gather_rows_ex.argtypes = [vp, C.POINTER(Hsp), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.POINTER(Hsp)), C.POINTER(C.c_size_t)]
    L.lm_gather_merge_rows_ex.argtypes = [vp, vp, C.POINTER(Hsp), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.POINTER(Hsp)),
                                          C.POINTER(C.c_size_t)]
    L.lm_merge_sharded_device_ex.argtypes = [vp, vp, vp, C.POINTER(C.c_size_t), vp, C.c_uint64, C.c_int, C.c_int,
                                             C.POINTER(C.POINTER(Hsp)), C.POINTER(C.c_size_t)]
    L.lm_tsv_header.argtypes = [C.c_int]
    L.lm_tsv_header.restype = C.c_char_p
    _lib = L
    return L


def _queries(seqs):
    arr = (Query * max(len(seqs), 1))()
    keep = []
    for i, s in enumerate(seqs):
        b = bytes(s)
        keep.append(b)
        arr[i].seq = b
        arr[i].len = len(b)
    return arr, keep


def default_options(**kw):
    o = Options()
    lib().lm_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class Index:
    """lm_index handle (replaces cmd.NewIndexSearcher / Index.Search / Index.Close of the reference)."""

    def __init__(self, path, options=None, device=0, _handle=None, residency=None):
        """residency: a Residency (lm_index_open_ex); None makes the plain lm_index_open call"""
        L = lib()
        self.opt = options or default_options()
        if _handle is not None:
            self.h = _handle
            return
        h = C.c_void_p()
        if residency is None:
            st = L.lm_index_open(path.encode(), C.byref(self.opt), device, C.byref(h))
        else:
            st = L.lm_index_open_ex(path.encode(), C.byref(self.opt), C.byref(residency), device, C.byref(h))
        _check(st, _global_error, "lm_index_open failed (%(status)d): %(text)s")
        self.h = h

    @classmethod
    def synthetic(cls, genomes, genome_len, families, seed=1000, max_div=0.10, masks=20000, options=None, device=0,
                  residency=None):
        """genomes + seed index generated directly in HBM by lm_index_build_synthetic (bench input); residency as in
        __init__ (the genomes beyond the device budget move to pinned host memory once the set is built)"""
        L = lib()
        opt = options or default_options()
        sp = SynthSpec(31, masks, 1, genomes, genome_len, families, max_div, seed, 100, 50)
        h = C.c_void_p()
        if residency is None:
            st = L.lm_index_build_synthetic(C.byref(sp), C.byref(opt), device, C.byref(h))
        else:
            st = L.lm_index_build_synthetic_ex(C.byref(sp), C.byref(opt), C.byref(residency), device, C.byref(h))
        _check(st, _global_error, "lm_index_build_synthetic failed (%(status)d): %(text)s")
        return cls(None, opt, device, _handle=h)

    @classmethod
    def from_genomes(cls, genomes, build_opt=None, options=None, device=0, residency=None, masks=None):
        """index built on the GPU from caller-supplied genomes (lm_index_builder_*): genomes is a list of
        (genome_id, [(contig_id, seq bytes), ...]); build_opt a BuildOpt (None: the defaults of `lexicmap index`); residency as
        in __init__.  A genome the builder refuses (LM_ERR_ARG: a contig longer than max_genome, a record shorter than k)
        raises ValueError with the builder's text; nothing of it is added.  masks: the mask set to build with, as in
        IndexBuilder (None: the set generated from build_opt.mask_seed)."""
        b = IndexBuilder(build_opt, options, device, residency, masks)
        try:
            for gid, contigs in genomes:
                b.add(gid, contigs)
            return b.finish()
        finally:
            b.close()

    def extend(self, genomes, build_opt=None, residency=None):
        """a NEW Index holding this one's genomes followed by `genomes` (lm_index_builder_extend): what one from_genomes build
        of all of them with this index's masks gives, without capturing this index's genomes again.  self stays open and
        unchanged.  build_opt None: the settings this index was built with; genomes and residency as in from_genomes."""
        b = IndexBuilder.extending(self, build_opt, residency)
        try:
            for gid, contigs in genomes:
                b.add(gid, contigs)
            return b.finish()
        finally:
            b.close()

    def join(self, *others, build_opt=None, residency=None):
        """a NEW Index holding this one's genomes followed by those of every Index in `others`, in that order
        (lm_index_builder_extend + lm_index_builder_add_index): what one from_genomes build of all of them gives, without
        capturing any genome again.  All inputs share this index's masks, k and contig interval, are unsharded and on one
        device; they stay open and unchanged.  build_opt and residency as in extend."""
        b = IndexBuilder.extending(self, build_opt, residency)
        try:
            for o in others:
                b.add_index(o)
            return b.finish()
        finally:
            b.close()

    def subset(self, keep_keys, build_opt=None, residency=None):
        """a NEW Index holding the records of this one whose keys (batch << 17 | index) are in keep_keys, in this index's
        order and numbered from 0 (lm_index_builder_like + lm_index_builder_add_index): what one from_genomes build of those
        genomes gives.  A split genome is kept with all of its records or none.  self stays open and unchanged."""
        b = IndexBuilder.like(self, build_opt, residency)
        try:
            b.add_index(self, keep_keys)
            return b.finish()
        finally:
            b.close()

    def residency(self):
        """lm_index_get_residency: genomes and 2-bit bytes on the device / in pinned host memory, staging bytes held"""
        r = ResidencyInfo()
        st = lib().lm_index_get_residency(self.h, C.byref(r))
        self._err(st)
        return {f[0]: getattr(r, f[0]) for f in ResidencyInfo._fields_}

    def save(self, path, chunks=16):
        """the resident index written in the reference's on-disk format (lm_index_save)"""
        st = lib().lm_index_save(self.h, path.encode(), chunks)
        self._err(st)

    def fetch(self, local_genome, start, length):
        buf = C.create_string_buffer(length)
        st = lib().lm_index_fetch(self.h, local_genome, start, length, buf)
        self._err(st)
        return buf.raw

    def close(self):
        if self.h:
            lib().lm_index_close(self.h)
            self.h = None

    def _err(self, st, refused=()):
        """raises for a status other than 0 of a call on this handle, with the handle's error text (_check)"""
        _check(st, lambda: lib().lm_last_error(self.h).decode(), refused=refused)

    def info(self):
        i = IndexInfo()
        lib().lm_index_get_info(self.h, C.byref(i))
        return {f[0]: getattr(i, f[0]) for f in IndexInfo._fields_}

    def masks(self):
        """the masks of the handle (lm_index_masks) as a numpy uint64 copy: what IndexBuilder(masks=...) and write_mask_file take"""
        import numpy as np
        M = self.info()["masks"]
        p = lib().lm_index_masks(self.h)
        return np.ctypeslib.as_array(p, shape=(M,)).astype(np.uint64, copy=True)

    def mask_seeds(self, mask):
        """(k-mers, values) stored under one mask as numpy uint64 arrays (reference value layout)"""
        import numpy as np
        n = C.c_size_t()
        st = lib().lm_index_mask_seeds(self.h, mask, None, None, 0, C.byref(n))
        self._err(st)
        k = np.zeros(max(n.value, 1), dtype=np.uint64)
        v = np.zeros(max(n.value, 1), dtype=np.uint64)
        st = lib().lm_index_mask_seeds(self.h, mask, k.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       v.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n))
        self._err(st)
        return k[:n.value], v[:n.value]

    @staticmethod
    def _record_keys(keys):
        if keys is None:
            return None, 0
        ks = [int(k) for k in keys]
        return (C.c_uint64 * max(len(ks), 1))(*ks), len(ks)

    def seed_positions(self, keys=None):
        """lm_index_seed_positions: per selected record (keys: record keys batch << 17 | index in any order; None: every
        record of this handle in record order) the sorted list of its forward seeds as a numpy uint32 array of
        pos << 1 | strand - extracted, sorted and cut on the GPU.  ValueError for a key that is no record of this handle
        (another shard's among them) or is given twice; an empty list of keys gives an empty list."""
        import numpy as np
        L = lib()
        arr, n = self._record_keys(keys)
        sp = C.c_void_p()
        st = L.lm_index_seed_positions(self.h, arr, n, C.byref(sp))
        self._err(st, REFUSED_ARG)
        try:
            off, locs = C.POINTER(C.c_int64)(), C.POINTER(C.c_uint32)()
            nrec = L.lm_seedpos_get(sp, None, C.byref(off), C.byref(locs))
            o = np.ctypeslib.as_array(off, shape=(nrec + 1,))
            a = np.ctypeslib.as_array(locs, shape=(int(o[nrec]),)).copy() if o[nrec] else np.zeros(0, np.uint32)
            return [a[o[s]:o[s + 1]] for s in range(nrec)]
        finally:
            L.lm_seedpos_free(sp)

    def seed_distances(self, keys=None, min_dist=0, bins=0, bin_width=0):
        """lm_index_seed_distances: the distances between consecutive seeds of the selected records (keys as in
        seed_positions), computed on the GPU.  -> dict of numpy arrays: `records` (one per selected record: key, seeds,
        max_dist, max_dist_pos, contigs, contigs_without_seeds), `hist` (bins counters of bin_width over the reported
        distances, the last one open-ended) and `rows` (record slot, contig, pos, pos_in_contig, strand, dist of every
        position with dist >= min_dist, in selection and position order: the lines of `lexicmap utils seed-pos -D`).
        ValueError as seed_positions, and for bins > 0 with bin_width < 1."""
        import numpy as np
        L = lib()
        arr, n = self._record_keys(keys)
        opt = SeedDistOpt(min_dist, bins, bin_width, 0)
        sd = C.c_void_p()
        st = L.lm_index_seed_distances(self.h, arr, n, C.byref(opt), C.byref(sd))
        self._err(st, REFUSED_ARG)
        try:
            def take(fn, ctype, dtype):
                p = C.POINTER(ctype)()
                k = fn(sd, C.byref(p))
                if not k:
                    return np.zeros(0, dtype)
                return np.frombuffer(C.string_at(p, k * C.sizeof(ctype)), dtype=dtype)
            return dict(records=take(L.lm_seed_dist_records, SeedDistRec, np.dtype(SeedDistRec)),
                        hist=take(L.lm_seed_dist_hist, C.c_uint64, np.uint64),
                        rows=take(L.lm_seed_dist_rows, SeedDistRow, np.dtype(SeedDistRow)))
        finally:
            L.lm_seed_dist_free(sd)

    def screen(self, genomes, min_prefix=21, windows=1, top_n=10, details=False, want_stats=False):
        """lm_index_screen_genomes: which genomes of the index are closest to each query genome - the screening stage of
        `lexicmap genome search` (-S), computed on the GPU.  genomes: [(genome_id, [(contig_id, seq bytes), ...]), ...] as
        from_genomes takes them.  -> per query a list of rows (dicts) in output order: score, batch_genome (the lowest key),
        genome_id, keys (the hit records of the genome, ascending: what set_genome_filter takes), and with details score2,
        hit_masks, hit_kmers and prefixes (the longest match under every hit mask, descending); without details those are
        0 and [].  top_n = 0 keeps all rows.  ValueError for what the library refuses as an argument or option (windows < 1,
        a query without contigs or of 2^28 bases or more, min_prefix out of range).  want_stats: (rows, stats dict)."""
        L = lib()
        keep, qs = [], (GenomeQuery * max(len(genomes), 1))()
        for i, (gid, contigs) in enumerate(genomes):
            arr = (Contig * max(len(contigs), 1))()
            for j, (cid, seq) in enumerate(contigs):
                b = bytes(seq)
                cb = cid if isinstance(cid, bytes) else str(cid).encode()
                keep += [b, cb]
                arr[j].id, arr[j].seq, arr[j].len = cb, b, len(b)
            gb = gid if isinstance(gid, bytes) else str(gid).encode()
            keep += [arr, gb]
            qs[i].id, qs[i].contigs, qs[i].ncontigs = gb, arr, len(contigs)
        opt = ScreenOpt(min_prefix, windows, top_n, 1 if details else 0)
        sc = C.c_void_p()
        st = L.lm_index_screen_genomes(self.h, qs, len(genomes), C.byref(opt), C.byref(sc))
        self._err(st, REFUSED_ARG_OR_OPTION)
        try:
            rows_p, keys_p, pref_p = C.POINTER(ScreenRow)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
            n = L.lm_screen_rows(sc, C.byref(rows_p))
            L.lm_screen_keys(sc, C.byref(keys_p))
            L.lm_screen_prefixes(sc, C.byref(pref_p))
            out = [[] for _ in genomes]
            for i in range(n):
                r = rows_p[i]
                d = {f[0]: getattr(r, f[0]) for f in ScreenRow._fields_ if f[0] not in ("pad", "keys_off", "prefixes_off", "nkeys")}
                d["keys"] = [keys_p[r.keys_off + j] for j in range(r.nkeys)]
                d["prefixes"] = list(C.string_at(C.addressof(pref_p.contents) + r.prefixes_off, r.hit_masks)) if r.hit_masks else []
                out[r.query].append(d)
            if not want_stats:
                return out
            stt = ScreenStats()
            L.lm_screen_get_stats(sc, C.byref(stt))
            return out, {f[0]: getattr(stt, f[0]) for f in ScreenStats._fields_}
        finally:
            L.lm_screen_free(sc)

    def pairs(self, keys=None, min_prefix=21, masks=1024, min_mask_fraction=0.25, want_stats=False, arrays=False):
        """lm_index_genome_pairs: the similar record pairs of this index - what `lexicmap genome pair -s 0` prints -
        computed on the GPU from the resident seed image.  keys: record keys (batch << 17 | index) to look among, None:
        every record; the whitelist of set_genome_filter is not consulted.  masks: 0 = all masks, else a power of 4 >= 64
        (the first mask of every prefix of log4(masks) bases).  -> the rows in output order (n_masks descending, sum_prefix
        descending, (key1, key2) ascending) as a list of dicts key1, key2, genome1, genome2, n_masks, sum_prefix; with
        arrays=True as ONE numpy structured array (key1, key2, n_masks, sum_prefix) without the names, for results of
        millions of rows.  want_stats: (rows, stats dict); stats["total_masks"] is what format_pair_rows takes.
        ValueError for what the library refuses as an argument or option (an unknown or repeated key, a sharded handle,
        min_prefix outside [mask_prefix + anchor_prefix, k], masks, a negative min_mask_fraction)."""
        arr, n = self._record_keys(keys)
        opt = PairOpt(min_prefix, masks, min_mask_fraction)
        pr = C.c_void_p()
        st = lib().lm_index_genome_pairs(self.h, arr, n, C.byref(opt), C.byref(pr))
        return self._pairs_result(st, pr, want_stats, arrays)

    def pair_seeds(self, keys=None, masks=1024):
        """lm_index_pair_seeds: the forward seeds of the taken masks of this handle's (selected) records as bytes, for the
        ranks that pair their records with these (pairs_across).  Works on shards and on unsharded handles; the blob of a
        handle or selection without records is valid and empty.  masks must be what pairs_across is called with."""
        L = lib()
        arr, n = self._record_keys(keys)
        opt = PairOpt(21, masks, 0.25)
        p, nb = C.c_void_p(), C.c_size_t()
        st = L.lm_index_pair_seeds(self.h, arr, n, C.byref(opt), C.byref(p), C.byref(nb))
        self._err(st, REFUSED_ARG_OR_OPTION)
        try:
            return C.string_at(p, nb.value)
        finally:
            L.lm_free(p)

    def pairs_across(self, blobs, keys=None, min_prefix=21, masks=1024, min_mask_fraction=0.25, want_stats=False, arrays=False):
        """lm_index_genome_pairs_across: the pairs among this handle's own (selected) records and between an own record and
        a record of any of `blobs` (pair_seeds() of other shards, exported with the same masks) - never between two blob
        records.  Rank r of a sharded index passes the blobs of the ranks s < r; merge_pair_rows of all ranks' rows is then
        the unsharded index's Index.pairs, row for row.  blobs=[]: the pairs within this handle, also on a shard.  Options,
        result and ValueError as Index.pairs; ValueError also for a blob that is broken, of other masks or another `masks`,
        or whose records overlap the handle's or another blob's."""
        L = lib()
        arr, n = self._record_keys(keys)
        opt = PairOpt(min_prefix, masks, min_mask_fraction)
        bl = [bytes(b) for b in blobs]
        ptrs = (C.c_char_p * max(len(bl), 1))(*bl)
        lens = (C.c_size_t * max(len(bl), 1))(*[len(b) for b in bl])
        pr = C.c_void_p()
        st = L.lm_index_genome_pairs_across(self.h, arr, n, C.cast(ptrs, C.POINTER(C.c_void_p)), lens, len(bl), C.byref(opt), C.byref(pr))
        return self._pairs_result(st, pr, want_stats, arrays)

    def _pairs_result(self, st, pr, want_stats, arrays):
        import numpy as np
        L = lib()
        self._err(st, REFUSED_ARG_OR_OPTION)
        try:
            rows_p = C.POINTER(PairRow)()
            nr = L.lm_pairs_rows(pr, C.byref(rows_p))
            if arrays:
                raw = np.dtype([("key1", np.uint64), ("key2", np.uint64), ("genome1", np.uintp), ("genome2", np.uintp),
                                ("n_masks", np.uint32), ("sum_prefix", np.uint32)])   # PairRow, the pointers as numbers
                assert raw.itemsize == C.sizeof(PairRow)
                full = np.frombuffer(C.string_at(rows_p, nr * raw.itemsize), dtype=raw) if nr else np.zeros(0, raw)
                out = np.zeros(nr, dtype=[("key1", np.uint64), ("key2", np.uint64), ("n_masks", np.uint32), ("sum_prefix", np.uint32)])
                for f in out.dtype.names:
                    out[f] = full[f]
            else:
                out = [{f[0]: getattr(rows_p[i], f[0]) for f in PairRow._fields_} for i in range(nr)]
            if not want_stats:
                return out
            stt = PairStats()
            L.lm_pairs_get_stats(pr, C.byref(stt))
            return out, {f[0]: getattr(stt, f[0]) for f in PairStats._fields_}
        finally:
            L.lm_pairs_free(pr)

    def _subseq_result(self, st, sp):
        self._err(st, REFUSED_ARG)
        return Subseqs(sp)

    def subseq(self, regions, upstream=0, downstream=0, ignore_errors=False):
        """lm_index_subseqs: the bases of regions of this index's records with flanks - what `lexicmap utils subseq` prints -
        extracted on the GPU from the resident 2-bit genomes.  regions: dicts with `key` (record key batch << 17 | index) or
        `genome_id`; `seq_id` or `seq_idx` (neither: concatenated coordinates); `begin`, `end` (1-based, inclusive); `rc`.
        -> Subseqs.  ValueError for what the library refuses as an argument: begin < 1, end < begin, a negative flank, and -
        unless ignore_errors - the first region that cannot be answered."""
        L = lib()
        arr = (Region * max(len(regions), 1))()
        keep = []
        for i, d in enumerate(regions):
            gid, sid = ((x if isinstance(x, bytes) or x is None else str(x).encode()) for x in (d.get("genome_id"), d.get("seq_id")))
            keep += [gid, sid]
            key = d.get("key")
            arr[i] = Region(REGION_BY_NAME if key is None else int(key), gid, sid, int(d.get("seq_idx", -1)),
                            1 if d.get("rc") else 0, int(d["begin"]), int(d["end"]))
        opt = SubseqOpt(upstream, downstream, 1 if ignore_errors else 0, 0)
        sp = C.c_void_p()
        return self._subseq_result(L.lm_index_subseqs(self.h, arr, len(regions), C.byref(opt), C.byref(sp)), sp)

    def subseq_rows(self, rows, upstream=0, downstream=0, ignore_errors=False):
        """lm_index_subseq_rows: the subject region of every search row (a numpy row array of merge.ROW_DTYPE, or the list
        of dicts Index.search returns) with flanks -> Subseqs, one entry per row"""
        import numpy as np
        from .merge import ROW_DTYPE, pack_rows
        arr = pack_rows(rows) if isinstance(rows, list) else np.ascontiguousarray(rows, dtype=ROW_DTYPE)
        opt = SubseqOpt(upstream, downstream, 1 if ignore_errors else 0, 0)
        sp = C.c_void_p()
        st = lib().lm_index_subseq_rows(self.h, arr.ctypes.data_as(C.POINTER(Hsp)), len(arr), C.byref(opt), C.byref(sp))
        return self._subseq_result(st, sp)

    def genome_seqs(self, genome_id):
        """lm_index_genome_seqs: every contig of every record of a genome, whole and forward, in record and contig order
        (`lexicmap utils genome-seqs`) -> Subseqs; ValueError for an unknown genome id"""
        sp = C.c_void_p()
        gid = genome_id if isinstance(genome_id, bytes) else str(genome_id).encode()
        return self._subseq_result(lib().lm_index_genome_seqs(self.h, gid, C.byref(sp)), sp)

    def screen_structure(self):
        """lm_index_screen_structure: what screening reads of this handle's lists beyond its own seeds (occupied partitions,
        outlier k-mers) as bytes, for the other shards of the index"""
        L = lib()
        p, n = C.c_void_p(), C.c_size_t()
        st = L.lm_index_screen_structure(self.h, C.byref(p), C.byref(n))
        self._err(st)
        try:
            return C.string_at(p, n.value)
        finally:
            L.lm_free(p)

    def add_screen_structure(self, blob):
        """lm_index_screen_add_structure: another shard's screen_structure(); once every shard has every other shard's,
        screen() on a shard gives the unsharded index's rows for its records.  None: back to the handle's own lists."""
        st = lib().lm_index_screen_add_structure(self.h, blob, len(blob) if blob else 0)
        self._err(st, REFUSED_ARG)

    def upload(self, seqs):
        arr, keep = _queries(seqs)
        qb = C.c_void_p()
        st = lib().lm_qbatch_upload(self.h, arr, len(seqs), C.byref(qb))
        self._err(st)
        return qb

    def free_batch(self, qb):
        lib().lm_qbatch_free(qb)

    def search_resident(self, qb, want_rows=True):
        L = lib()
        res = C.c_void_p()
        st = L.lm_search_resident(self.h, qb, C.byref(res))
        self._err(st)
        out = self._collect(res, want_rows)
        L.lm_result_free(res)
        return out

    def search_resident_np(self, qb):
        """rows as a numpy structured array VIEW of the library's lm_hsp rows (no copy; the lm_result is released when
        the array is garbage collected) + stats. The six `char *` columns are process-local addresses (valid while the
        array / the index are alive); lexicmap_amd.merge zeroes them before rows leave the process."""
        L = lib()
        res = C.c_void_p()
        st = L.lm_search_resident(self.h, qb, C.byref(res))
        self._err(st)
        return self._view(res)

    def search_resident_keep_np(self, qb, keep_query, keep_bg):
        """search_resident_keep with the rows as search_resident_np gives them: a numpy VIEW whose pointer columns are live
        while the array is alive (what a sharded -n search hands to Comm.gather_merge_rows(strings=True))"""
        import numpy as np
        L = lib()
        kq = np.ascontiguousarray(keep_query, dtype=np.uint32)
        kg = np.ascontiguousarray(keep_bg, dtype=np.uint64)
        res = C.c_void_p()
        st = L.lm_search_resident_keep(self.h, qb, kq.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       kg.ctypes.data_as(C.POINTER(C.c_uint64)), len(kq), C.byref(res))
        self._err(st)
        return self._view(res)

    def _view(self, res):
        import weakref
        import numpy as np
        from .merge import ROW_DTYPE
        L = lib()
        rows_p = C.POINTER(Hsp)()
        n = L.lm_result_rows(res, C.byref(rows_p))
        stats = StageStats()
        L.lm_result_stats(res, C.byref(stats))
        if n:
            buf = (C.c_char * (n * C.sizeof(Hsp))).from_address(C.addressof(rows_p.contents))
            arr = np.frombuffer(buf, dtype=ROW_DTYPE)
            weakref.finalize(buf, L.lm_result_free, res)  # arr -> buf keeps the rows alive
        else:
            arr = np.zeros(0, dtype=ROW_DTYPE)
            L.lm_result_free(res)
        return arr, {f[0]: getattr(stats, f[0]) for f in StageStats._fields_}

    def set_genome_filter(self, keys):
        """genome whitelist (batch<<17|index keys) for the searches that follow; empty / None clears it"""
        keys = list(keys or [])
        arr = (C.c_uint64 * max(len(keys), 1))(*keys)
        st = lib().lm_index_set_genome_filter(self.h, arr, len(keys))
        self._err(st)

    def search_scores(self, qb):
        """(query, batch_genome, score) numpy arrays: this shard's candidates for the -n cut"""
        import numpy as np
        L = lib()
        sg, n = C.c_void_p(), C.c_size_t()
        q, g, s = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_float)()
        st = L.lm_search_scores(self.h, qb, C.byref(sg), C.byref(n), C.byref(q), C.byref(g), C.byref(s))
        self._err(st)
        k = n.value
        out = (np.ctypeslib.as_array(q, shape=(k,)).copy() if k else np.zeros(0, np.uint32),
               np.ctypeslib.as_array(g, shape=(k,)).copy() if k else np.zeros(0, np.uint64),
               np.ctypeslib.as_array(s, shape=(k,)).copy() if k else np.zeros(0, np.float32))
        L.lm_stage_free(sg)
        return out

    def search_resident_keep(self, qb, keep_query, keep_bg):
        import numpy as np
        L = lib()
        kq = np.ascontiguousarray(keep_query, dtype=np.uint32)
        kg = np.ascontiguousarray(keep_bg, dtype=np.uint64)
        res = C.c_void_p()
        st = L.lm_search_resident_keep(self.h, qb, kq.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       kg.ctypes.data_as(C.POINTER(C.c_uint64)), len(kq), C.byref(res))
        self._err(st)
        out = self._collect(res)
        L.lm_result_free(res)
        return out

    def _collect(self, res, want_rows=True):
        L = lib()
        rows_p = C.POINTER(Hsp)()
        n = L.lm_result_rows(res, C.byref(rows_p))
        stats = StageStats()
        L.lm_result_stats(res, C.byref(stats))
        rows = []
        if want_rows:
            for i in range(n):
                r = rows_p[i]
                rows.append({f[0]: getattr(r, f[0]) for f in Hsp._fields_})
        return rows, {f[0]: getattr(stats, f[0]) for f in StageStats._fields_}

    def search(self, seqs):
        """rows (list of dict) for a batch of query sequences + stage statistics"""
        L = lib()
        arr, keep = _queries(seqs)
        res = C.c_void_p()
        st = L.lm_search_batch(self.h, arr, len(seqs), C.byref(res))
        self._err(st)
        out = self._collect(res)
        L.lm_result_free(res)
        return out

    def search_tsv(self, ids, seqs, more_columns=False):
        L = lib()
        arr, keep = _queries(seqs)
        res = C.c_void_p()
        st = L.lm_search_batch(self.h, arr, len(seqs), C.byref(res))
        self._err(st)
        rows_p = C.POINTER(Hsp)()
        n = L.lm_result_rows(res, C.byref(rows_p))
        size = 1 << 22 if more_columns else 1 << 16
        buf = C.create_string_buffer(size)
        lines = []
        for i in range(n):
            q = rows_p[i].query
            L.lm_format_row(C.byref(rows_p[i]), ids[q].encode(), len(seqs[q]), int(more_columns), buf, size)
            lines.append(buf.value.decode())
        L.lm_result_free(res)
        return lines

    # ---- stage-level entry points (parity tests) ----
    def mask(self, seqs):
        L = lib()
        arr, keep = _queries(seqs)
        sg, km, lo, lc = C.c_void_p(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
        st = L.lm_mask_batch(self.h, arr, len(seqs), C.byref(sg), C.byref(km), C.byref(lo), C.byref(lc))
        self._err(st)
        M = self.info()["masks"]
        n = len(seqs) * M
        kmers = [km[i] for i in range(n)]
        off = [lo[i] for i in range(n + 1)]
        locs = [lc[i] for i in range(off[n])]
        L.lm_stage_free(sg)
        return kmers, off, locs

    def seed_chain(self, seqs):
        L = lib()
        arr, keep = _queries(seqs)
        sg, npairs = C.c_void_p(), C.c_size_t()
        pairs, raw, clr = C.POINTER(Pair)(), C.POINTER(Anchor)(), C.POINTER(Anchor)()
        cptr, cidx = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
        st = L.lm_seed_chain_batch(self.h, arr, len(seqs), C.byref(sg), C.byref(npairs), C.byref(pairs), C.byref(raw),
                                   C.byref(clr), C.byref(cptr), C.byref(cidx))
        self._err(st)
        out = []
        tup = lambda a: (a.qbegin, a.tbegin, a.len, a.qrc, a.trc)
        for i in range(npairs.value):
            p = pairs[i]
            chains = []
            for c in range(p.chain_n):
                chains.append([cidx[j] for j in range(cptr[p.chain_off + c], cptr[p.chain_off + c + 1])])
            out.append(dict(query=p.query, genome=p.batch_genome,
                            raw=[tup(raw[p.raw_off + j]) for j in range(p.raw_n)],
                            cleared=[tup(clr[p.clr_off + j]) for j in range(p.clr_n)],
                            score=p.score, chains=chains))
        L.lm_stage_free(sg)
        return out

    def pseudoalign(self, queries, problems):
        """problems: list of (query index, qbegin, qend, target bytes)"""
        L = lib()
        qarr, k1 = _queries(queries)
        tarr, k2 = _queries([p[3] for p in problems])
        n = len(problems)
        qi = (C.c_uint32 * max(n, 1))(*[p[0] for p in problems])
        qb = (C.c_uint32 * max(n, 1))(*[p[1] for p in problems])
        qe = (C.c_uint32 * max(n, 1))(*[p[2] for p in problems])
        sg, ro, rv = C.c_void_p(), C.POINTER(C.c_int64)(), C.POINTER(Chain2)()
        st = L.lm_pseudoalign_batch(self.h, qarr, len(queries), tarr, qi, qb, qe, n, C.byref(sg), C.byref(ro),
                                    C.byref(rv))
        self._err(st)
        out = []
        for i in range(n):
            out.append([{f[0]: getattr(rv[j], f[0]) for f in Chain2._fields_} for j in range(ro[i], ro[i + 1])])
        L.lm_stage_free(sg)
        return out

    @staticmethod
    def _chains_and_anchors(n, ro, rv, ao, av):
        import numpy as np
        chains = [[{f[0]: getattr(rv[j], f[0]) for f in Chain2._fields_} for j in range(ro[i], ro[i + 1])] for i in range(n)]
        off = [ao[i] for i in range(n + 1)]
        rec = np.dtype([("qbegin", "<i4"), ("tbegin", "<i4"), ("len", "u1"), ("trc", "u1"), ("qrc", "u1"), ("pad", "u1")])
        a = np.ctypeslib.as_array(C.cast(av, C.POINTER(C.c_uint8)), shape=(off[n] * C.sizeof(Anchor),)).view(rec) if off[n] else \
            np.zeros(0, rec)
        cols = list(zip(a["qbegin"].tolist(), a["tbegin"].tolist(), a["len"].tolist(), a["trc"].tolist(), a["qrc"].tolist()))
        return chains, [cols[off[i]:off[i + 1]] for i in range(n)]

    def pseudoalign_anchors(self, queries, problems):
        """pseudoalign (ASCII windows of the caller), and per problem the emitted anchors (qbegin, tbegin, len, trc, qrc) in the
        order of the sorted device list (lm_pseudoalign_batch_ex): (chains, anchors)"""
        L = lib()
        qarr, k1 = _queries(queries)
        tarr, k2 = _queries([p[3] for p in problems])
        n = len(problems)
        qi = (C.c_uint32 * max(n, 1))(*[p[0] for p in problems])
        qb = (C.c_uint32 * max(n, 1))(*[p[1] for p in problems])
        qe = (C.c_uint32 * max(n, 1))(*[p[2] for p in problems])
        sg, ro, rv = C.c_void_p(), C.POINTER(C.c_int64)(), C.POINTER(Chain2)()
        ao, av = C.POINTER(C.c_int64)(), C.POINTER(Anchor)()
        st = L.lm_pseudoalign_batch_ex(self.h, qarr, len(queries), tarr, qi, qb, qe, n, C.byref(sg), C.byref(ro), C.byref(rv),
                                       C.byref(ao), C.byref(av))
        self._err(st)
        out = self._chains_and_anchors(n, ro, rv, ao, av)
        L.lm_stage_free(sg)
        return out

    def pseudoalign_regions(self, queries, regions):
        """pseudo-alignment of windows of the resident genomes, through the kernels a search runs (lm_pseudoalign_regions).
        regions: list of (query index, qbegin, qend, local genome, tbegin, wlen, rc) with tbegin in concatenated-genome
        coordinates (as fetch).  Returns (chains, anchors) as pseudoalign_anchors.  A region the library refuses (LM_ERR_ARG)
        raises ValueError with its text."""
        L = lib()
        qarr, k1 = _queries(queries)
        n = len(regions)
        arr = (PaRegion * max(n, 1))()
        for i, (q, qb, qe, g, tb, wl, rc) in enumerate(regions):
            arr[i] = PaRegion(q, qb, qe, int(rc), g, tb, wl)
        sg, ro, rv = C.c_void_p(), C.POINTER(C.c_int64)(), C.POINTER(Chain2)()
        ao, av = C.POINTER(C.c_int64)(), C.POINTER(Anchor)()
        st = L.lm_pseudoalign_regions(self.h, qarr, len(queries), arr, n, C.byref(sg), C.byref(ro), C.byref(rv), C.byref(ao),
                                      C.byref(av))
        self._err(st, REFUSED_ARG)
        out = self._chains_and_anchors(n, ro, rv, ao, av)
        L.lm_stage_free(sg)
        return out

    def wfa(self, pairs):
        L = lib()
        qarr, k1 = _queries([p[0] for p in pairs])
        tarr, k2 = _queries([p[1] for p in pairs])
        sg, rv, ops = C.c_void_p(), C.POINTER(Wfa)(), C.POINTER(C.c_uint64)()
        st = L.lm_wfa_batch(self.h, qarr, tarr, len(pairs), C.byref(sg), C.byref(rv), C.byref(ops))
        self._err(st)
        out = []
        for i in range(len(pairs)):
            r = rv[i]
            out.append(dict(status=r.status, score=r.score, ops=[ops[r.ops_off + j] for j in range(r.nops)],
                            qbegin=r.qbegin, qend=r.qend, tbegin=r.tbegin, tend=r.tend, align_len=r.align_len,
                            matches=r.matches, gaps=r.gaps, gap_regions=r.gap_regions))
        L.lm_stage_free(sg)
        return out

    def profile(self, on=True):
        lib().lm_profile_enable(self.h, int(on))

    def profile_reset(self):
        lib().lm_profile_reset(self.h)

    def profile_exclusive(self, on=True):
        """kernels of the following searches one after the other: exclusive per-kernel times (measurement only)"""
        lib().lm_profile_exclusive(self.h, int(on))

    def profile_mark(self, ident):
        """an empty marker kernel between idle points of the device: where a rocprofv3 pass is cut (measurement only)"""
        lib().lm_profile_mark(self.h, int(ident))

    def tuning_reload(self):
        """re-read the LM_* experiment switches from the environment (measurement only: results do not depend on them)"""
        lib().lm_tuning_reload(self.h)

    def profile_get(self):
        p = C.POINTER(KernelTime)()
        n = lib().lm_profile_get(self.h, C.byref(p))
        return [dict(name=p[i].name.decode(), launches=p[i].launches, total_ms=p[i].total_ms, bytes=p[i].bytes)
                for i in range(n)]


class IndexBuilder:
    """lm_index_builder: genomes are added one at a time (the host may stream them), finish() returns the Index"""

    def __init__(self, build_opt=None, options=None, device=0, residency=None, masks=None):
        """masks: None makes the plain lm_index_builder_new call (a mask set generated from build_opt.mask_seed; k = 31 only).
        A sequence or numpy array of uint64 builds with exactly those masks (lm_index_builder_new_masks: build_opt.k is their
        k, build_opt.masks is ignored) - e.g. Index.masks() of another index or read_mask_file(); a set the library refuses
        (LM_ERR_ARG) raises ValueError with its text."""
        L = lib()
        self.opt = options or default_options()
        self.bo = build_opt or BuildOpt.default()
        self.device = device
        h = C.c_void_p()
        res = C.byref(residency) if residency is not None else None
        if masks is None:
            st = L.lm_index_builder_new(C.byref(self.bo), C.byref(self.opt), res, device, C.byref(h))
            _check(st, _global_error, "lm_index_builder_new failed (%(status)d): %(text)s")
        else:
            import numpy as np
            ms = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1)  # (the library copies them before it returns)
            st = L.lm_index_builder_new_masks(C.byref(self.bo), ms.ctypes.data_as(C.POINTER(C.c_uint64)), ms.size, C.byref(self.opt),
                                              res, device, C.byref(h))
            _check(st, _global_error, "lm_index_builder_new_masks failed (%(status)d): %(text)s", REFUSED_ARG)
        self.h = h

    @classmethod
    def extending(cls, index, build_opt=None, residency=None):
        """lm_index_builder_extend: a builder that continues `index`, which must stay open until finish() or close()"""
        L = lib()
        self = cls.__new__(cls)
        self.opt = index.opt
        self.bo = build_opt
        self.device = 0
        self.base = index  # (kept alive for as long as the builder reads it)
        h = C.c_void_p()
        st = L.lm_index_builder_extend(index.h, C.byref(build_opt) if build_opt is not None else None,
                                       C.byref(residency) if residency is not None else None, C.byref(h))
        _check(st, _global_error, "lm_index_builder_extend failed (%(status)d): %(text)s")
        self.h = h
        return self

    @classmethod
    def like(cls, index, build_opt=None, residency=None):
        """lm_index_builder_like: an empty builder with the masks, options, device and build settings of `index`"""
        L = lib()
        self = cls.__new__(cls)
        self.opt = index.opt
        self.bo = build_opt
        self.device = 0
        h = C.c_void_p()
        st = L.lm_index_builder_like(index.h, C.byref(build_opt) if build_opt is not None else None,
                                     C.byref(residency) if residency is not None else None, C.byref(h))
        _check(st, _global_error, "lm_index_builder_like failed (%(status)d): %(text)s")
        self.h = h
        return self

    def last_error(self):
        return lib().lm_index_builder_last_error(self.h).decode()

    def try_add_index(self, index, keep=None):
        """lm_index_builder_add_index: the status (0 = appended; 7 = LM_ERR_ARG: refused, see last_error(), the builder stays
        usable).  keep: record keys (batch << 17 | index) of `index`, None for all of its records."""
        if keep is None:
            arr, n = None, 0
        else:
            keys = [int(k) for k in keep]
            n = len(keys)
            arr = (C.c_uint64 * max(n, 1))(*keys)
        st = lib().lm_index_builder_add_index(self.h, index.h, arr, n)
        if st == 0:
            if not hasattr(self, "sources"):
                self.sources = []
            self.sources.append(index)  # (kept alive for as long as the builder reads it)
        return st

    def add_index(self, index, keep=None):
        st = self.try_add_index(index, keep)
        _check(st, self.last_error, "lm_index_builder_add_index failed (%(status)d): %(text)s", REFUSED_ARG)
        return self

    def try_add(self, genome_id, contigs):
        """lm_index_builder_add: the status (0 = added; 7 = LM_ERR_ARG: refused, see last_error(), the builder stays usable)"""
        n = len(contigs)
        arr = (Contig * max(n, 1))()
        keep = []
        for i, (cid, seq) in enumerate(contigs):
            s = bytes(seq)
            keep.append(s)
            arr[i].id = cid.encode() if isinstance(cid, str) else cid
            arr[i].seq = s
            arr[i].len = len(s)
        gid = genome_id.encode() if isinstance(genome_id, str) else genome_id
        return lib().lm_index_builder_add(self.h, gid, arr, n)

    def add(self, genome_id, contigs):
        st = self.try_add(genome_id, contigs)
        _check(st, self.last_error, "lm_index_builder_add failed (%(status)d): %(text)s", REFUSED_ARG)

    def finish(self):
        """lm_index_builder_finish: the builder is consumed whether it succeeds or not"""
        L = lib()
        h = C.c_void_p()
        bh, self.h = self.h, None
        st = L.lm_index_builder_finish(bh, C.byref(h))
        _check(st, _global_error, "lm_index_builder_finish failed (%(status)d): %(text)s")
        return Index(None, self.opt, self.device, _handle=h)

    def close(self):
        if self.h:
            lib().lm_index_builder_free(self.h)
            self.h = None


def write_mask_file(path, k, masks):
    """a mask set in the text form `lexicmap utils masks` prints and `lexicmap index -M/--mask-file` reads: one mask per
    line, `<1-based number>\\t<k-mer>`, A = 0, C = 1, G = 2, T = 3 with the first base in the highest bits; gzip-compressed
    when path ends in .gz.  Host-side file work, like FASTA reading."""
    import gzip
    k = int(k)
    if not 1 <= k <= 32:
        raise ValueError("write_mask_file: k = %d is outside [1, 32]" % k)
    lines = []
    for i, m in enumerate(masks):
        m = int(m)
        if m < 0 or m >> (2 * k):
            raise ValueError("write_mask_file: mask %d is not below 4^k (k = %d)" % (i, k))
        lines.append("%d\t%s\n" % (i + 1, "".join("ACGT"[(m >> (2 * (k - 1 - j))) & 3] for j in range(k))))
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "wb") as f:
        f.write("".join(lines).encode())


def read_mask_file(path):
    """-> (k, numpy uint64 array): the masks of a file in the form of write_mask_file, in file order.  ValueError for lines of
    different k-mer lengths, a letter outside ACGT (either case), numbers that are not 1..n in order, or no mask at all."""
    import gzip
    import numpy as np
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rb") as f:
        text = f.read().decode("ascii", "replace")
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    k, out = None, []
    for ln, line in enumerate(text.splitlines(), 1):
        if not line.strip():
            continue
        cols = line.rstrip("\r").split("\t")
        if len(cols) < 2 or not cols[0].strip().isdigit() or int(cols[0]) != len(out) + 1:
            raise ValueError("%s line %d: expected mask number %d and a k-mer separated by a tab" % (path, ln, len(out) + 1))
        kmer = cols[1].strip().upper()
        if k is None:
            k = len(kmer)
            if not 1 <= k <= 32:
                raise ValueError("%s line %d: a k-mer of %d bases (1..32 fit a mask)" % (path, ln, k))
        elif len(kmer) != k:
            raise ValueError("%s line %d: a k-mer of %d bases after k-mers of %d" % (path, ln, len(kmer), k))
        v = 0
        for c in kmer:
            if c not in code:
                raise ValueError("%s line %d: letter %r is not one of ACGT" % (path, ln, c))
            v = (v << 2) | code[c]
        out.append(v)
    if not out:
        raise ValueError("%s holds no mask" % path)
    return k, np.array(out, dtype=np.uint64)


def format_rows(rows, ids, lens, flags=0, want_text=True):
    """lm_format_rows: the TSV text (bytes) of a numpy row array (merge.ROW_DTYPE, pointer columns live in this process); ids /
    lens: id and length of every batch query.  want_text=False: only (bytes, seconds) - the text is released unseen."""
    import time
    import numpy as np
    from .merge import ROW_DTYPE
    L = lib()
    arr = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
    idarr = (C.c_char_p * len(ids))(*[i if isinstance(i, bytes) else str(i).encode() for i in ids])
    lnarr = (C.c_uint32 * len(lens))(*[int(x) for x in lens])
    text, n = C.c_void_p(), C.c_size_t(0)
    t0 = time.time()
    st = L.lm_format_rows(arr.ctypes.data_as(C.POINTER(Hsp)), len(arr), idarr, lnarr, len(ids), flags, C.byref(text), C.byref(n))
    dt = time.time() - t0
    _check(st, "", "lm_format_rows failed (%(status)d)")
    out = C.string_at(text, n.value) if want_text else None
    L.lm_free(text)
    return (out if want_text else n.value), dt


def format_screen_rows(rows, query_ids, min_prefix, masks, extra=False, header=False):
    """the lines `lexicmap genome search -S` prints for the rows Index.screen returned (one list per query; query_ids their
    ids), each formatted by lm_format_screen_row; header: lm_screen_header first.  masks: the index's mask count."""
    L = lib()
    out = [L.lm_screen_header(1 if extra else 0).decode()] if header else []
    buf = C.create_string_buffer(1 << 20)
    for qid, qrows in zip(query_ids, rows):
        qb = qid if isinstance(qid, bytes) else str(qid).encode()
        for d in qrows:
            gid = d["genome_id"]
            pref = (C.c_uint8 * max(len(d["prefixes"]), 1))(*d["prefixes"])
            r = ScreenRow(0, len(d["keys"]), d["score"], d["batch_genome"], gid, 0, d["score2"], d["hit_masks"], 0, d["hit_kmers"], 0)
            n = L.lm_format_screen_row(C.byref(r), pref, qb, min_prefix, masks, 1 if extra else 0, buf, len(buf))
            if n >= len(buf):
                buf = C.create_string_buffer(n + 1)
                L.lm_format_screen_row(C.byref(r), pref, qb, min_prefix, masks, 1 if extra else 0, buf, len(buf))
            out.append(buf.value.decode())
    return out


def format_pair_rows(rows, min_prefix, total_masks, header=False):
    """the lines `lexicmap genome pair` prints for the rows Index.pairs returned (the list of dicts), each formatted by
    lm_format_pair_row; header: lm_pair_header first.  total_masks: stats["total_masks"] of the call."""
    L = lib()
    out = [L.lm_pair_header().decode()] if header else []
    buf = C.create_string_buffer(1 << 12)
    for d in rows:
        g1, g2 = (x if isinstance(x, bytes) or x is None else str(x).encode() for x in (d["genome1"], d["genome2"]))
        r = PairRow(d["key1"], d["key2"], g1, g2, d["n_masks"], d["sum_prefix"])
        n = L.lm_format_pair_row(C.byref(r), min_prefix, total_masks, buf, len(buf))
        if n >= len(buf):
            buf = C.create_string_buffer(n + 1)
            L.lm_format_pair_row(C.byref(r), min_prefix, total_masks, buf, len(buf))
        out.append(buf.value.decode())
    return out


def merge_pair_rows(parts):
    """lm_pairs_merge: the rows of several Index.pairs_across calls (lists of dicts, one list per rank) as ONE list in the
    rule's order - what rank 0 does with the ranks' rows; each list goes through lm_pairs_from_rows, as rows that came over
    the wire do.  ValueError when a pair occurs twice (the ranks did not follow the s < r scheme) or a list is out of order."""
    L = lib()
    handles, keep = [], []
    merged = C.c_void_p()
    try:
        for rows in parts:
            arr = (PairRow * max(len(rows), 1))()
            for i, d in enumerate(rows):
                g1, g2 = (x if isinstance(x, bytes) or x is None else str(x).encode() for x in (d["genome1"], d["genome2"]))
                keep += [g1, g2]
                arr[i] = PairRow(d["key1"], d["key2"], g1, g2, d["n_masks"], d["sum_prefix"])
            h = C.c_void_p()
            st = L.lm_pairs_from_rows(arr, len(rows), None, C.byref(h))
            _check(st, "", "lm_pairs_from_rows: status %(status)d")
            handles.append(h)
        hs = (C.c_void_p * max(len(handles), 1))(*[h.value for h in handles])
        st = L.lm_pairs_merge(hs, len(handles), C.byref(merged))
        _check(st, _global_error, "lm_pairs_merge: status %(status)d", REFUSED_ARG)
        rows_p = C.POINTER(PairRow)()
        nr = L.lm_pairs_rows(merged, C.byref(rows_p))
        return [{f[0]: getattr(rows_p[i], f[0]) for f in PairRow._fields_} for i in range(nr)]
    finally:
        for h in handles:
            L.lm_pairs_free(h)
        if merged:
            L.lm_pairs_free(merged)


class Subseqs:
    """lm_subseqs: the answer of Index.subseq / subseq_rows / genome_seqs.  info: one dict per region (key, seq_idx, status,
    rc, begin, end, off, len, genome_id, seq_id); seqs: the bases of every region as bytes (b"" where status != 0); stats.
    The library's result is released by close() or with the object."""

    def __init__(self, handle):
        L = lib()
        self.h = handle
        info_p, bases = C.POINTER(SubseqInfo)(), C.c_void_p()
        self.n = L.lm_subseqs_get(self.h, C.byref(info_p), C.byref(bases))
        self.info = [{f[0]: getattr(info_p[i], f[0]) for f in SubseqInfo._fields_ if f[0] != "pad"} for i in range(self.n)]
        stt = SubseqStats()
        L.lm_subseqs_get_stats(self.h, C.byref(stt))
        self.stats = {f[0]: getattr(stt, f[0]) for f in SubseqStats._fields_}
        self.blob = C.string_at(bases, self.stats["blob_bytes"]) if self.stats["blob_bytes"] else b""

    @property
    def seqs(self):
        return [self.blob[d["off"]:d["off"] + d["len"]] for d in self.info]

    def close(self):
        if self.h:
            lib().lm_subseqs_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_subseqs(sub, rows=None, ids=None, lens=None, line_width=60):
    """lm_format_subseqs: the FASTA text (bytes) `lexicmap utils subseq` / `genome-seqs` print for a Subseqs.  rows (with ids /
    lens, the id and length of every batch query): the rows Index.subseq_rows was given - the long header of
    `utils subseq -f`.  line_width <= 0: no wrapping."""
    import numpy as np
    from .merge import ROW_DTYPE, pack_rows
    L = lib()
    rp, idarr, lnarr, nq = None, None, None, 0
    if rows is not None:
        # (pack_rows drops the names of a list of dicts: the formatter takes them from the result)
        arr = pack_rows(rows) if isinstance(rows, list) else np.ascontiguousarray(rows, dtype=ROW_DTYPE)
        if len(arr) != sub.n:
            raise ValueError("format_subseqs: %d rows for %d regions" % (len(arr), sub.n))
        rp = arr.ctypes.data_as(C.POINTER(Hsp))
        idarr = (C.c_char_p * max(len(ids), 1))(*[i if isinstance(i, bytes) else str(i).encode() for i in ids])
        lnarr = (C.c_uint32 * max(len(lens), 1))(*[int(x) for x in lens])
        nq = len(ids)
    text, n = C.c_void_p(), C.c_size_t(0)
    st = L.lm_format_subseqs(sub.h, rp, idarr, lnarr, nq, line_width, C.byref(text), C.byref(n))
    _check(st, "", "lm_format_subseqs failed (%(status)d)")
    out = C.string_at(text, n.value)
    L.lm_free(text)
    return out


def row_names(rows, i):
    """(genome_id, seq_id) of row i of a numpy row array (merge.ROW_DTYPE) whose pointer columns are live in THIS process"""
    out = []
    for f in ("genome_id", "seq_id"):
        a = int(rows[f][i])
        out.append(C.string_at(a).decode() if a else None)
    return tuple(out)


def row_strings(rows, i):
    """(cigar, qseq, sseq, align) of row i of a numpy row array (merge.ROW_DTYPE) whose pointer columns are live in THIS
    process; a NULL column is None"""
    out = []
    for f in ("cigar", "qseq", "sseq", "align"):
        a = int(rows[f][i])
        out.append(C.string_at(a).decode() if a else None)
    return tuple(out)


LM_ROW_ALL = 1  # include/lexicmap_hip.h: -a/--all, the four string columns (also the flag of the gather and merge calls)


COMM_ID_BYTES = 128


class Comm:
    """ctypes view of lm_comm (include/lexicmap_hip.h): the RCCL communicator of the sharded search's row gather.
    Rank 0 calls Comm.unique_id() and hands the 128 bytes to the other ranks by the host's own means (bench.py: a
    torch.distributed broadcast); every rank then opens Comm(id, nranks, rank, device)."""

    @staticmethod
    def _error(h):
        """what _check calls for the text of a failed communicator call (h None: a call without a communicator)"""
        return lambda: (lib().lm_comm_last_error(h) or b"").decode()

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        st = lib().lm_comm_unique_id(buf)
        _check(st, Comm._error(None), "lm_comm_unique_id failed (%(status)d): %(text)s")
        return buf.raw

    def __init__(self, uid, nranks, rank, device=0):
        self.L = lib()
        h = C.c_void_p()
        st = self.L.lm_comm_init(bytes(uid), nranks, rank, device, C.byref(h))
        _check(st, Comm._error(None), "lm_comm_init failed (%(status)d): %(text)s")
        self.h = h
        self.nranks, self.rank = nranks, rank

    def close(self):
        if self.h:
            self.L.lm_comm_free(self.h)
            self.h = None

    def gather_rows(self, arr, root=0, strings=False):
        """arr: numpy rows of merge.ROW_DTYPE (this rank's).  -> (list of per-rank row arrays on `root` - views of the
        communicator's buffer, valid until the next call - or None elsewhere, the per-rank counts).  strings=True (every rank
        alike): the cigar / qseq / sseq / align of arr must be live in this process (e.g. search_resident_np's rows, kept alive
        meanwhile); on `root` the rows' string columns then point into the communicator's buffer (api.row_strings)."""
        import numpy as np
        from .merge import ROW_DTYPE
        arr = np.ascontiguousarray(arr, dtype=ROW_DTYPE)
        allp = C.POINTER(Hsp)()
        cnt = (C.c_size_t * self.nranks)()
        st = self.L.lm_gather_rows_ex(self.h, arr.ctypes.data_as(C.POINTER(Hsp)), len(arr), root, LM_ROW_ALL if strings else 0,
                                      C.byref(allp), cnt)
        _check(st, Comm._error(self.h), "lm_gather_rows failed (%(status)d): %(text)s")
        counts = [int(x) for x in cnt]
        if self.rank != root:
            return None, counts
        total = sum(counts)
        if total == 0:
            return [np.zeros(0, dtype=ROW_DTYPE) for _ in counts], counts
        buf = (C.c_char * (total * C.sizeof(Hsp))).from_address(C.addressof(allp.contents))
        allr = np.frombuffer(buf, dtype=ROW_DTYPE)
        out, o = [], 0
        for n in counts:
            out.append(allr[o:o + n])
            o += n
        return out, counts

    def merge_sharded_device(self, dev_ptr, counts, index=None, strings_ptr=None, string_bytes=0):
        """lm_merge_sharded_device: rows of shard 0, 1, ... back to back in device memory at address dev_ptr (counts[r] rows each)
        -> the merged rows (a view of the communicator's pinned buffer, valid until its next call).  strings_ptr (a device
        address): the rows' string columns in the wire form of lm_merge_sharded_device_ex (include/lexicmap_hip.h) - uint32
        lengths [total][4], then string_bytes of 16-byte blocks - which then follow their rows (api.row_strings)."""
        import numpy as np
        from .merge import ROW_DTYPE
        outp = C.POINTER(Hsp)()
        total = C.c_size_t(0)
        cnt = (C.c_size_t * len(counts))(*[int(x) for x in counts])
        if strings_ptr is None:
            st = self.L.lm_merge_sharded_device(self.h, index.h if index is not None else None, C.c_void_p(int(dev_ptr)), cnt, len(counts),
                                                C.byref(outp), C.byref(total))
        else:
            st = self.L.lm_merge_sharded_device_ex(self.h, index.h if index is not None else None, C.c_void_p(int(dev_ptr)), cnt,
                                                   C.c_void_p(int(strings_ptr)), int(string_bytes), len(counts), LM_ROW_ALL,
                                                   C.byref(outp), C.byref(total))
        _check(st, Comm._error(self.h), "lm_merge_sharded_device failed (%(status)d): %(text)s")
        if total.value == 0:
            return np.zeros(0, dtype=ROW_DTYPE)
        buf = (C.c_char * (total.value * C.sizeof(Hsp))).from_address(C.addressof(outp.contents))
        return np.frombuffer(buf, dtype=ROW_DTYPE)

    def gather_merge_rows(self, arr, root=0, index=None, strings=False):
        """lm_gather_merge_rows: the gather and the merge (on the device) in one call.  -> on `root` the merged rows of all ranks
        in output order (a view of the communicator's pinned buffer, valid until its next call), None elsewhere.  index: the
        root's Index (names are re-attached from it) or None.  strings=True (every rank alike): the string columns of arr
        (live in this process) travel too and the merged rows carry them (api.row_strings, api.format_rows with LM_ROW_ALL)."""
        import numpy as np
        from .merge import ROW_DTYPE
        arr = np.ascontiguousarray(arr, dtype=ROW_DTYPE)
        outp = C.POINTER(Hsp)()
        total = C.c_size_t(0)
        st = self.L.lm_gather_merge_rows_ex(self.h, index.h if index is not None else None, arr.ctypes.data_as(C.POINTER(Hsp)), len(arr),
                                            root, LM_ROW_ALL if strings else 0, C.byref(outp), C.byref(total))
        _check(st, Comm._error(self.h), "lm_gather_merge_rows failed (%(status)d): %(text)s")
        if self.rank != root:
            return None
        if total.value == 0:
            return np.zeros(0, dtype=ROW_DTYPE)
        buf = (C.c_char * (total.value * C.sizeof(Hsp))).from_address(C.addressof(outp.contents))
        return np.frombuffer(buf, dtype=ROW_DTYPE)
