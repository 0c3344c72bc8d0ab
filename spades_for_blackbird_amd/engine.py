"""ctypes binding of libbbk.so (include/bbk.h).  Fails loudly when the HIP library is missing."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

BOTH_STRANDS, CANONICAL, WITH_COUNTS, UNSORTED, REFERENCE_ORDER, WITH_MASKS = 1, 2, 4, 8, 16, 32
ORDER_SORTED, ORDER_REFERENCE_BUCKETS16 = 0, 1
NO_TRIM = -2 ** 31  # BBK_NO_TRIM: the trim_quality of records that are trimmed already
# bbk_path_range of include/bbk.h
PATH_RANGE = np.dtype([("edge", np.uint64), ("read", np.uint32), ("init_start", np.uint32), ("init_end", np.uint32),
                       ("map_start", np.uint32), ("map_end", np.uint32), ("reserved", np.uint32)])

ORIENT_FF, ORIENT_FR, ORIENT_RF, ORIENT_RR = 0, 1, 2, 3  # BBK_ORIENT_*: which mate is reverse-complemented


class ClusterParams(C.Structure):
    """bbk_cluster_params of include/bbk.h"""
    _fields_ = [("insert_size", C.c_uint64), ("read_length", C.c_uint64), ("delta", C.c_uint64),
                ("linkage_distance", C.c_uint64), ("max_distance", C.c_uint64), ("filter_threshold", C.c_double)]


class PairInfoStats(C.Structure):
    """bbk_pairinfo_stats of include/bbk.h"""
    _fields_ = [("total", C.c_uint64), ("mapped", C.c_uint64), ("negative", C.c_uint64), ("edge_pairs", C.c_uint64),
                ("mean", C.c_double), ("deviation", C.c_double), ("median", C.c_double), ("mad", C.c_double),
                ("left_quantile", C.c_double), ("right_quantile", C.c_double), ("percentiles", C.c_uint64 * 19),
                ("ok", C.c_int)]


# every symbol include/bbk.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "bbk_last_error", "bbk_version", "bbk_ctx_create", "bbk_ctx_destroy", "bbk_ctx_set_stream",
    "bbk_ctx_synchronize", "bbk_ctx_trim", "bbk_kmerset_verify_order", "bbk_kmerset_get", "bbk_ctx_profile_enable", "bbk_ctx_profile_reset", "bbk_ctx_profile_get",
    "bbk_reads_from_ascii", "bbk_reads_from_packed", "bbk_host_alloc", "bbk_host_free", "bbk_reads_from_device", "bbk_reads_synth", "bbk_reads_synth_meta", "bbk_reads_from_spades_binary",
    "bbk_reads_write_spades_binary", "bbk_reads_count", "bbk_reads_bases",
    "bbk_reads_get_ascii", "bbk_reads_export_ascii", "bbk_reads_free",
    "bbk_count", "bbk_count_begin", "bbk_count_push_reads", "bbk_count_push_ascii", "bbk_count_finish", "bbk_count_finish_min_count", "bbk_count_abort",
    "bbk_count_pushed_instances", "bbk_extindex_from_device", "bbk_extindex_export_u32", "bbk_extindex_begin", "bbk_extindex_push_reads", "bbk_extindex_finish",
    "bbk_extindex_abort", "bbk_extindex_finish_with_set", "bbk_count_extindex", "bbk_kmerset_from_device", "bbk_kmerset_from_device_ex", "bbk_kmerset_both_strands", "bbk_kmerset_both_strands_ex", "bbk_words", "bbk_kmerset_size", "bbk_kmerset_k", "bbk_kmerset_keys", "bbk_reads_median_filter",
    "bbk_kmerset_instances", "bbk_kmerset_export", "bbk_kmerset_export_by_owner", "bbk_kmerset_free",
    "bbk_kmerset_write_final_kmers",
    "bbk_extindex_build", "bbk_extindex_size", "bbk_extindex_k", "bbk_extindex_export", "bbk_extindex_clip_tips",
    "bbk_extindex_remove_at_edges", "bbk_extindex_remove_at_tips", "bbk_extindex_free",
    "bbk_unitigs_build", "bbk_unitigs_build_ex", "bbk_unitigs_to_reads", "bbk_unitigs_add_coverage", "bbk_unitigs_add_coverage_counts", "bbk_unitigs_export_kc", "bbk_unitigs_count", "bbk_unitigs_loops", "bbk_unitigs_total_bases",
    "bbk_unitigs_vertices", "bbk_unitigs_links", "bbk_unitigs_export", "bbk_unitigs_export_links",
    "bbk_unitigs_write_gfa", "bbk_unitigs_write_fasta", "bbk_unitigs_write_fastg", "bbk_unitigs_write_spades", "bbk_unitigs_free",
    "bbk_edgeindex_from_gfa", "bbk_edgeindex_from_unitigs", "bbk_edgeindex_segments", "bbk_edgeindex_size", "bbk_edgeindex_free",
    "bbk_profiles_begin", "bbk_profiles_push_reads", "bbk_profiles_export_raw", "bbk_profiles_write", "bbk_profiles_free",
    "bbk_edgeindex_map_paths", "bbk_edgeindex_from_gfa_with_graph", "bbk_paths_reads", "bbk_paths_ranges", "bbk_paths_export", "bbk_paths_free",
    "bbk_edgeindex_links", "bbk_edgeindex_total_bases", "bbk_edgeindex_name", "bbk_edgeindex_export_graph",
    "bbk_edgeindex_export_segments", "bbk_pairinfo_begin", "bbk_pairinfo_push_estimate", "bbk_pairinfo_estimate", "bbk_pairinfo_hist_size", "bbk_pairinfo_hist_export",
    "bbk_pairinfo_fill_begin", "bbk_pairinfo_push_fill", "bbk_pairinfo_fill_finish", "bbk_pairinfo_points", "bbk_pairinfo_export",
    "bbk_pairinfo_write", "bbk_pairinfo_free",
    "bbk_pairinfo_import", "bbk_pairinfo_cluster", "bbk_clustered_points", "bbk_clustered_pairs", "bbk_clustered_host_pairs",
    "bbk_clustered_export", "bbk_clustered_write", "bbk_clustered_free",
    "bbk_kmerprofile_begin", "bbk_kmerprofile_add_sample", "bbk_kmerprofile_finish", "bbk_kmerprofile_abort",
    "bbk_kmerprofile_size", "bbk_kmerprofile_samples", "bbk_kmerprofile_k", "bbk_kmerprofile_export",
    "bbk_kmerprofile_write", "bbk_kmerprofile_load", "bbk_kmerprofile_abundance", "bbk_kmerprofile_abundance_pieces",
    "bbk_kmerprofile_free",
    "bbk_kmerset_hamming_clusters", "bbk_hamclusters_count", "bbk_hamclusters_size", "bbk_hamclusters_replayed",
    "bbk_hamclusters_export", "bbk_hamclusters_write", "bbk_hamclusters_free",
    "bbk_quals_from_host", "bbk_quals_free", "bbk_kmerstats_begin", "bbk_kmerstats_push", "bbk_kmerstats_finish",
    "bbk_kmerstats_size", "bbk_kmerstats_export", "bbk_kmerstats_write", "bbk_kmerstats_free",
    "bbk_kmerstats_load", "bbk_hamclusters_load", "bbk_hamclusters_subcluster", "bbk_subclusters_count",
    "bbk_subclusters_size", "bbk_subclusters_new_kmers", "bbk_subclusters_host_kmers", "bbk_subclusters_export",
    "bbk_subclusters_write", "bbk_subclusters_free",
    "bbk_expander_from_subclusters", "bbk_expander_from_host", "bbk_expander_round_begin", "bbk_expander_push",
    "bbk_expander_round_end", "bbk_expander_run", "bbk_expander_good", "bbk_expander_export", "bbk_expander_store",
    "bbk_expander_free",
    "bbk_corrector_from_expander", "bbk_corrector_from_host", "bbk_corrector_limits", "bbk_corrector_correct",
    "bbk_corrector_stats", "bbk_corrector_free",
    "bbk_hreads_from_host", "bbk_hreads_size", "bbk_hreads_kmer_stretches", "bbk_hreads_corrector_stretches", "bbk_hreads_candidates",
    "bbk_hreads_export", "bbk_hreads_stretch_view", "bbk_hreads_candidate_view", "bbk_corrector_correct_prepared", "bbk_hreads_free",
    "bbk_corrector_correct_resident", "bbk_corrected_size", "bbk_corrected_export", "bbk_corrected_free", "bbk_corrected_print",
    "bbk_fastq_text_streams", "bbk_fastq_text_size", "bbk_fastq_text_export", "bbk_fastq_text_write", "bbk_fastq_text_free",
    "bbk_hreads_bases", "bbk_hreads_name_bytes", "bbk_hreads_export_records", "bbk_corrected_print_resident",
    "bbk_fastq_input_from_host", "bbk_fastq_input_records", "bbk_fastq_input_verdict", "bbk_fastq_input_text_end",
    "bbk_fastq_input_records_within", "bbk_fastq_input_free", "bbk_hreads_from_fastq_input",
    "bbk_group_create", "bbk_group_size", "bbk_group_device", "bbk_group_destroy", "bbk_group_abort", "bbk_group_exchange_kmers",
    "bbk_group_exchange_extindex", "bbk_group_gather_extindex", "bbk_group_gather_kmers", "bbk_ctx_memory_stats", "bbk_ctx_device_info", "bbk_kmerset_bucket_offsets",
]


class BBKError(RuntimeError):
    pass


def lib_path():
    # BBK_LIB selects an experimental build variant (python -m spades_for_blackbird_amd.build --suffix=...)
    return os.environ.get("BBK_LIB") or os.path.join(_HERE, "libbbk.so")


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64, libbbk.so links the system ones
    (/opt/rocm).  Two HSA runtimes cannot both drive the GPU from one process: whichever initialises second sees "no
    devices" (observed: engine first, then torch -> "No HIP GPUs are available").  Python users of this binding
    normally have torch in the process (bench.py, distributed.py), so when torch is installed its HIP runtime is put
    into the global symbol scope BEFORE libbbk.so is loaded and libbbk's hip* calls bind to it -- one runtime, in
    either order.  Without torch (or for the C++ CLIs) the system runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand) and not os.environ.get("BBK_SYSTEM_HIP"):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library():
    """Loads libbbk.so; raises BBKError if it has not been built (no fallback exists)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise BBKError("libbbk.so is missing: build it with `python -m spades_for_blackbird_amd.build` "
                       "(hipcc --offload-arch=gfx950); this engine has no CPU fallback")
    _share_torch_hip_runtime()
    L = C.CDLL(p)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    L.bbk_last_error.restype = C.c_char_p
    L.bbk_version.restype = C.c_char_p
    L.bbk_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.bbk_ctx_destroy.argtypes = [vp]
    L.bbk_ctx_set_stream.argtypes = [vp, vp]
    L.bbk_ctx_synchronize.argtypes = [vp]
    L.bbk_ctx_trim.argtypes = [vp]
    L.bbk_kmerset_verify_order.argtypes = [vp, vp, C.POINTER(u64), C.POINTER(u64), vp, C.c_uint]
    L.bbk_kmerset_get.argtypes = [vp, vp, u64, u64, vp, vp]
    L.bbk_ctx_profile_enable.argtypes = [vp, i32]
    L.bbk_ctx_profile_reset.argtypes = [vp]
    L.bbk_ctx_profile_get.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(C.c_double)]
    L.bbk_reads_from_ascii.argtypes = [vp, C.c_char_p, vp, u64, C.POINTER(vp)]
    L.bbk_reads_from_device.argtypes = [vp, vp, vp, vp, u64, u64, C.POINTER(vp)]
    L.bbk_reads_from_packed.argtypes = [vp, vp, u64, vp, u64, C.POINTER(vp)]
    L.bbk_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.bbk_host_free.argtypes = [vp]
    L.bbk_reads_synth.argtypes = [vp, u64, u32, u64, C.c_double, u64, u64, C.POINTER(vp)]
    L.bbk_reads_synth_meta.argtypes = [vp, u64, u32, u32, u64, u64, C.c_double, C.c_double, u64, C.POINTER(vp), vp, vp]
    L.bbk_reads_from_spades_binary.argtypes = [vp, C.c_char_p, C.POINTER(vp)]
    L.bbk_reads_write_spades_binary.argtypes = [vp, vp, C.c_char_p]
    L.bbk_reads_count.restype = u64
    L.bbk_reads_count.argtypes = [vp]
    L.bbk_reads_bases.restype = u64
    L.bbk_reads_bases.argtypes = [vp]
    L.bbk_reads_get_ascii.argtypes = [vp, vp, u64, C.c_char_p, u32, C.POINTER(u32)]
    L.bbk_reads_export_ascii.argtypes = [vp, vp, vp, vp, u64]
    L.bbk_reads_free.argtypes = [vp]
    L.bbk_count.argtypes = [vp, vp, C.c_uint, C.c_uint, C.POINTER(vp)]
    L.bbk_count_begin.argtypes = [vp, C.c_uint, C.c_uint, C.POINTER(vp)]
    L.bbk_count_push_reads.argtypes = [vp, vp]
    L.bbk_count_push_ascii.argtypes = [vp, C.c_char_p, vp, u64]
    L.bbk_count_finish.argtypes = [vp, C.POINTER(vp)]
    L.bbk_count_finish_min_count.argtypes = [vp, u32, C.POINTER(vp), C.POINTER(u64)]
    L.bbk_count_abort.argtypes = [vp]
    L.bbk_count_pushed_instances.restype = u64
    L.bbk_count_pushed_instances.argtypes = [vp]
    L.bbk_extindex_begin.argtypes = [vp, C.c_uint, C.POINTER(vp)]
    L.bbk_extindex_push_reads.argtypes = [vp, vp]
    L.bbk_extindex_finish.argtypes = [vp, C.POINTER(vp)]
    L.bbk_extindex_abort.argtypes = [vp]
    L.bbk_extindex_finish_with_set.argtypes = [vp, C.c_uint, C.POINTER(vp), C.POINTER(vp)]
    L.bbk_count_extindex.argtypes = [vp, vp, C.c_uint, C.c_uint, C.POINTER(vp), C.POINTER(vp)]
    L.bbk_kmerset_from_device.argtypes = [vp, vp, vp, u64, C.c_uint, C.POINTER(vp)]
    L.bbk_kmerset_from_device_ex.argtypes = [vp, vp, vp, u64, C.c_uint, C.c_uint, C.POINTER(vp)]
    L.bbk_kmerset_both_strands.argtypes = [vp, vp, C.POINTER(vp)]
    L.bbk_kmerset_both_strands_ex.argtypes = [vp, vp, C.c_uint, C.POINTER(vp)]
    L.bbk_words.restype = C.c_uint
    L.bbk_words.argtypes = [C.c_uint]
    L.bbk_kmerset_size.restype = u64
    L.bbk_kmerset_size.argtypes = [vp]
    L.bbk_kmerset_keys.restype = vp
    L.bbk_kmerset_keys.argtypes = [vp, C.POINTER(C.c_uint)]
    L.bbk_kmerset_k.restype = C.c_uint
    L.bbk_kmerset_k.argtypes = [vp]
    L.bbk_kmerset_instances.restype = u64
    L.bbk_kmerset_instances.argtypes = [vp]
    L.bbk_kmerset_export.argtypes = [vp, vp, C.c_uint, vp, vp]
    L.bbk_kmerset_export_by_owner.argtypes = [vp, vp, C.c_uint, vp, vp, vp]
    L.bbk_kmerset_free.argtypes = [vp]
    L.bbk_kmerset_write_final_kmers.argtypes = [vp, vp, C.c_char_p]
    if hasattr(L, "bbk_extindex_build"):
        L.bbk_extindex_build.argtypes = [vp, vp, C.c_uint, C.POINTER(vp)]
        L.bbk_extindex_size.restype = u64
        L.bbk_extindex_size.argtypes = [vp]
        L.bbk_extindex_k.restype = C.c_uint
        L.bbk_extindex_k.argtypes = [vp]
        L.bbk_extindex_export.argtypes = [vp, vp, vp, vp]
        L.bbk_extindex_export_u32.argtypes = [vp, vp, vp, vp]
        L.bbk_extindex_from_device.argtypes = [vp, vp, vp, u64, C.c_uint, C.POINTER(vp)]
        L.bbk_extindex_clip_tips.argtypes = [vp, vp, C.c_uint32, C.POINTER(u64), C.POINTER(u64)]
        L.bbk_extindex_remove_at_edges.argtypes = [vp, vp, C.c_double, C.POINTER(u64), C.POINTER(u64)]
        L.bbk_extindex_remove_at_tips.argtypes = [vp, vp, C.c_double, C.c_uint32, C.c_uint32, C.POINTER(u64),
                                                  C.POINTER(u64)]
        L.bbk_extindex_free.argtypes = [vp]
    if hasattr(L, "bbk_unitigs_build"):
        L.bbk_unitigs_build.argtypes = [vp, vp, C.POINTER(vp)]
        L.bbk_unitigs_build_ex.argtypes = [vp, vp, C.c_uint, C.POINTER(vp)]
        L.bbk_unitigs_to_reads.argtypes = [vp, vp, C.POINTER(vp)]
        for f in ("count", "loops", "total_bases", "vertices", "links"):
            getattr(L, "bbk_unitigs_" + f).restype = u64
            getattr(L, "bbk_unitigs_" + f).argtypes = [vp]
        L.bbk_unitigs_add_coverage.argtypes = [vp, vp, vp]
        L.bbk_unitigs_add_coverage_counts.argtypes = [vp, vp, vp]
        L.bbk_unitigs_export_kc.argtypes = [vp, vp, vp]
        L.bbk_unitigs_export.argtypes = [vp, vp, vp, vp]
        L.bbk_unitigs_export_links.argtypes = [vp, vp, vp]
        L.bbk_unitigs_write_gfa.argtypes = [vp, vp, C.c_char_p]
        L.bbk_unitigs_write_fasta.argtypes = [vp, vp, C.c_char_p]
        L.bbk_unitigs_write_fastg.argtypes = [vp, vp, C.c_char_p]
        L.bbk_unitigs_write_spades.argtypes = [vp, vp, C.c_char_p]
        L.bbk_unitigs_free.argtypes = [vp]
        L.bbk_edgeindex_from_gfa.argtypes = [vp, C.c_char_p, C.c_uint, C.POINTER(vp)]
        L.bbk_edgeindex_from_unitigs.argtypes = [vp, vp, C.POINTER(vp)]
        L.bbk_edgeindex_segments.restype = u64
        L.bbk_edgeindex_segments.argtypes = [vp]
        L.bbk_edgeindex_size.restype = u64
        L.bbk_edgeindex_size.argtypes = [vp]
        L.bbk_edgeindex_free.argtypes = [vp]
        L.bbk_profiles_begin.argtypes = [vp, vp, C.c_uint, C.POINTER(vp)]
        L.bbk_profiles_push_reads.argtypes = [vp, C.c_uint, vp]
        L.bbk_profiles_export_raw.argtypes = [vp, vp, vp]
        L.bbk_profiles_write.argtypes = [vp, vp, C.c_char_p]
        L.bbk_profiles_free.argtypes = [vp]
        L.bbk_edgeindex_map_paths.argtypes = [vp, vp, vp, C.POINTER(vp)]
        L.bbk_edgeindex_from_gfa_with_graph.argtypes = [vp, C.c_char_p, C.c_uint, C.POINTER(vp)]
        for f in ("reads", "ranges"):
            getattr(L, "bbk_paths_" + f).restype = u64
            getattr(L, "bbk_paths_" + f).argtypes = [vp]
        L.bbk_paths_export.argtypes = [vp, vp, vp, vp]
        L.bbk_paths_free.argtypes = [vp]
        L.bbk_paths_free.restype = None
        for f in ("links", "total_bases"):
            getattr(L, "bbk_edgeindex_" + f).restype = u64
            getattr(L, "bbk_edgeindex_" + f).argtypes = [vp]
        L.bbk_edgeindex_name.restype = C.c_char_p
        L.bbk_edgeindex_name.argtypes = [vp, u64]
        L.bbk_edgeindex_export_graph.argtypes = [vp, vp, vp, vp, vp]
        L.bbk_edgeindex_export_segments.argtypes = [vp, vp, vp]
        L.bbk_pairinfo_begin.argtypes = [vp, vp, u64, C.POINTER(vp)]
        L.bbk_pairinfo_push_estimate.argtypes = [vp, vp, vp, C.c_int, vp]
        L.bbk_pairinfo_estimate.argtypes = [vp, C.POINTER(PairInfoStats)]
        for f in ("hist_size", "points"):
            getattr(L, "bbk_pairinfo_" + f).restype = u64
            getattr(L, "bbk_pairinfo_" + f).argtypes = [vp]
        L.bbk_pairinfo_hist_export.argtypes = [vp, vp, vp]
        L.bbk_pairinfo_fill_begin.argtypes = [vp, u64, C.c_uint, C.c_uint]
        L.bbk_pairinfo_push_fill.argtypes = [vp, vp, vp, C.c_int, vp]
        L.bbk_pairinfo_fill_finish.argtypes = [vp]
        L.bbk_pairinfo_export.argtypes = [vp, vp, vp, vp, vp]
        L.bbk_pairinfo_write.argtypes = [vp, C.c_char_p]
        L.bbk_pairinfo_free.argtypes = [vp]
        L.bbk_pairinfo_import.argtypes = [vp, vp, u64, vp, vp, vp, vp, C.POINTER(vp)]
        L.bbk_pairinfo_cluster.argtypes = [vp, C.POINTER(ClusterParams), C.POINTER(vp)]
        for f in ("points", "pairs", "host_pairs"):
            getattr(L, "bbk_clustered_" + f).restype = u64
            getattr(L, "bbk_clustered_" + f).argtypes = [vp]
        L.bbk_clustered_export.argtypes = [vp, vp, vp, vp, vp, vp]
        L.bbk_clustered_write.argtypes = [vp, C.c_char_p]
        L.bbk_clustered_free.argtypes = [vp]
    L.bbk_kmerprofile_begin.argtypes = [vp, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.POINTER(vp)]
    L.bbk_kmerprofile_add_sample.argtypes = [vp, C.c_uint, vp]
    L.bbk_kmerprofile_finish.argtypes = [vp, u64, u64, C.POINTER(vp)]
    L.bbk_kmerprofile_abort.argtypes = [vp]
    L.bbk_kmerprofile_abort.restype = None
    L.bbk_kmerprofile_size.restype = u64
    L.bbk_kmerprofile_size.argtypes = [vp]
    L.bbk_kmerprofile_samples.restype = C.c_uint
    L.bbk_kmerprofile_samples.argtypes = [vp]
    L.bbk_kmerprofile_k.restype = C.c_uint
    L.bbk_kmerprofile_k.argtypes = [vp]
    L.bbk_kmerprofile_export.argtypes = [vp, vp, vp, vp]
    L.bbk_kmerprofile_write.argtypes = [vp, vp, C.c_char_p]
    L.bbk_kmerprofile_load.argtypes = [vp, C.c_char_p, C.c_uint, C.c_uint, C.POINTER(vp)]
    L.bbk_kmerprofile_abundance.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.bbk_kmerprofile_abundance_pieces.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp]
    L.bbk_kmerprofile_free.argtypes = [vp]
    L.bbk_kmerprofile_free.restype = None
    L.bbk_kmerset_hamming_clusters.argtypes = [vp, vp, C.c_uint, u64, u64, C.POINTER(vp)]
    for f in ("count", "size", "replayed"):
        getattr(L, "bbk_hamclusters_" + f).restype = u64
        getattr(L, "bbk_hamclusters_" + f).argtypes = [vp]
    L.bbk_hamclusters_export.argtypes = [vp, vp, vp, vp, vp]
    L.bbk_hamclusters_write.argtypes = [vp, vp, C.c_char_p]
    L.bbk_hamclusters_free.argtypes = [vp]
    L.bbk_hamclusters_free.restype = None
    L.bbk_quals_from_host.argtypes = [vp, vp, vp, vp, u64, C.POINTER(vp)]
    L.bbk_quals_free.argtypes = [vp]
    L.bbk_quals_free.restype = None
    L.bbk_kmerstats_begin.argtypes = [vp, vp, C.POINTER(vp)]
    L.bbk_kmerstats_push.argtypes = [vp, vp, vp]
    L.bbk_kmerstats_finish.argtypes = [vp]
    L.bbk_kmerstats_size.restype = u64
    L.bbk_kmerstats_size.argtypes = [vp]
    L.bbk_kmerstats_export.argtypes = [vp, vp, vp, vp, vp]
    L.bbk_kmerstats_write.argtypes = [vp, vp, C.c_char_p]
    L.bbk_kmerstats_free.argtypes = [vp]
    L.bbk_kmerstats_free.restype = None
    L.bbk_kmerstats_load.argtypes = [vp, vp, C.c_char_p, C.POINTER(vp)]
    L.bbk_hamclusters_load.argtypes = [vp, u64, C.c_char_p, C.POINTER(vp)]
    L.bbk_hamclusters_subcluster.argtypes = [vp, vp, vp, vp, vp, C.POINTER(vp)]
    for f in ("count", "size", "new_kmers", "host_kmers"):
        getattr(L, "bbk_subclusters_" + f).restype = u64
        getattr(L, "bbk_subclusters_" + f).argtypes = [vp]
    L.bbk_subclusters_export.argtypes = [vp] * 10
    L.bbk_subclusters_write.argtypes = [vp, vp, vp, C.c_char_p]
    L.bbk_subclusters_free.argtypes = [vp]
    L.bbk_subclusters_free.restype = None
    L.bbk_expander_from_subclusters.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.bbk_expander_from_host.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.bbk_expander_round_begin.argtypes = [vp]
    L.bbk_expander_push.argtypes = [vp, vp, vp]
    L.bbk_expander_round_end.argtypes = [vp, C.POINTER(u64)]
    L.bbk_expander_run.argtypes = [vp, vp, C.c_uint, u64, C.POINTER(C.c_uint), vp]
    L.bbk_expander_good.restype = u64
    L.bbk_expander_good.argtypes = [vp]
    L.bbk_expander_export.argtypes = [vp, vp, vp]
    L.bbk_expander_store.argtypes = [vp, vp]
    L.bbk_expander_free.argtypes = [vp]
    L.bbk_expander_free.restype = None
    L.bbk_corrector_from_expander.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.bbk_corrector_from_host.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.bbk_corrector_limits.argtypes = [C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.bbk_corrector_limits.restype = None
    L.bbk_corrector_correct.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp]
    L.bbk_corrector_stats.argtypes = [vp, vp]
    L.bbk_corrector_free.argtypes = [vp]
    L.bbk_corrector_free.restype = None
    L.bbk_hreads_from_host.argtypes = [vp, vp, vp, vp, u64, C.c_uint, C.c_int, C.POINTER(vp)]
    for f in ("size", "kmer_stretches", "corrector_stretches", "candidates"):
        getattr(L, "bbk_hreads_" + f).restype = u64
        getattr(L, "bbk_hreads_" + f).argtypes = [vp]
    L.bbk_hreads_export.argtypes = [vp] * 8
    L.bbk_hreads_stretch_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.bbk_hreads_candidate_view.argtypes = [vp, C.POINTER(vp)]
    L.bbk_corrector_correct_prepared.argtypes = [vp] * 6
    L.bbk_hreads_free.argtypes = [vp]
    L.bbk_hreads_free.restype = None
    L.bbk_corrector_correct_resident.argtypes = [vp, vp, C.POINTER(vp)]
    L.bbk_corrected_size.restype = u64
    L.bbk_corrected_size.argtypes = [vp]
    L.bbk_corrected_export.argtypes = [vp] * 8
    L.bbk_corrected_free.argtypes = [vp]
    L.bbk_corrected_free.restype = None
    L.bbk_corrected_print.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.bbk_fastq_text_streams.argtypes = [vp]
    L.bbk_fastq_text_size.restype = u64
    L.bbk_fastq_text_size.argtypes = [vp, C.c_int]
    L.bbk_fastq_text_export.argtypes = [vp, vp, C.c_int, vp]
    L.bbk_fastq_text_write.argtypes = [vp, vp, C.c_int, C.c_char_p, C.c_int]
    L.bbk_fastq_text_free.argtypes = [vp]
    L.bbk_fastq_text_free.restype = None
    for f in ("bases", "name_bytes"):
        getattr(L, "bbk_hreads_" + f).restype = u64
        getattr(L, "bbk_hreads_" + f).argtypes = [vp]
    L.bbk_hreads_export_records.argtypes = [vp] * 7
    L.bbk_corrected_print_resident.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.bbk_fastq_input_from_host.argtypes = [vp, vp, u64, C.c_int, C.c_int, C.POINTER(vp)]
    L.bbk_fastq_input_records.restype = u64
    L.bbk_fastq_input_records.argtypes = [vp]
    L.bbk_fastq_input_verdict.argtypes = [vp, C.POINTER(u64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.bbk_fastq_input_text_end.restype = u64
    L.bbk_fastq_input_text_end.argtypes = [vp, u64]
    L.bbk_fastq_input_records_within.restype = u64
    L.bbk_fastq_input_records_within.argtypes = [vp, u64, u64]
    L.bbk_fastq_input_free.argtypes = [vp]
    L.bbk_fastq_input_free.restype = None
    L.bbk_hreads_from_fastq_input.argtypes = [vp, u64, u64, C.c_uint, C.c_int, C.POINTER(vp)]
    L.bbk_group_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_uint, C.POINTER(vp)]
    L.bbk_group_size.argtypes = [vp]
    L.bbk_group_device.argtypes = [vp, C.c_int]
    L.bbk_group_destroy.argtypes = [vp]
    L.bbk_group_destroy.restype = None
    L.bbk_group_abort.argtypes = [vp]
    L.bbk_group_abort.restype = None
    L.bbk_group_exchange_kmers.argtypes = [vp, C.c_int, vp, vp, C.c_uint, C.POINTER(vp)]
    L.bbk_group_exchange_extindex.argtypes = [vp, C.c_int, vp, vp, C.POINTER(vp)]
    L.bbk_group_gather_extindex.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.POINTER(vp)]
    L.bbk_group_gather_kmers.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.POINTER(vp)]
    L.bbk_ctx_memory_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64)]
    L.bbk_ctx_device_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.bbk_kmerset_bucket_offsets.argtypes = [vp, vp, vp]
    _LIB = L
    return L


def _check(rc):
    if rc != 0:
        raise BBKError("bbk error %d: %s" % (rc, load_library().bbk_last_error().decode(errors="replace")))


def _ptr(x):
    """Host numpy array, torch tensor (host or device) or raw int -> void pointer."""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError("cannot take a pointer of %r" % type(x))


def words(k):
    return (k + 31) // 32


class Context:
    """One per GPU / process (bbk_ctx)."""

    def __init__(self, device=0, stream=None):
        self._L = load_library()
        h = C.c_void_p()
        _check(self._L.bbk_ctx_create(device, C.byref(h)))
        self._h = h
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, stream):
        """stream: raw hipStream_t as int, or a torch.cuda.Stream."""
        raw = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        _check(self._L.bbk_ctx_set_stream(self._h, C.c_void_p(raw)))

    def synchronize(self):
        _check(self._L.bbk_ctx_synchronize(self._h))

    def trim(self):
        """Gives the device memory the allocator holds but does not use back to the driver (free chunks at the end of
        the calling thread's arena are unmapped and released).  The next calls map what they need again: ~30 ms/GiB
        when the driver has to clear the memory first -- trim when another process or library needs the memory, not
        between the steps of a loop."""
        _check(self._L.bbk_ctx_trim(self._h))

    def memory_stats(self):
        """dict(mapped_now, mapped_total, map_seconds, device_free, device_total) of this thread's allocator / device"""
        a, b, f, t = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        sec = C.c_double()
        _check(self._L.bbk_ctx_memory_stats(self._h, C.byref(a), C.byref(b), C.byref(sec), C.byref(f), C.byref(t)))
        return {"mapped_now": a.value, "mapped_total": b.value, "map_seconds": sec.value, "device_free": f.value,
                "device_total": t.value}

    def device_info(self):
        """{'num_cus', 'num_xcds'}: what the engine found at context creation (8 XCDs switch the XCD-local fill fronts on)"""
        a, b = C.c_int(), C.c_int()
        _check(self._L.bbk_ctx_device_info(self._h, C.byref(a), C.byref(b)))
        return {"num_cus": a.value, "num_xcds": b.value}

    def profile(self, on=True):
        _check(self._L.bbk_ctx_profile_enable(self._h, int(on)))

    def profile_reset(self):
        _check(self._L.bbk_ctx_profile_reset(self._h))

    def profile_get(self, family):
        ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
        _check(self._L.bbk_ctx_profile_get(self._h, family.encode(), C.byref(ms), C.byref(n), C.byref(b)))
        return {"ms": ms.value, "launches": n.value, "bytes": b.value}

    # ---- reads -------------------------------------------------------------------------------
    def reads_from_ascii(self, reads):
        bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
        offs = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        return self.reads_from_blob(b"".join(bs), offs)

    def reads_from_blob(self, blob, offsets):
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        _check(self._L.bbk_reads_from_ascii(self._h, blob, _ptr(offsets), len(offsets) - 1, C.byref(h)))
        return Reads(self, h)

    def reads_from_packed(self, words, lens):
        """Host-packed reads (numpy uint64 words, uint32 lengths; every read starts on a word)."""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        h = C.c_void_p()
        _check(self._L.bbk_reads_from_packed(self._h, _ptr(words), len(words), _ptr(lens), len(lens), C.byref(h)))
        return Reads(self, h)

    def reads_from_device(self, d_words, d_word_off, d_len, n_reads, n_words):
        h = C.c_void_p()
        _check(self._L.bbk_reads_from_device(self._h, _ptr(d_words), _ptr(d_word_off), _ptr(d_len), n_reads, n_words,
                                             C.byref(h)))
        r = Reads(self, h)
        r._keep = (d_words, d_word_off, d_len)
        return r

    def reads_from_spades_binary(self, seq_path):
        """SPAdes binary read cache (<prefix>.seq)."""
        h = C.c_void_p()
        _check(self._L.bbk_reads_from_spades_binary(self._h, seq_path.encode(), C.byref(h)))
        return Reads(self, h)

    def reads_synth(self, n_reads, read_len=150, genome_len=None, sub_rate=0.005, seed_genome=42, seed_reads=43):
        if genome_len is None:
            genome_len = max(read_len, n_reads * read_len // 50)
        h = C.c_void_p()
        _check(self._L.bbk_reads_synth(self._h, n_reads, read_len, genome_len, sub_rate, seed_genome, seed_reads,
                                       C.byref(h)))
        return Reads(self, h)

    def reads_synth_meta(self, n_reads, read_len=150, n_genomes=200, min_len=500_000, max_len=8_000_000, sigma=2.0,
                         sub_rate=0.005, seed=44, want_community=False):
        """Metagenome-shaped reads (SURVEY 8d / BASELINE configs[4]); want_community: also (genome lengths, abundances)."""
        h = C.c_void_p()
        gl = np.zeros(n_genomes, dtype=np.uint64)
        ab = np.zeros(n_genomes, dtype=np.float64)
        _check(self._L.bbk_reads_synth_meta(self._h, n_reads, read_len, n_genomes, min_len, max_len, sigma, sub_rate, seed,
                                            C.byref(h), _ptr(gl), _ptr(ab)))
        r = Reads(self, h)
        return (r, gl, ab) if want_community else r

    # ---- operators -----------------------------------------------------------------------------
    def count(self, reads, k, flags=BOTH_STRANDS):
        """KMerCounter::Count analogue (reference kmer_index_builder.hpp:195-217)."""
        h = C.c_void_p()
        _check(self._L.bbk_count(self._h, reads._h, k, flags, C.byref(h)))
        return KMerSet(self, h)

    def counter(self, k, flags=BOTH_STRANDS):
        """Streaming count (bbk_count_begin / push / finish): KMerSortingSplitter's bounded rounds + MergeKMers."""
        return Counter(self, k, flags)

    def extbuilder(self, k):
        """Streaming extension-index build (bbk_extindex_begin / push / finish)."""
        return ExtBuilder(self, k)

    def kmerset_from_device(self, d_keys, n, k, d_counts=None, flags=0):
        h = C.c_void_p()
        _check(self._L.bbk_kmerset_from_device_ex(self._h, _ptr(d_keys), _ptr(d_counts), n, k, flags, C.byref(h)))
        return KMerSet(self, h)

    def median_filter(self, reads, counts, threshold):
        """CoverageFilter::CheckMedianMlt for every read: uint8[n] (1 = keep), see bbk_reads_median_filter."""
        keep = np.zeros(len(reads), dtype=np.uint8)
        kept = C.c_uint64(0)
        self._L.bbk_reads_median_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p,
                                                    C.POINTER(C.c_uint64)]
        _check(self._L.bbk_reads_median_filter(self._h, reads._h, counts._h, threshold, _ptr(keep), C.byref(kept)))
        assert int(kept.value) == int(keep.sum())
        return keep

    def quals(self, reads, qual_bytes, offsets):
        """Qualities of `reads` (offset already subtracted): qual_bytes uint8, read i at [offsets[i], offsets[i + 1]);
        every length must equal the read's.  The reads must outlive the result."""
        q = np.ascontiguousarray(np.frombuffer(qual_bytes, dtype=np.uint8) if isinstance(qual_bytes, (bytes, bytearray))
                                 else qual_bytes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        _check(self._L.bbk_quals_from_host(self._h, reads._h, _ptr(q), _ptr(offsets), len(offsets) - 1, C.byref(h)))
        r = Quals(self, h)
        r._reads = reads
        return r

    def hammer_reads(self, bases, quals, offsets, k, trim_quality=4):
        """FASTQ records as parsed -> HammerReads: bases and quals uint8 back to back (any byte values; qualities with the
        offset already subtracted, at most 93), record i at [offsets[i], offsets[i + 1]).  trim_quality=NO_TRIM: the records
        are trimmed already and are taken whole."""
        b = np.ascontiguousarray(np.frombuffer(bases, dtype=np.uint8) if isinstance(bases, (bytes, bytearray)) else bases,
                                 dtype=np.uint8)
        q = np.ascontiguousarray(np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else quals,
                                 dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if len(offsets) < 1 or len(b) != len(q) or (len(offsets) > 1 and int(offsets.max()) > len(b)):
            raise ValueError("hammer_reads: %d bases, %d qualities, offsets up to %d"
                             % (len(b), len(q), int(offsets.max()) if len(offsets) else -1))
        h = C.c_void_p()
        _check(self._L.bbk_hreads_from_host(self._h, _ptr(b), _ptr(q), _ptr(offsets), len(offsets) - 1, k, trim_quality,
                                            C.byref(h)))
        r = HammerReads(self, h)
        r.k, r.bases = k, len(b)
        return r

    def fastq_input(self, text, final=True, qvoffset=33):
        """One chunk of FASTQ text (bytes, after any gunzip) -> FastqInput: the text on the device with the index of its
        records.  final=False: the text goes on in a later chunk, and only terminated lines count."""
        t = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview))
                                 else text, dtype=np.uint8)
        h = C.c_void_p()
        _check(self._L.bbk_fastq_input_from_host(self._h, _ptr(t), len(t), 1 if final else 0, int(qvoffset), C.byref(h)))
        return FastqInput(self, h)

    def extindex(self, reads, k):
        """DeBruijnExtensionIndexBuilder::BuildExtensionIndexFromStream analogue."""
        h = C.c_void_p()
        _check(self._L.bbk_extindex_build(self._h, reads._h, k, C.byref(h)))
        return ExtIndex(self, h)

    def count_extindex(self, reads, k, flags=BOTH_STRANDS):
        """k-mer set (both strands) and extension index from ONE pass over the reads: (KMerSet, ExtIndex)"""
        hs, hx = C.c_void_p(), C.c_void_p()
        _check(self._L.bbk_count_extindex(self._h, reads._h, k, flags, C.byref(hs), C.byref(hx)))
        return KMerSet(self, hs), ExtIndex(self, hx)

    def extindex_from_device(self, d_keys, d_masks_u32, n, k):
        """Index of (canonical k-mer, u32 mask) records in HBM: any order, duplicates OR-ed (a shard after the exchange)."""
        h = C.c_void_p()
        _check(self._L.bbk_extindex_from_device(self._h, _ptr(d_keys), _ptr(d_masks_u32), n, k, C.byref(h)))
        return ExtIndex(self, h)

    def unitigs(self, ext, ref_threads=0):
        """UnbranchingPathExtractor + FastGraphFromSequencesConstructor analogue.  ref_threads > 0: perfect loops are
        collected in the k-mer file order of a reference run with that -t (loop rotation, SplitLoop choice)."""
        h = C.c_void_p()
        _check(self._L.bbk_unitigs_build_ex(self._h, ext._h, ref_threads, C.byref(h)))
        return Unitigs(self, h)

    def edgeindex_from_gfa(self, path, k, keep_graph=False):
        """(k+1)-mer index of a GFA graph for unitig-coverage: S lines are the segments, L lines must be kM overlaps.
        keep_graph: the index also keeps the bases, links and KC (EdgeIndex.graph)."""
        h = C.c_void_p()
        f = self._L.bbk_edgeindex_from_gfa_with_graph if keep_graph else self._L.bbk_edgeindex_from_gfa
        _check(f(self._h, path.encode(), k, C.byref(h)))
        return EdgeIndex(self, h)

    def edgeindex_from_unitigs(self, unitigs):
        """the same index of an in-process graph (segment i named 3 + 2i, as in its GFA)"""
        h = C.c_void_p()
        _check(self._L.bbk_edgeindex_from_unitigs(self._h, unitigs._h, C.byref(h)))
        return EdgeIndex(self, h)

    def kmerprofile(self, k, sets, min_samples, min_mult=5, ci=2, cs=255):
        """KmerMultiplicityCounter::FilterCombinedKmers: the join of one ascending canonical KMerSet with counts per
        sample (count(reads, k, CANONICAL | WITH_COUNTS)) into a KmerProfile.  ci / cs: KMC's per-sample filter."""
        b = C.c_void_p()
        _check(self._L.bbk_kmerprofile_begin(self._h, k, len(sets), ci, cs, C.byref(b)))
        try:
            for i, s in enumerate(sets):
                _check(self._L.bbk_kmerprofile_add_sample(b, i, s._h))
        except Exception:
            self._L.bbk_kmerprofile_abort(b)
            raise
        h = C.c_void_p()
        _check(self._L.bbk_kmerprofile_finish(b, min_samples, min_mult, C.byref(h)))
        return KmerProfile(self, h)

    def kmerprofile_load(self, prefix, k, n_samples):
        """the <prefix>.kmers / <prefix>.bpr pair KmerProfile.write leaves"""
        h = C.c_void_p()
        _check(self._L.bbk_kmerprofile_load(self._h, str(prefix).encode(), k, n_samples, C.byref(h)))
        return KmerProfile(self, h)

    def kmerstats_load(self, kmer_set, path):
        """the inverse of KmerStats.write: the statistics of every k-mer of kmer_set from a .kmstat file"""
        h = C.c_void_p()
        _check(self._L.bbk_kmerstats_load(self._h, kmer_set._h, str(path).encode(), C.byref(h)))
        ks = KmerStats(self, h)
        ks._set, ks.k = kmer_set, kmer_set.k
        return ks

    def hamclusters_load(self, n, path):
        """the inverse of HamClusters.write: <path> and <path>.idx for a set of n k-mers, clusters in any order"""
        h = C.c_void_p()
        _check(self._L.bbk_hamclusters_load(self._h, n, str(path).encode(), C.byref(h)))
        return HamClusters(self, h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.bbk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Handle:
    _free = None

    def __init__(self, ctx, h):
        self.ctx, self._h, self._L = ctx, h, ctx._L

    def free(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                getattr(self._L, self._free)(self._h)
            self._h = None

    @classmethod
    def borrowed(cls, ctx, h, owner):
        """a handle the library object `owner` owns: never freed from here, and `owner` is kept alive with it"""
        x = cls(ctx, h)
        x._borrowed, x._owner = True, owner
        return x

    def close(self):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Reads(_Handle):
    _free = "bbk_reads_free"

    def __len__(self):
        return int(self._L.bbk_reads_count(self._h))

    @property
    def bases(self):
        return int(self._L.bbk_reads_bases(self._h))

    def to_ascii(self):
        """(blob bytes, offsets np.uint64[n+1])"""
        n = len(self)
        offs = np.zeros(n + 1, dtype=np.uint64)
        _check(self._L.bbk_reads_export_ascii(self.ctx._h, self._h, None, _ptr(offs), 0))
        total = int(offs[n])
        buf = np.zeros(total + 1, dtype=np.uint8)
        _check(self._L.bbk_reads_export_ascii(self.ctx._h, self._h, _ptr(buf), _ptr(offs), total))
        return buf[:total].tobytes(), offs

    def write_spades_binary(self, prefix):
        _check(self._L.bbk_reads_write_spades_binary(self.ctx._h, self._h, prefix.encode()))

    def to_list(self):
        blob, offs = self.to_ascii()
        return [blob[int(offs[i]):int(offs[i + 1])].decode() for i in range(len(offs) - 1)]


class KMerSet(_Handle):
    _free = "bbk_kmerset_free"

    def __len__(self):
        return int(self._L.bbk_kmerset_size(self._h))

    @property
    def k(self):
        return int(self._L.bbk_kmerset_k(self._h))

    @property
    def instances(self):
        return int(self._L.bbk_kmerset_instances(self._h))

    def device_keys(self):
        """(device pointer of the records, order they are stored in); valid until the set is freed."""
        o = C.c_uint(0)
        p = self._L.bbk_kmerset_keys(self._h, C.byref(o))
        return p, int(o.value)

    def both_strands(self, flags=0):
        """canon U rc(canon); flags=REFERENCE_ORDER stores it in the final_kmers order."""
        h = C.c_void_p()
        _check(self._L.bbk_kmerset_both_strands_ex(self.ctx._h, self._h, flags, C.byref(h)))
        return KMerSet(self.ctx, h)

    def export(self, order=ORDER_SORTED, with_counts=False):
        n, nw = len(self), words(self.k)
        keys = np.zeros((n, nw), dtype=np.uint64)
        cnt = np.zeros(n, dtype=np.uint32) if with_counts else None
        _check(self._L.bbk_kmerset_export(self.ctx._h, self._h, order, _ptr(keys), _ptr(cnt)))
        return (keys, cnt) if with_counts else keys

    def export_to(self, dst_keys, order=ORDER_SORTED, dst_counts=None):
        """dst_*: preallocated torch tensors (device or host) or numpy arrays."""
        _check(self._L.bbk_kmerset_export(self.ctx._h, self._h, order, _ptr(dst_keys), _ptr(dst_counts)))

    def export_by_owner(self, nranks, dst_keys=None, dst_counts=None):
        n, nw = len(self), words(self.k)
        counts = np.zeros(nranks, dtype=np.uint64)
        ret = None
        if dst_keys is None:
            dst_keys = ret = np.zeros((n, nw), dtype=np.uint64)
        _check(self._L.bbk_kmerset_export_by_owner(self.ctx._h, self._h, nranks, _ptr(dst_keys), _ptr(dst_counts),
                                                   _ptr(counts)))
        return (ret, counts) if ret is not None else counts

    def verify_order(self):
        """(ascending runs of the stored order, equal neighbours, start index of the first runs) -- on the device"""
        runs, eq = C.c_uint64(), C.c_uint64()
        starts = np.zeros(33, dtype=np.uint64)
        _check(self._L.bbk_kmerset_verify_order(self.ctx._h, self._h, C.byref(runs), C.byref(eq), _ptr(starts), 33))
        return int(runs.value), int(eq.value), [int(x) for x in starts[:min(int(runs.value), 33)]]

    def get(self, first, count, with_counts=False):
        keys = np.zeros((count, words(self.k)), dtype=np.uint64)
        cnt = np.zeros(count, dtype=np.uint32) if with_counts else None
        _check(self._L.bbk_kmerset_get(self.ctx._h, self._h, first, count, _ptr(keys), _ptr(cnt)))
        return (keys, cnt) if with_counts else keys

    def write_final_kmers(self, path):
        _check(self._L.bbk_kmerset_write_final_kmers(self.ctx._h, self._h, path.encode()))

    def hamming_clusters(self, lock_size=0, chunk=0, tau=1):
        """TauOneKMerHamClusterer::cluster over this ascending both-strand set (k <= 32): HamClusters.  lock_size /
        chunk: 0 = the reference's 2500 / 65536."""
        h = C.c_void_p()
        _check(self._L.bbk_kmerset_hamming_clusters(self.ctx._h, self._h, tau, lock_size, chunk, C.byref(h)))
        return HamClusters(self.ctx, h)

    def kmer_stats(self):
        """KMerData over this ascending both-strand set (k <= 32): KmerStats, all empty; the set must outlive it."""
        h = C.c_void_p()
        _check(self._L.bbk_kmerstats_begin(self.ctx._h, self._h, C.byref(h)))
        ks = KmerStats(self.ctx, h)
        ks._set, ks.k = self, self.k
        return ks

    def expander(self, good):
        """Expander over this ascending both-strand set (k <= 32) from the good bit of every k-mer: `good` is one byte
        per k-mer, 0 or 1.  The set must outlive it."""
        good = np.ascontiguousarray(good, dtype=np.uint8)
        if good.shape != (len(self),):
            raise ValueError("one good byte per k-mer of the set: %d, not %r" % (len(self), good.shape))
        h = C.c_void_p()
        _check(self._L.bbk_expander_from_host(self.ctx._h, self._h, _ptr(good), C.byref(h)))
        e = Expander(self.ctx, h)
        e._set = self
        return e

    def corrector(self, good):
        """Corrector over this ascending both-strand set (k <= 32) from the good bit of every k-mer (one byte each, 0 or
        1).  The set must outlive it."""
        good = np.ascontiguousarray(good, dtype=np.uint8)
        if good.shape != (len(self),):
            raise ValueError("one good byte per k-mer of the set: %d, not %r" % (len(self), good.shape))
        h = C.c_void_p()
        _check(self._L.bbk_corrector_from_host(self.ctx._h, self._h, _ptr(good), C.byref(h)))
        c = Corrector(self.ctx, h)
        c._set = self
        return c


KmerSet = KMerSet


class Quals(_Handle):
    """one quality byte per base of a Reads (offset already subtracted)"""
    _free = "bbk_quals_free"


class HammerReads(_Handle):
    """A batch of FASTQ records prepared on the device (bbk_hreads_*): what Read::trimNsAndBadQuality leaves of every
    record, the valid k-mer starts of ValidKMerGenerator as stretches, and the records the Expander can find solid."""
    _free = "bbk_hreads_free"

    def __len__(self):
        return int(self._L.bbk_hreads_size(self._h))

    def trims(self):
        """np.uint32[n, 2]: (start, length) of the trimmed read in the record as parsed; (0, 0): nothing is left"""
        t = np.zeros((len(self), 2), dtype=np.uint32)
        _check(self._L.bbk_hreads_export(self.ctx._h, self._h, _ptr(t), None, None, None, None, None))
        return t

    def candidates(self):
        """np.uint8[n]: 1 where the valid starts cover the whole trimmed read (host/hammer_reads.hpp: expander_candidate)"""
        c = np.zeros(len(self), dtype=np.uint8)
        _check(self._L.bbk_hreads_export(self.ctx._h, self._h, None, _ptr(c), None, None, None, None))
        return c

    def stretches(self, table="kmer"):
        """(offsets np.uint64[n + 1], stretches np.uint32[S, 2]): the (start, length) stretches of record i are rows
        offsets[i] .. offsets[i + 1].  table "kmer": ACGTacgt are nucleotides, starts in the record as parsed, nothing
        for a trimmed read shorter than k; "corrector": ACGT only, starts in the trimmed read."""
        if table not in ("kmer", "corrector"):
            raise ValueError("table is 'kmer' or 'corrector', not %r" % (table,))
        kmer = table == "kmer"
        s = int((self._L.bbk_hreads_kmer_stretches if kmer else self._L.bbk_hreads_corrector_stretches)(self._h))
        off = np.zeros(len(self) + 1, dtype=np.uint64)
        st = np.zeros((s, 2), dtype=np.uint32)
        a = (_ptr(off), _ptr(st), None, None) if kmer else (None, None, _ptr(off), _ptr(st))
        _check(self._L.bbk_hreads_export(self.ctx._h, self._h, None, None, *a))
        return off, st

    def records(self):
        """(bases np.uint8, quals np.uint8, offsets np.uint64[n + 1], names np.uint8, name offsets np.uint64[n + 1]): the
        records as the batch holds them, qualities with the offset subtracted; a batch made from host arrays has no names"""
        n = len(self)
        b = np.zeros(int(self._L.bbk_hreads_bases(self._h)), dtype=np.uint8)
        q = np.zeros(len(b), dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        names = np.zeros(int(self._L.bbk_hreads_name_bytes(self._h)), dtype=np.uint8)
        noff = np.zeros(n + 1, dtype=np.uint64)
        _check(self._L.bbk_hreads_export_records(self.ctx._h, self._h, _ptr(b), _ptr(q), _ptr(off), _ptr(names), _ptr(noff)))
        return b, q, off, names, noff

    def stretch_view(self):
        """(Reads, Quals) the batch owns: one engine read per k-mer stretch, for Counter.push and KmerStats.push"""
        r, q = C.c_void_p(), C.c_void_p()
        _check(self._L.bbk_hreads_stretch_view(self._h, C.byref(r), C.byref(q)))
        return Reads.borrowed(self.ctx, r, self), Quals.borrowed(self.ctx, q, self)

    def candidate_view(self):
        """Reads the batch owns: the trimmed read of every candidate, for Expander.push / Expander.run"""
        r = C.c_void_p()
        _check(self._L.bbk_hreads_candidate_view(self._h, C.byref(r)))
        return Reads.borrowed(self.ctx, r, self)


class FastqInput(_Handle):
    """One chunk of FASTQ text on the device with the index of its records (bbk_fastq_input_*): record r is lines
    4r .. 4r + 3, judged against the strict four-line form; the verdict is the first record the device does not take."""
    _free = "bbk_fastq_input_free"
    FORM, QUALITY = 1, 2  # BBK_FASTQ_FORM, BBK_FASTQ_QUALITY

    @property
    def records(self):
        """complete records of the chunk: lines // 4"""
        return int(self._L.bbk_fastq_input_records(self._h))

    def verdict(self):
        """None, or (record, kind, byte): the first record that is not in the strict form (FORM) or holds a quality
        character outside [qvoffset, qvoffset + 93] (QUALITY: byte is that character, otherwise -1)"""
        r, k, b = C.c_uint64(), C.c_int(), C.c_int()
        if not self._L.bbk_fastq_input_verdict(self._h, C.byref(r), C.byref(k), C.byref(b)):
            return None
        return int(r.value), int(k.value), int(b.value)

    def text_end(self, n):
        """the byte just past record n - 1: where the next chunk starts, or where a serial reader resumes"""
        e = int(self._L.bbk_fastq_input_text_end(self._h, n))
        if e == 2 ** 64 - 1:
            raise ValueError("text_end(%d): the chunk has %d records" % (n, self.records))
        return e

    def records_within(self, first, max_bases):
        """records from `first` up to and including the one at which their bases reach max_bases (all the records
        before the verdict when they do not)"""
        return int(self._L.bbk_fastq_input_records_within(self._h, first, max_bases))

    def hammer_reads(self, first, n, k, trim_quality=4):
        """records [first, first + n), which lie before the verdict, gathered and prepared on the device -> HammerReads
        with names"""
        h = C.c_void_p()
        _check(self._L.bbk_hreads_from_fastq_input(self._h, first, n, k, trim_quality, C.byref(h)))
        r = HammerReads(self.ctx, h)
        r.k, r.bases = k, int(self._L.bbk_hreads_bases(h))
        return r


class KmerStats(_Handle):
    """BayesHammer's KMerStat of every k-mer of a set: count, total_qual and the saturating 6-bit quality sums; an index
    is a position in the ascending set"""
    _free = "bbk_kmerstats_free"

    def __len__(self):
        return int(self._L.bbk_kmerstats_size(self._h))

    def push(self, reads, quals):
        """every k-mer position of every read is an occurrence, of the k-mer and of its reverse complement"""
        _check(self._L.bbk_kmerstats_push(self._h, reads._h, quals._h))

    def finish(self):
        _check(self._L.bbk_kmerstats_finish(self._h))

    def export(self):
        """(count np.uint32[n], total_qual np.float32[n], qual_words np.uint64[n, ceil(6k / 64)])"""
        n, nw = len(self), (6 * self.k + 63) // 64
        cnt = np.zeros(n, dtype=np.uint32)
        tq = np.zeros(n, dtype=np.float32)
        qw = np.zeros((n, nw), dtype=np.uint64)
        _check(self._L.bbk_kmerstats_export(self.ctx._h, self._h, _ptr(cnt), _ptr(tq), _ptr(qw)))
        return cnt, tq, qw

    def qual_matrix(self):
        """np.uint8[n, k]: the quality sums unpacked (sum i of a k-mer is bits [6i, 6i + 6) of its words)"""
        qw = self.export()[2]
        bits = np.unpackbits(np.ascontiguousarray(qw).view(np.uint8), axis=1, bitorder="little")[:, :6 * self.k]
        return (bits.reshape(len(self), self.k, 6) << np.arange(6, dtype=np.uint8)).sum(axis=2).astype(np.uint8)

    def write(self, path):
        """one binary_write(KMerStat) record per k-mer: u32 count << 1, float total_qual, the QualBitSet words"""
        _check(self._L.bbk_kmerstats_write(self.ctx._h, self._h, str(path).encode()))


class HamClusters(_Handle):
    """clusters of k-mers at Hamming distance 1 (the reference's kmers.hamming); an index is a position in the
    ascending set, a label the smallest index of a cluster"""
    _free = "bbk_hamclusters_free"

    def __len__(self):
        return int(self._L.bbk_hamclusters_count(self._h))

    @property
    def size(self):
        return int(self._L.bbk_hamclusters_size(self._h))

    @property
    def replayed(self):
        """k-mers of components of lock_size members or more, which went through the host replay"""
        return int(self._L.bbk_hamclusters_replayed(self._h))

    def labels(self):
        """np.uint64 [size]: the label of every k-mer"""
        a = np.zeros(self.size, dtype=np.uint64)
        _check(self._L.bbk_hamclusters_export(self.ctx._h, self._h, _ptr(a), None, None))
        return a

    def members(self):
        """np.uint64 [size]: the indices cluster by cluster (by ascending label), ascending inside a cluster"""
        a = np.zeros(self.size, dtype=np.uint64)
        _check(self._L.bbk_hamclusters_export(self.ctx._h, self._h, None, _ptr(a), None))
        return a

    def sizes(self):
        """np.uint64 [len]: members of every cluster, in the order of members()"""
        a = np.zeros(len(self), dtype=np.uint64)
        _check(self._L.bbk_hamclusters_export(self.ctx._h, self._h, None, None, _ptr(a)))
        return a

    def write(self, path):
        """<path> (member indices, u64) and <path>.idx (cluster sizes, u64): ConcurrentDSU::extract_to_file"""
        _check(self._L.bbk_hamclusters_write(self.ctx._h, self._h, str(path).encode()))

    def subcluster(self, kmer_stats, singleton_threshold=0.995, nonsingleton_threshold=0.9, correct_threshold=0.98,
                   correct_use_threshold=True):
        """KMerClustering::process over these clusters and the finished statistics of the same set: SubClusters.  The
        defaults are the thresholds of configs/hammer/config.info."""
        p = SubclusterParams(singleton_threshold, nonsingleton_threshold, correct_threshold, int(bool(correct_use_threshold)))
        h = C.c_void_p()
        _check(self._L.bbk_hamclusters_subcluster(self.ctx._h, kmer_stats._set._h, self._h, kmer_stats._h, C.byref(p),
                                                  C.byref(h)))
        sc = SubClusters(self.ctx, h)
        sc._n, sc._clusters, sc._stats_of = self.size, len(self), kmer_stats
        return sc


class SubclusterParams(C.Structure):
    """bbk_subcluster_params of include/bbk.h"""
    _fields_ = [("singleton_threshold", C.c_double), ("nonsingleton_threshold", C.c_double),
                ("correct_threshold", C.c_double), ("correct_use_threshold", C.c_int)]


class SubClusters(_Handle):
    """BayesHammer's subclusters of the Hamming clusters, the good bit of every k-mer and the new k-mers"""
    _free = "bbk_subclusters_free"
    STATS = ("gsingl", "tsingl", "tcsingl", "gcsingl", "tcls", "gcls", "tkmers", "tncls", "newkmers")

    def __len__(self):
        return int(self._L.bbk_subclusters_count(self._h))

    @property
    def size(self):
        """entries of all lists together"""
        return int(self._L.bbk_subclusters_size(self._h))

    @property
    def new_kmers(self):
        return int(self._L.bbk_subclusters_new_kmers(self._h))

    @property
    def host_kmers(self):
        """k-mers of the clusters that went through the host path (more than 256 members, or BBK_SUBCLUSTER_HOST=1)"""
        return int(self._L.bbk_subclusters_host_kmers(self._h))

    def export(self):
        """dict: good u8[n + new], members u64[size] (the center first, a new k-mer as n + j), sizes u64[len],
        per_cluster u64[clusters], new_keys u64[new], bic f64[clusters] (-inf for a singleton), errs u64[16]
        (4 * center base + k-mer base), stats u64[9] (SubClusters.STATS)"""
        r = dict(good=np.zeros(self._n + self.new_kmers, dtype=np.uint8), members=np.zeros(self.size, dtype=np.uint64),
                 sizes=np.zeros(len(self), dtype=np.uint64), per_cluster=np.zeros(self._clusters, dtype=np.uint64),
                 new_keys=np.zeros(self.new_kmers, dtype=np.uint64), bic=np.zeros(self._clusters, dtype=np.float64),
                 errs=np.zeros(16, dtype=np.uint64), stats=np.zeros(9, dtype=np.uint64))
        _check(self._L.bbk_subclusters_export(self.ctx._h, self._h, *[_ptr(r[x]) for x in (
            "good", "members", "sizes", "per_cluster", "new_keys", "bic", "errs", "stats")]))
        return r

    @property
    def stats(self):
        """the counters of the reference's "Subclustering statistics" lines, by name"""
        a = np.zeros(9, dtype=np.uint64)
        _check(self._L.bbk_subclusters_export(self.ctx._h, self._h, None, None, None, None, None, None, None, _ptr(a)))
        return dict(zip(self.STATS, (int(x) for x in a)))

    def write(self, prefix):
        """<prefix>.kmstat (good bits set, new k-mers appended), .subclusters, .subclusters.idx, .newkmers"""
        _check(self._L.bbk_subclusters_write(self.ctx._h, self._h, self._stats_of._h, str(prefix).encode()))

    def expander(self):
        """Expander over the set these subclusters were made for, from their good bits"""
        kmer_set = self._stats_of._set
        h = C.c_void_p()
        _check(self._L.bbk_expander_from_subclusters(self.ctx._h, kmer_set._h, self._h, C.byref(h)))
        e = Expander(self.ctx, h)
        e._set = kmer_set
        return e


class Expander(_Handle):
    """BayesHammer's expansion of the solid k-mers in snapshot rounds (bbk_expander_*): a read that good k-mers cover end to
    end makes all of its k-mers good.  The reads are the candidates of host/hammer_reads.hpp, one trimmed read each."""
    _free = "bbk_expander_free"

    def begin_round(self):
        _check(self._L.bbk_expander_round_begin(self._h))

    def push(self, reads, status=False):
        """the reads of a round, in any order and batching; status=True: np.uint8[len(reads)], 0 not solid, 1 solid,
        2 every start already good (and the call waits for the device).  Keep the reads until end_round."""
        st = np.zeros(len(reads), dtype=np.uint8) if status else None
        _check(self._L.bbk_expander_push(self._h, reads._h, _ptr(st)))
        return st

    def end_round(self):
        """the k-mers the round made good"""
        c = C.c_uint64()
        _check(self._L.bbk_expander_round_end(self._h, C.byref(c)))
        return int(c.value)

    def run(self, reads, max_rounds=25, min_changed=10):
        """rounds over resident reads until one adds fewer than min_changed k-mers or max_rounds have run (the
        reference's expand_max_iterations 25 and 10): the list of the rounds' counts"""
        n = C.c_uint(0)
        counts = np.zeros(max(int(max_rounds), 1), dtype=np.uint64)
        _check(self._L.bbk_expander_run(self._h, reads._h, max_rounds, min_changed, C.byref(n), _ptr(counts)))
        return [int(x) for x in counts[:n.value]]

    @property
    def good(self):
        """good k-mers now"""
        return int(self._L.bbk_expander_good(self._h))

    def export(self):
        """np.uint8[n]: the good bit of every k-mer of the set"""
        a = np.zeros(len(self._set), dtype=np.uint8)
        _check(self._L.bbk_expander_export(self.ctx._h, self._h, _ptr(a)))
        return a

    def store(self, subclusters):
        """the bits back into the subclusters (their first n k-mers): SubClusters.export() / write() then carry them"""
        _check(self._L.bbk_expander_store(self._h, subclusters._h))

    def corrector(self):
        """Corrector over the expander's set from its bits as they are now (copied)"""
        h = C.c_void_p()
        _check(self._L.bbk_corrector_from_expander(self.ctx._h, self._set._h, self._h, C.byref(h)))
        c = Corrector(self.ctx, h)
        c._set = self._set
        return c


class Corrector(_Handle):
    """BayesHammer's ReadCorrector (bbk_corrector_*): trimmed reads corrected outwards from their longest solid island,
    equal to the reference base for base"""
    _free = "bbk_corrector_free"
    STATS = ("changed_reads", "changed_nucleotides", "uncorrected_nucleotides", "total_nucleotides", "host_searches")

    def limits(self):
        """(heap_cap, pop_cap) of a search on the device; a search beyond them runs through the host rule"""
        a, b = C.c_uint(), C.c_uint()
        self._L.bbk_corrector_limits(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def correct(self, reads):
        """reads: [(seq, quals)], trimmed, quals with the offset subtracted -> (corrected sequences, result np.uint8[n],
        where np.uint8[n]: 0 no search, 1 device, 2 host rule)"""
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s, _ in reads]
        off = np.zeros(len(reads) + 1, dtype=np.uint64)
        if reads:
            off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
        bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
        qual = np.zeros(len(bases), dtype=np.uint8)
        for i, (_, q) in enumerate(reads):
            if len(q) != len(seqs[i]):
                raise ValueError("read %d: %d bases, %d qualities" % (i, len(seqs[i]), len(q)))
            qual[int(off[i]):int(off[i + 1])] = np.asarray(q, dtype=np.int64).clip(0, 255)
        out, res, where = self.correct_arrays(bases, qual, off)
        raw = out.tobytes()
        return [raw[int(off[i]):int(off[i + 1])].decode() for i in range(len(reads))], res, where

    def correct_arrays(self, bases, qual, offsets):
        """the same over the arrays of the C call: bases and qual np.uint8 back to back, offsets np.uint64[n + 1] ->
        (corrected bases np.uint8, result np.uint8[n], where np.uint8[n])"""
        n = len(offsets) - 1
        out = np.zeros(len(bases), dtype=np.uint8)
        res = np.zeros(n, dtype=np.uint8)
        where = np.zeros(n, dtype=np.uint8)
        _check(self._L.bbk_corrector_correct(self._h, _ptr(bases), _ptr(qual), _ptr(offsets), n, _ptr(out), _ptr(res),
                                             _ptr(where)))
        return out, res, where

    def correct_prepared(self, hr):
        """the same over the trimmed reads of a HammerReads, from its resident bytes and corrector table ->
        (corrected bases np.uint8, offsets np.uint64[n + 1], result np.uint8[n], where np.uint8[n])"""
        n = len(hr)
        out = np.zeros(hr.bases, dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        res = np.zeros(n, dtype=np.uint8)
        where = np.zeros(n, dtype=np.uint8)
        _check(self._L.bbk_corrector_correct_prepared(self._h, hr._h, _ptr(out), _ptr(off), _ptr(res), _ptr(where)))
        return out[:int(off[n])], off, res, where

    def correct_resident(self, hr):
        """correct_prepared with the outcome kept on the device -> Corrected (it borrows hr)"""
        h = C.c_void_p()
        _check(self._L.bbk_corrector_correct_resident(self._h, hr._h, C.byref(h)))
        cr = Corrected(self.ctx, h)
        cr._hr, cr._corrector = hr, self
        return cr

    @property
    def stats(self):
        """the counters summed over the calls so far, by name (Corrector.STATS)"""
        a = np.zeros(5, dtype=np.uint64)
        _check(self._L.bbk_corrector_stats(self._h, _ptr(a)))
        return dict(zip(self.STATS, (int(x) for x in a)))


def _name_blob(names, n, what):
    """names: n str / bytes -> (blob np.uint8, offsets np.uint64[n + 1])"""
    raw = [x.encode() if isinstance(x, str) else bytes(x) for x in names]
    if len(raw) != n:
        raise ValueError("%d %s names for %d records" % (len(raw), what, n))
    off = np.zeros(n + 1, dtype=np.uint64)
    if raw:
        off[1:] = np.cumsum([len(x) for x in raw], dtype=np.uint64)
    return np.frombuffer(b"".join(raw), dtype=np.uint8), off


class Corrected(_Handle):
    """What the corrector made of a HammerReads, resident (bbk_corrected_*): the corrected trimmed reads, the result
    flags, where the searches ran, and per read the changed positions and the kind of its BH: tag"""
    _free = "bbk_corrected_free"
    TAGS = ("", " BH:ok", " BH:failed", " BH:changed:")

    def __len__(self):
        return int(self._L.bbk_corrected_size(self._h))

    def export(self, outcome=False):
        """(corrected bases np.uint8, offsets np.uint64[n + 1], result np.uint8[n], where np.uint8[n]) as
        Corrector.correct_prepared gives them; with outcome also (changed np.uint32[n], tag np.uint8[n])"""
        n = len(self)
        out = np.zeros(self._hr.bases, dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        res = np.zeros(n, dtype=np.uint8)
        where = np.zeros(n, dtype=np.uint8)
        changed = np.zeros(n, dtype=np.uint32)
        tag = np.zeros(n, dtype=np.uint8)
        _check(self._L.bbk_corrected_export(self.ctx._h, self._h, _ptr(out), _ptr(off), _ptr(res), _ptr(where),
                                            _ptr(changed) if outcome else None, _ptr(tag) if outcome else None))
        r = (out[:int(off[n])], off, res, where)
        return r + (changed, tag) if outcome else r

    def print(self, names, qvoffset=33, tags=False, mate=None, mate_names=None):
        """Read::print of every record, named names[i], routed like CorrectReadFile -> FastqText with streams (good, bad);
        with mate (the Corrected of the right reads) and mate_names like CorrectPairedReadFiles -> streams (cor-left,
        cor-right, unpaired, bad-left, bad-right).  tags: the BH: tags of correct_stats 1."""
        bl, ol = _name_blob(names, len(self), "left" if mate is not None else "read")
        br, orr = _name_blob(mate_names or [], len(mate), "right") if mate is not None else (None, None)
        h = C.c_void_p()
        _check(self._L.bbk_corrected_print(self._h, mate._h if mate is not None else None, _ptr(bl), _ptr(ol),
                                           _ptr(br) if mate is not None else None, _ptr(orr) if mate is not None else None,
                                           int(qvoffset), 1 if tags else 0, C.byref(h)))
        return FastqText(self.ctx, h)


    def print_resident(self, mate=None, qvoffset=33, tags=False):
        """print with the names the batches hold themselves (HammerReads made by FastqInput.hammer_reads)"""
        h = C.c_void_p()
        _check(self._L.bbk_corrected_print_resident(self._h, mate._h if mate is not None else None, int(qvoffset),
                                                    1 if tags else 0, C.byref(h)))
        return FastqText(self.ctx, h)


class FastqText(_Handle):
    """FASTQ text on the device, one stream per output file (bbk_fastq_text_*)"""
    _free = "bbk_fastq_text_free"

    @property
    def sizes(self):
        return [int(self._L.bbk_fastq_text_size(self._h, i)) for i in range(int(self._L.bbk_fastq_text_streams(self._h)))]

    def stream(self, i):
        """the bytes of stream i"""
        buf = np.zeros(int(self._L.bbk_fastq_text_size(self._h, i)), dtype=np.uint8)
        _check(self._L.bbk_fastq_text_export(self.ctx._h, self._h, i, _ptr(buf)))
        return buf.tobytes()

    def write(self, i, path, append=False):
        _check(self._L.bbk_fastq_text_write(self.ctx._h, self._h, i, os.fsencode(path), 1 if append else 0))


class Counter:
    """bbk_counter: push batches of reads, finish() returns the KMerSet (and releases the counter)."""

    def __init__(self, ctx, k, flags):
        self.ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        _check(self._L.bbk_count_begin(ctx._h, k, flags, C.byref(h)))
        self._h = h

    def push(self, reads):
        _check(self._L.bbk_count_push_reads(self._h, reads._h))

    def push_ascii(self, reads):
        bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
        offs = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        _check(self._L.bbk_count_push_ascii(self._h, b"".join(bs), _ptr(offs), len(bs)))

    @property
    def instances(self):
        return int(self._L.bbk_count_pushed_instances(self._h))

    def finish(self, min_count=None):
        """the KMerSet; with min_count only the records whose multiplicity reaches it (bbk_count_finish_min_count: the
        counter needs WITH_COUNTS), and the set's n_dropped tells how many records of the unfiltered set are absent"""
        h = C.c_void_p()
        c, self._h = self._h, None
        if min_count is None:
            _check(self._L.bbk_count_finish(c, C.byref(h)))
            return KMerSet(self.ctx, h)
        dropped = C.c_uint64(0)
        _check(self._L.bbk_count_finish_min_count(c, int(min_count), C.byref(h), C.byref(dropped)))
        s = KMerSet(self.ctx, h)
        s.n_dropped = int(dropped.value)
        return s

    def abort(self):
        if getattr(self, "_h", None):
            self._L.bbk_count_abort(self._h)
            self._h = None

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


class ExtBuilder:
    """bbk_extbuilder: push batches of reads, finish() returns the ExtIndex."""

    def __init__(self, ctx, k):
        self.ctx, self._L = ctx, ctx._L
        h = C.c_void_p()
        _check(self._L.bbk_extindex_begin(ctx._h, k, C.byref(h)))
        self._h = h

    def push(self, reads):
        _check(self._L.bbk_extindex_push_reads(self._h, reads._h))

    def finish(self):
        h = C.c_void_p()
        b, self._h = self._h, None
        _check(self._L.bbk_extindex_finish(b, C.byref(h)))
        return ExtIndex(self.ctx, h)

    def finish_with_set(self, flags=BOTH_STRANDS):
        """(KMerSet of both strands, ExtIndex) from the one accumulation (bbk_extindex_finish_with_set)"""
        hs, hx = C.c_void_p(), C.c_void_p()
        b, self._h = self._h, None
        _check(self._L.bbk_extindex_finish_with_set(b, flags, C.byref(hs), C.byref(hx)))
        return KMerSet(self.ctx, hs), ExtIndex(self.ctx, hx)

    def abort(self):
        if getattr(self, "_h", None):
            self._L.bbk_extindex_abort(self._h)
            self._h = None

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


class ExtIndex(_Handle):
    _free = "bbk_extindex_free"

    def __len__(self):
        return int(self._L.bbk_extindex_size(self._h))

    @property
    def k(self):
        return int(self._L.bbk_extindex_k(self._h))

    def clip_tips(self, length_bound):
        """EarlyTipClipperProcessor(index, length_bound).ClipTips() in place; returns (isolated k-mers, removed links)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.bbk_extindex_clip_tips(self.ctx._h, self._h, length_bound, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def remove_at_edges(self, ratio=0.8):
        """EarlyLowComplexityClipperProcessor::RemoveATEdges in place; returns (collected edges, removed links)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.bbk_extindex_remove_at_edges(self.ctx._h, self._h, ratio, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def remove_at_tips(self, ratio=0.8, min_len=10, max_len=200):
        """EarlyLowComplexityClipperProcessor::RemoveATTips in place; returns (isolated k-mers, clipped links)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.bbk_extindex_remove_at_tips(self.ctx._h, self._h, ratio, min_len, max_len, C.byref(a),
                                                   C.byref(b)))
        return int(a.value), int(b.value)

    def export_to_u32(self, dst_keys, dst_masks_u32):
        """keys + masks widened to u32 (the payload layout of the owner exchange) into preallocated tensors/arrays"""
        _check(self._L.bbk_extindex_export_u32(self.ctx._h, self._h, _ptr(dst_keys), _ptr(dst_masks_u32)))

    def export(self):
        n, nw = len(self), words(self.k)
        keys = np.zeros((n, nw), dtype=np.uint64)
        masks = np.zeros(n, dtype=np.uint8)
        _check(self._L.bbk_extindex_export(self.ctx._h, self._h, _ptr(keys), _ptr(masks)))
        return keys, masks


class Unitigs(_Handle):
    _free = "bbk_unitigs_free"

    def __len__(self):
        return int(self._L.bbk_unitigs_count(self._h))

    @property
    def n_loops(self):
        return int(self._L.bbk_unitigs_loops(self._h))

    @property
    def n_vertices(self):
        return int(self._L.bbk_unitigs_vertices(self._h))

    @property
    def n_links(self):
        return int(self._L.bbk_unitigs_links(self._h))

    @property
    def total_bases(self):
        return int(self._L.bbk_unitigs_total_bases(self._h))

    def sequences(self):
        n = len(self)
        offs = np.zeros(n + 1, dtype=np.uint64)
        buf = np.zeros(self.total_bases + 1, dtype=np.uint8)
        _check(self._L.bbk_unitigs_export(self.ctx._h, self._h, _ptr(buf), _ptr(offs)))
        b = buf.tobytes()
        return [b[int(offs[i]):int(offs[i + 1])].decode() for i in range(n)]

    def to_reads(self):
        """the condensed edges as a device-resident read set (contigs of this K as input of the next,
        stages/construction.cpp:117-119,228-236)"""
        h = C.c_void_p()
        _check(self._L.bbk_unitigs_to_reads(self.ctx._h, self._h, C.byref(h)))
        return Reads(self.ctx, h)

    def add_coverage(self, reads):
        """gbuilder -c: KC / DP of every condensed edge from the reads."""
        _check(self._L.bbk_unitigs_add_coverage(self.ctx._h, self._h, reads._h))

    def add_coverage_counts(self, kp1_counts):
        """same from an already counted ascending canonical (k+1)-mer KMerSet with counts"""
        _check(self._L.bbk_unitigs_add_coverage_counts(self.ctx._h, self._h, kp1_counts._h))

    def kc(self):
        a = np.zeros(len(self), dtype=np.uint64)
        _check(self._L.bbk_unitigs_export_kc(self.ctx._h, self._h, _ptr(a)))
        return a

    def links(self):
        a = np.zeros((self.n_links, 4), dtype=np.uint32)
        _check(self._L.bbk_unitigs_export_links(self.ctx._h, self._h, _ptr(a)))
        return a

    def write_gfa(self, path):
        _check(self._L.bbk_unitigs_write_gfa(self.ctx._h, self._h, path.encode()))

    def write_fastg(self, path):
        _check(self._L.bbk_unitigs_write_fastg(self.ctx._h, self._h, path.encode()))

    def write_fasta(self, path):
        _check(self._L.bbk_unitigs_write_fasta(self.ctx._h, self._h, path.encode()))

    def write_spades(self, basename):
        """<basename>.grseq + <basename>.cvr (the SPAdes binary graph of gbuilder --spades)"""
        _check(self._L.bbk_unitigs_write_spades(self.ctx._h, self._h, basename.encode()))


class EdgeIndex(_Handle):
    """every (k+1)-mer of a graph's segments with its place (unitig-coverage's EdgeIndex)"""
    _free = "bbk_edgeindex_free"

    @property
    def segments(self):
        return int(self._L.bbk_edgeindex_segments(self._h))

    def __len__(self):
        return int(self._L.bbk_edgeindex_size(self._h))

    def profiles(self, n_samples):
        h = C.c_void_p()
        _check(self._L.bbk_profiles_begin(self.ctx._h, self._h, n_samples, C.byref(h)))
        return Profiles(self, h, n_samples)

    def map_paths(self, reads):
        """MapSequence of every read as it stands (spades-gmapper's mapper): (offsets, ranges), offsets np.uint64
        [reads + 1], ranges a PATH_RANGE array in read order (edge = 2 * segment + 1 on the reverse strand)"""
        h = C.c_void_p()
        _check(self._L.bbk_edgeindex_map_paths(self.ctx._h, self._h, reads._h, C.byref(h)))
        try:
            off = np.zeros(int(self._L.bbk_paths_reads(h)) + 1, dtype=np.uint64)
            rec = np.zeros(int(self._L.bbk_paths_ranges(h)), dtype=PATH_RANGE)
            _check(self._L.bbk_paths_export(self.ctx._h, h, _ptr(off), _ptr(rec)))
        finally:
            self._L.bbk_paths_free(h)
        return off, rec

    def segment_lengths(self):
        """(lengths np.uint64 in (k+1)-mers, self-conjugate np.uint8) of the segments"""
        n = self.segments
        a, c = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        _check(self._L.bbk_edgeindex_export_segments(self._h, _ptr(a), _ptr(c)))
        return a, c

    def pairinfo(self, min_edge_length=0):
        """paired-read info over this index (PairInfoCount for a paired-end library): a PairInfo"""
        h = C.c_void_p()
        _check(self._L.bbk_pairinfo_begin(self.ctx._h, self._h, min_edge_length, C.byref(h)))
        return PairInfo(self, h)

    def pairinfo_from_points(self, e1, e2, gap, weight):
        """a filled PairInfo from host points (bbk_pairinfo_import): canonicalised, sorted, equal points added"""
        e1, e2 = np.ascontiguousarray(e1, dtype=np.uint64), np.ascontiguousarray(e2, dtype=np.uint64)
        gap, weight = np.ascontiguousarray(gap, dtype=np.int32), np.ascontiguousarray(weight, dtype=np.uint64)
        if not (e1.shape == e2.shape == gap.shape == weight.shape and e1.ndim == 1):
            raise ValueError("e1, e2, gap and weight must be one-dimensional and equally long")
        h = C.c_void_p()
        _check(self._L.bbk_pairinfo_import(self.ctx._h, self._h, len(e1), _ptr(e1), _ptr(e2), _ptr(gap), _ptr(weight),
                                           C.byref(h)))
        return PairInfo(self, h)

    def graph(self):
        """(names, sequences, links [(a, '+'|'-', b, '+'|'-')], kc np.uint32) as the index holds the graph"""
        ns, nl = self.segments, int(self._L.bbk_edgeindex_links(self._h))
        bases = C.create_string_buffer(int(self._L.bbk_edgeindex_total_bases(self._h)) + 1)
        off = np.zeros(ns + 1, dtype=np.uint64)
        lk = np.zeros(4 * nl + 1, dtype=np.uint32)
        kc = np.zeros(ns, dtype=np.uint32)
        _check(self._L.bbk_edgeindex_export_graph(self._h, bases, _ptr(off), _ptr(lk), _ptr(kc)))
        raw = bases.raw
        seqs = [raw[int(off[i]):int(off[i + 1])].decode() for i in range(ns)]
        names = [self._L.bbk_edgeindex_name(self._h, i).decode() for i in range(ns)]
        sign = lambda x: "+" if x else "-"  # noqa: E731
        links = [(int(lk[4 * j]), sign(lk[4 * j + 1]), int(lk[4 * j + 2]), sign(lk[4 * j + 3])) for j in range(nl)]
        return names, seqs, links, kc


class PairInfo(_Handle):
    """insert sizes, edge pairs and the raw paired index of one paired-end library: push_estimate the batches, estimate(),
    fill_begin(), push_fill the same batches, fill_finish(), then points() or write()"""
    _free = "bbk_pairinfo_free"

    def __init__(self, index, h):
        super().__init__(index.ctx, h)
        self.index = index  # the index must outlive the handle

    @staticmethod
    def _cut(cut, n):
        if cut is None:
            return None
        cut = np.ascontiguousarray(cut, dtype=np.uint32)
        if cut.shape != (n, 4):
            raise ValueError("cut must hold (left1, right1, left2, right2) for each of the %d pairs" % n)
        return cut

    def push_estimate(self, first, second, orientation=ORIENT_FR, cut=None):
        cut = self._cut(cut, len(first))
        _check(self._L.bbk_pairinfo_push_estimate(self._h, first._h, second._h, orientation, _ptr(cut) if cut is not None else None))

    def estimate(self):
        """the statistics of CollectLibInformation as a dict (percentiles: 19 values, 5 % ... 95 %)"""
        st = PairInfoStats()
        _check(self._L.bbk_pairinfo_estimate(self._h, C.byref(st)))
        d = {f: getattr(st, f) for f, _ in PairInfoStats._fields_ if f != "percentiles"}
        d["percentiles"] = [int(x) for x in st.percentiles]
        d["ok"] = bool(st.ok)
        return d

    def hist(self):
        """(insert sizes np.int32, counts np.uint64), ascending"""
        n = int(self._L.bbk_pairinfo_hist_size(self._h))
        a, c = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64)
        _check(self._L.bbk_pairinfo_hist_export(self._h, _ptr(a), _ptr(c)))
        return a, c

    def fill_begin(self, insert_size, round_distance=0, filter_threshold=0):
        _check(self._L.bbk_pairinfo_fill_begin(self._h, int(insert_size), round_distance, filter_threshold))

    def push_fill(self, first, second, orientation=ORIENT_FR, cut=None):
        cut = self._cut(cut, len(first))
        _check(self._L.bbk_pairinfo_push_fill(self._h, first._h, second._h, orientation, _ptr(cut) if cut is not None else None))

    def fill_finish(self):
        _check(self._L.bbk_pairinfo_fill_finish(self._h))

    def points(self):
        """(e1 np.uint64, e2 np.uint64, gap np.int32, weight np.uint64) of the index, ascending"""
        n = int(self._L.bbk_pairinfo_points(self._h))
        e1, e2 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        gap, w = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64)
        _check(self._L.bbk_pairinfo_export(self._h, _ptr(e1), _ptr(e2), _ptr(gap), _ptr(w)))
        return e1, e2, gap, w

    def write(self, path):
        """the index in the layout of PairedBuffer::BinWrite (.prd), ids = edge + 1"""
        _check(self._L.bbk_pairinfo_write(self._h, str(path).encode()))

    def cluster(self, insert_size, read_length, delta, linkage_distance=0, max_distance=0, filter_threshold=2.0):
        """DistanceEstimator and the weight filter over the points (bbk_pairinfo_cluster): a Clustered.  The index must
        keep its graph (edgeindex_from_gfa(..., keep_graph=True))"""
        prm = ClusterParams(int(insert_size), int(read_length), int(delta), int(linkage_distance), int(max_distance),
                            float(filter_threshold))
        h = C.c_void_p()
        _check(self._L.bbk_pairinfo_cluster(self._h, C.byref(prm), C.byref(h)))
        return Clustered(self, h)


class Clustered(_Handle):
    """the clustered paired index of one library: export() or write()"""
    _free = "bbk_clustered_free"

    def __init__(self, pairinfo, h):
        super().__init__(pairinfo.ctx, h)
        self.pairinfo = pairinfo  # the raw index (and with it the edge index) must outlive the handle

    def __len__(self):
        return int(self._L.bbk_clustered_points(self._h))

    @property
    def pairs(self):
        """edge pairs of the raw index"""
        return int(self._L.bbk_clustered_pairs(self._h))

    @property
    def host_pairs(self):
        """of these, the pairs the host searched"""
        return int(self._L.bbk_clustered_host_pairs(self._h))

    def export(self):
        """(e1 np.uint64, e2 np.uint64, centre np.float32, half-span np.float32 (0, as the reference leaves it), weight in half-units np.uint64),
        ascending (e1, e2, centre)"""
        n = len(self)
        e1, e2, w = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        c, v = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        _check(self._L.bbk_clustered_export(self._h, _ptr(e1), _ptr(e2), _ptr(c), _ptr(v), _ptr(w)))
        return e1, e2, c, v, w

    def write(self, path):
        """the index in the layout of PairedBuffer::BinWrite (.clustered.prd), ids = edge + 1"""
        _check(self._L.bbk_clustered_write(self._h, str(path).encode()))


class Profiles(_Handle):
    """per-sample edge abundance profiles (EdgeProfileStorage): push the reads of each sample, then raw() or write()"""
    _free = "bbk_profiles_free"

    def __init__(self, index, h, n_samples):
        super().__init__(index.ctx, h)
        self.index, self.samples = index, n_samples  # the index must outlive the profiles

    def push(self, sample, reads):
        _check(self._L.bbk_profiles_push_reads(self._h, sample, reads._h))

    def raw(self):
        """np.uint64 [segments, samples]: summed mapped-range sizes of every segment's edge and its conjugate"""
        a = np.zeros((self.index.segments, self.samples), dtype=np.uint64)
        _check(self._L.bbk_profiles_export_raw(self.ctx._h, self._h, _ptr(a)))
        return a

    def write(self, path):
        """the unitig-coverage output file (EdgeProfileStorage::Save)"""
        _check(self._L.bbk_profiles_write(self.ctx._h, self._h, path.encode()))


class KmerProfile(_Handle):
    """kept k-mers x samples table of u16 multiplicities (the reference's .bpr with its k-mer index)"""
    _free = "bbk_kmerprofile_free"

    def __len__(self):
        return int(self._L.bbk_kmerprofile_size(self._h))

    @property
    def k(self):
        return int(self._L.bbk_kmerprofile_k(self._h))

    @property
    def samples(self):
        return int(self._L.bbk_kmerprofile_samples(self._h))

    def keys(self):
        """np.uint64 [size, words]: the kept canonical k-mers, ascending"""
        a = np.zeros((len(self), words(self.k)), dtype=np.uint64)
        _check(self._L.bbk_kmerprofile_export(self.ctx._h, self._h, _ptr(a), None))
        return a

    def rows(self):
        """np.uint16 [size, samples]: the multiplicity of every kept k-mer in every sample (0: absent)"""
        a = np.zeros((len(self), self.samples), dtype=np.uint16)
        _check(self._L.bbk_kmerprofile_export(self.ctx._h, self._h, None, _ptr(a)))
        return a

    def write(self, prefix):
        """<prefix>.bpr and <prefix>.kmers"""
        _check(self._L.bbk_kmerprofile_write(self.ctx._h, self._h, str(prefix).encode()))

    def abundance(self, reads, first_piece=None):
        """(n, positions, sum, sumsq): per contig the k-mers found and the k-mer positions, per (contig, sample) the sum
        and the sum of squares of the winsorised column; integers only (see bbk_kmerprofile_abundance).  Every read is
        a contig, or with first_piece (contigs + 1 entries) contig c is the reads [first_piece[c], first_piece[c + 1]):
        its maximal ACGT stretches."""
        if first_piece is None:
            nc = len(reads)
        else:
            first_piece = np.ascontiguousarray(first_piece, dtype=np.uint64)
            nc = len(first_piece) - 1
        n = np.zeros(nc, dtype=np.uint64)
        pos = np.zeros(nc, dtype=np.uint64)
        sm = np.zeros((nc, self.samples), dtype=np.uint64)
        sq = np.zeros((nc, self.samples), dtype=np.uint64)
        if first_piece is None:
            _check(self._L.bbk_kmerprofile_abundance(self.ctx._h, self._h, reads._h, _ptr(n), _ptr(pos), _ptr(sm),
                                                     _ptr(sq)))
        else:
            _check(self._L.bbk_kmerprofile_abundance_pieces(self.ctx._h, self._h, reads._h, _ptr(first_piece), nc, _ptr(n),
                                                            _ptr(pos), _ptr(sm), _ptr(sq)))
        return n, pos, sm, sq
