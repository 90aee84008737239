"""ctypes binding of ``libfastani_hip.so`` (the C ABI declared in ``include/fastani_hip.h``).

The product binding is the Cython module ``pyfastani_amd._fastani``; this table of every exported symbol serves the
tests (symbol / layout checks), the debug and timing entry points used by ``bench.py`` and ``scripts/``, and as the
ctypes stub shown in INTEGRATION.md.  The library is the only compute backend: if it is missing, importing this module
raises ``ImportError`` with build instructions -- there is no CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfastani_hip.so")

FA_OK, FA_ERR_INVALID, FA_ERR_NO_DEVICE, FA_ERR_NOMEM, FA_ERR_UNSUPPORTED, FA_ERR_INTERNAL, FA_ERR_IO, FA_ERR_BUFFER = range(8)


class Params(C.Structure):
    # skch::Parameters, include/fastani/map/map_parameters.pxd:9-24 of the reference
    _fields_ = [
        ("kmer_size", C.c_int32),
        ("window_size", C.c_int32),
        ("fragment_length", C.c_int32),
        ("alphabet_size", C.c_int32),
        ("min_fraction", C.c_float),
        ("percentage_identity", C.c_float),
        ("p_value", C.c_double),
        ("reference_size", C.c_uint64),
    ]


class RulesStruct(C.Structure):
    # fa_rules: the open readings of the arithmetic a mapper follows (pyfastani_amd.Rules is the Python face of it)
    _fields_ = [
        ("l2_confidence", C.c_float),
        ("slide_end", C.c_int32),
        ("cgi_ties", C.c_int32),
    ]


class CgiRow(C.Structure):
    # cgi::CGI_Results, include/fastani/cgi/cgid_types.pxd:19-27
    _fields_ = [
        ("query_id", C.c_int32),
        ("ref_genome_id", C.c_int32),
        ("count_seq", C.c_int32),
        ("total_query_fragments", C.c_int32),
        ("identity", C.c_float),
    ]


class Mapping(C.Structure):
    _fields_ = [
        ("query_seq_id", C.c_int32),
        ("ref_seq_id", C.c_int32),
        ("ref_start_pos", C.c_int32),
        ("sketch_size", C.c_int32),
        ("conserved", C.c_int32),
        ("query_id", C.c_int32),
    ]


class HitMapping(C.Structure):
    # one mapping computeCGI kept (fa_hit_mapping)
    _fields_ = [
        ("query_id", C.c_int32),
        ("query_seq_id", C.c_int32),
        ("ref_genome_id", C.c_int32),
        ("ref_seq_id", C.c_int32),
        ("ref_start_pos", C.c_int32),
        ("sketch_size", C.c_int32),
        ("conserved", C.c_int32),
        ("identity", C.c_float),
    ]


class Pair(C.Structure):
    # fa_pair: one unordered genome pair of an all-vs-all table (pyfastani_amd._batch.PAIR_DTYPE is the numpy face of it)
    _fields_ = [
        ("a", C.c_int32),
        ("b", C.c_int32),
        ("identity_ab", C.c_float),
        ("identity_ba", C.c_float),
        ("identity", C.c_double),
    ]


class Merge(C.Structure):
    # fa_merge: one merge of an average-linkage dendrogram (pyfastani_amd._batch.MERGE_DTYPE is the numpy face of it)
    _fields_ = [
        ("lo", C.c_int32),
        ("hi", C.c_int32),
        ("size_lo", C.c_int32),
        ("size_hi", C.c_int32),
        ("s", C.c_int64),
        ("present", C.c_int64),
    ]


class TableParams(C.Structure):
    # fa_table_params: the filter and the cut-off of fa_table_pairs / fa_table_clusters
    _fields_ = [
        ("min_fraction", C.c_float),
        ("fragment_length", C.c_int32),
        ("min_identity", C.c_float),
        ("reciprocal", C.c_int32),
    ]


class BestParams(C.Structure):
    # fa_best_params: the filters, the cut-offs and k of fa_table_best
    _fields_ = [
        ("min_fraction", C.c_float),
        ("fragment_length", C.c_int32),
        ("min_identity", C.c_float),
        ("min_aligned_fraction", C.c_float),
        ("k", C.c_int32),
        ("exclude_self", C.c_int32),
    ]


class ScreenPair(C.Structure):
    # fa_screen_pair: one genome pair of the signature screen (pyfastani_amd.screen.SCREEN_DTYPE is the numpy face of it)
    _fields_ = [
        ("a", C.c_int32),
        ("b", C.c_int32),
        ("shared", C.c_int32),
        ("denom", C.c_int32),
    ]


# fa_mapping_sink: int (*)(void *user, const fa_hit_mapping *records, int64_t n); the entry points take it as a plain pointer
# (None = count only), so wrap a Python function as ``MAPPING_SINK(fn)`` and pass ``ctypes.cast(cb, ctypes.c_void_p)``
MAPPING_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(HitMapping), C.c_int64)

# every symbol of include/fastani_hip.h: (restype, argtypes)
_vp, _i32, _i64, _u64, _u32, _f32, _f64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint32, C.c_float, C.c_double
_P = C.POINTER
SIGNATURES = {
    "fa_last_error": (C.c_char_p, []),
    "fa_version": (_i32, []),
    "fa_device_trim": (_i32, [_P(C.c_uint64)]),
    "fa_device_count": (_i32, [_P(_i32)]),
    "fa_set_device": (_i32, [_i32]),
    "fa_recommended_window_size": (_i32, [_f64, _i32, _i32, _f32, _i32, _u64, _P(_i32)]),
    "fa_estimate_minimum_hits_relaxed": (_i32, [_i32, _i32, _f32, _P(_i32)]),
    "fa_mapping_identity": (_i32, [_i32, _i32, _i32, _P(_f32), _P(_f32)]),
    "fa_pass_threshold": (_i32, [_i32, _i32, _f32, _f32, _P(_i32)]),
    "fa_hash": (_u32, [C.c_char_p, _i32]),
    "fa_sketch_new": (_i32, [_P(Params), _P(_vp)]),
    "fa_sketch_free": (None, [_vp]),
    "fa_sketch_add_contig": (_i32, [_vp, _vp, _i64, _i32, _P(_i32)]),
    "fa_sketch_end_genome": (_i32, [_vp]),
    "fa_sketch_abort_genome": (_i32, [_vp]),
    "fa_sketch_clear": (_i32, [_vp]),
    "fa_sketch_num_minimizers": (_i32, [_vp, _P(_i64)]),
    "fa_sketch_get_minimizers": (_i32, [_vp, _vp, _vp, _vp]),
    "fa_sketch_num_genomes": (_i32, [_vp, _P(_i64)]),
    "fa_sketch_get_state": (_i32, [_vp, _vp, _vp, _P(_i64)]),
    "fa_sketch_set_state": (_i32, [_vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "fa_sketch_get_minimizers_device": (_i32, [_vp, _i64, _vp, _vp, _vp]),
    "fa_sketch_set_state_device": (_i32, [_vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "fa_sketch_index": (_i32, [_vp, _P(_vp)]),
    "fa_sketch_select": (_i32, [_vp, _vp, _i32, _P(_vp)]),
    "fa_sketch_frequency": (_i32, [_vp, _P(_i32), _i64, _vp, _P(_i64)]),
    "fa_mapper_free": (None, [_vp]),
    "fa_mapper_freq_threshold": (_i32, [_vp, _P(_i32)]),
    "fa_mapper_lookup_export_device": (_i32, [_vp, _i64, _vp, _vp]),
    "fa_mapper_set_global_frequency": (_i32, [_vp, _i32, _i64, _vp]),
    "fa_mapper_lookup_size": (_i32, [_vp, _P(_i64)]),
    "fa_mapper_device": (_i32, [_vp, _P(_i32)]),
    "fa_mapper_lookup_keys": (_i32, [_vp, _vp]),
    "fa_mapper_lookup_count": (_i32, [_vp, _u32, _P(_i64)]),
    "fa_mapper_lookup_get": (_i32, [_vp, _u32, _vp, _vp, _i64]),
    "fa_mapper_num_minimizers": (_i32, [_vp, _P(_i64)]),
    "fa_mapper_get_minimizers": (_i32, [_vp, _vp, _vp, _vp]),
    "fa_mapper_num_genomes": (_i32, [_vp, _P(_i64)]),
    "fa_mapper_get_state": (_i32, [_vp, _vp, _vp]),
    "fa_mapper_query": (_i32, [_vp, _P(_vp), _P(_i64), _i32, _i32, _vp, _i64, _P(_i64), _P(_i32), _P(_u64), _P(_u64)]),
    "fa_mapper_query_mappings": (_i32, [_vp, _P(_vp), _P(_i64), _i32, _i32, _vp, _i64, _P(_i64), _P(_i32), _P(_u64), _P(_u64),
                                        _vp, _i64, _P(_i64)]),
    "fa_genomes_upload": (_i32, [_vp, _P(_vp), _P(_i64), _vp, _i64, _i32, _i32, _P(_vp)]),
    "fa_genomes_free": (None, [_vp]),
    "fa_genomes_info": (_i32, [_vp, _P(_i32), _vp, _vp, _vp]),
    "fa_mapper_query_genomes": (_i32, [_vp, _vp, _i32, _i32, _vp, _i64, _P(_i64), _i32]),
    "fa_mapper_query_genomes_mappings": (_i32, [_vp, _vp, _i32, _i32, _vp, _i64, _P(_i64), _i32, _vp, _i64, _P(_i64), _i32]),
    "fa_mapper_query_mappings_stream": (_i32, [_vp, _P(_vp), _P(_i64), _i32, _i32, _vp, _i64, _P(_i64), _P(_i32), _P(_u64), _P(_u64),
                                               _vp, _vp, _P(_i64)]),
    "fa_mapper_query_genomes_mappings_stream": (_i32, [_vp, _vp, _i32, _i32, _vp, _i64, _P(_i64), _i32, _vp, _vp, _P(_i64)]),
    "fa_mapper_set_mapping_stage": (_i32, [_vp, _i64]),
    "fa_rules_default": (_i32, [_P(RulesStruct)]),
    "fa_mapper_set_rules": (_i32, [_vp, _P(RulesStruct)]),
    "fa_mapper_get_rules": (_i32, [_vp, _P(RulesStruct)]),
    "fa_mapper_mapping_memory": (_i32, [_vp, _P(_i64)]),
    "fa_table_pairs": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _P(TableParams), _vp, _i64, _P(_i64), _i32]),
    "fa_table_clusters": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _P(TableParams), _vp, _i32, _P(_i32), _vp]),
    "fa_table_representatives": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _P(TableParams), _vp, _vp, _vp, _i32, _P(_i32), _vp]),
    "fa_table_linkage": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _P(TableParams), _f32, _vp, _i32, _P(_i32), _vp]),
    "fa_table_dendrogram": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _P(TableParams), _f32, _vp, _i64, _P(_i64), _vp, _i32, _P(_i32), _vp]),
    "fa_dendrogram_cut": (_i32, [_vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _vp]),
    "fa_debug_linkage_order": (_i32, [_P(_i64), _P(_i64), _P(_i32)]),
    "fa_table_medoids": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _P(TableParams), _f32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    "fa_debug_medoid_better": (_i32, [_f64, _i64, _i32, _f64, _i64, _i32, _i32, _P(_i64), _P(_i32)]),
    "fa_mappings_profile": (_i32, [_vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp]),
    "fa_profile_summary": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i32]),
    "fa_profile_chunk": (_i32, [_P(_i32), _P(_i32)]),
    "fa_debug_profile_road": (_i32, [_i32]),
    "fa_mapper_reference_bins": (_i32, [_vp, _P(_i32), _P(_i64), _vp, _vp]),
    "fa_mappings_reference_profile": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp]),
    "fa_reference_profile_chunk": (_i32, [_P(_i32)]),
    "fa_profile_regions": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _i64, _P(_i64), _i32]),
    "fa_profile_regions_chunk": (_i32, [_P(_i32)]),
    "fa_table_best": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _P(BestParams), _vp, _vp, _i64, _P(_i64), _i32, _vp]),
    "fa_screen_tile": (_i32, [_i32, _P(_i32)]),
    "fa_screen_signatures": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32, _vp, _vp]),
    "fa_genomes_signatures": (_i32, [_vp, _vp, _i32, _i32, _i32, _i64, _vp, _vp, _vp]),
    "fa_screen_pairs": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _P(_i64), _i32, _vp]),
    "fa_screen_groups": (_i32, [_vp, _i64, _i32, _i32, _vp, _i32, _P(_i32)]),
    "fa_screen_contents": (_i32, [_vp, _vp, _i64, _vp, _i32, _vp, _vp, _i64, _P(_i64)]),
    "fa_screen_contain_slice": (_i32, [_P(_i32)]),
    "fa_screen_contained": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _i64, _P(_i64), _i32, _vp]),
    "fa_screen_contained_winner": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _i64, _P(_i64), _i32, _vp]),
    "fa_debug_contain_winner_threads": (_i32, [_i32]),
    "fa_mapper_debug_mappings": (_i32, [_vp, _vp, _i64, _P(_i64)]),
    "fa_mapper_debug_l1": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _P(_i64)]),
    "fa_mapper_debug_query_sketch": (_i32, [_vp, _i64, _vp, _i32, _P(_i32)]),
    "fa_debug_sketch_sequence": (_i32, [_P(Params), _vp, _i64, _i32, _vp, _vp, _i64, _P(_i64)]),
    "fa_fasta_open": (_i32, [C.c_char_p, _P(_vp)]),
    "fa_fasta_next": (_i32, [_vp, _P(_i32), _P(_vp), _P(_i64), _P(_vp), _P(_i64)]),
    "fa_fasta_close": (None, [_vp]),
    "fa_sketch_add_fasta": (_i32, [_vp, C.c_char_p, _P(_i64), _P(_i64)]),
    "fa_genomes_upload_fasta": (_i32, [_vp, _P(C.c_char_p), _i32, _P(_vp)]),
    "fa_packed_read": (_i32, [_P(C.c_char_p), _i32, _i32, _P(_vp)]),
    "fa_packed_append": (_i32, [_vp, _P(C.c_char_p), _i32]),
    "fa_packed_free": (None, [_vp]),
    "fa_packed_info": (_i32, [_vp, _P(_i32), _P(C.c_uint64), _P(_i64), _P(_i64)]),
    "fa_sketch_add_packed": (_i32, [_vp, _vp, _i32, _i32, _P(_i64), _P(_i64)]),
    "fa_genomes_reload_packed": (_i32, [_vp, _vp, _vp, _i32, _i32]),
    "fa_genomes_reload_fasta": (_i32, [_vp, _vp, _P(C.c_char_p), _i32]),
    "fa_sketch_add_genomes": (_i32, [_vp, _P(_vp), _P(_i64), _P(_i32), _i64, _i32, _i32, _P(_i32)]),
    "fa_sketch_add_fasta_many": (_i32, [_vp, _P(C.c_char_p), _i32, _P(_i64), _P(_i64)]),
    "fa_debug_probe_occupancy": (_i32, [_i32, _P(_i32)]),
    "fa_mapper_debug_items": (_i32, [_vp, _vp, _i64]),
    "fa_mapper_debug_locus_events": (_i32, [_vp, _vp, _i64, _vp]),
    "fa_mapper_debug_links": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "fa_mapper_last_timings": (_i32, [_vp, _P(_f32), _i32]),
    "fa_mapper_debug_spec": (_i32, [_vp, _P(_i64), _i32]),
    "fa_mapper_set_stage_events": (_i32, [_vp, _i32]),
    "fa_mapper_stream": (_i32, [_vp, _P(_vp)]),
    "fa_bench_sketch_kernel": (_i32, [_vp, _vp, _i32, _P(_f32), _P(_u64), _P(_u64)]),
}

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). pyfastani_amd has no CPU fallback."
    )



# Concurrent query calls each use their own stream; the runtime's default of 4 hardware queues would put several of them
# on one queue (measured: two part streams serialised), so ask for more before HIP starts.  Nothing else is touched at
# import: in particular PyTorch is NOT imported here (a process that uses both imports torch first, see sharding.py).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
lib = C.CDLL(LIB_PATH)
for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here means the library and the header disagree
    _fn.restype = _res
    _fn.argtypes = _args


def last_error():
    msg = lib.fa_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(code):
    """Map a C status code onto the exception the reference would raise."""
    if code == FA_OK:
        return
    msg = last_error()
    if code == FA_ERR_INVALID:
        raise ValueError(msg)
    if code == FA_ERR_NOMEM:
        raise MemoryError(msg)
    if code == FA_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if code == FA_ERR_IO:
        raise OSError(msg)
    if code == FA_ERR_BUFFER:
        raise BufferError(msg)
    raise RuntimeError(msg)


def device_count():
    n = C.c_int(0)
    lib.fa_device_count(C.byref(n))
    return n.value
