"""ctypes mirror of include/lmat_hip.h (same names, same argument order, same error codes)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LMAT_LIB") or os.path.join(_HERE, "liblmat_hip.so")  # LMAT_LIB: A/B builds when profiling


class LmatError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lmat error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """lmat_params: ScoreOptions + proc_line thresholds (src/read_label.cpp:487-497,1336-1337)."""
    _fields_ = [("sdiff", C.c_float), ("hbias", C.c_float), ("min_score", C.c_float), ("min_kmer", C.c_int32),
                ("min_fnd_kmer", C.c_int32), ("prn_all", C.c_int32), ("screen_phix", C.c_int32)]

    @classmethod
    def run_rl(cls, prn_all=1):
        """The flags bin/run_rl.sh passes with --nullm=no: -x 0 -j 30 -l 0 -b 1.0 -p."""
        return cls(1.0, 0.0, 0.0, 30, 1, prn_all, 1)


class BuildStats(C.Structure):
    """lmat_build_stats: what lmat_build_run counted and the HIP-event time of every stage."""
    _fields_ = [("bases", C.c_uint64), ("windows", C.c_uint64), ("emitted_pairs", C.c_uint64), ("distinct_kmers", C.c_uint64),
                ("records_written", C.c_uint64), ("dropped_unknown", C.c_uint64), ("singletons", C.c_uint64),
                ("total_list_entries", C.c_uint64), ("longest_list", C.c_uint64), ("passes", C.c_uint32), ("prefix_bits", C.c_uint32),
                ("extract_ms", C.c_float), ("sort_ms", C.c_float), ("segment_ms", C.c_float), ("closure_ms", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MergeStats(C.Structure):
    """lmat_merge_stats: what the merge of tax_histo inputs counted and the HIP-event time of its stages."""
    _fields_ = [("inputs", C.c_uint32), ("passes", C.c_uint32), ("records_in", C.c_uint64), ("entries_in", C.c_uint64),
                ("records_one_source", C.c_uint64), ("records_merged", C.c_uint64), ("records_grown", C.c_uint64),
                ("upload_ms", C.c_float), ("sort_ms", C.c_float), ("segment_ms", C.c_float), ("union_ms", C.c_float), ("histogram_ms", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CovStats(C.Structure):
    """lmat_cov_stats: what lmat_cov_run counted and the HIP-event time of every stage."""
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("windows", C.c_uint64), ("runs", C.c_uint64), ("passes", C.c_uint32),
                ("prefix_bits", C.c_uint32), ("extract_ms", C.c_float), ("sort_ms", C.c_float), ("segment_ms", C.c_float),
                ("histogram_ms", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ExportStats(C.Structure):
    """lmat_export_stats: what lmat_export_run counted, the HIP-event time of the device stages and the host time of fetch and file."""
    _fields_ = [("records", C.c_uint64), ("entries", C.c_uint64), ("singletons", C.c_uint64), ("from_buckets", C.c_uint64),
                ("from_overflow", C.c_uint64), ("passes", C.c_uint64), ("prefix_bits", C.c_int), ("ms_scan", C.c_double),
                ("ms_sort", C.c_double), ("ms_lists", C.c_double), ("ms_fetch", C.c_double), ("ms_write", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ExportFilter(C.Structure):
    """lmat_export_filter: the taxonomic slice of an export (Export.set_filter)."""
    _fields_ = [("taxa", C.POINTER(C.c_uint32)), ("n_taxa", C.c_uint32), ("mode", C.c_int), ("min_lca_depth", C.c_uint32), ("max_entries", C.c_uint32)]


SLICE_MODES = {"any": 1, "all": 2, "none": 3}    # LMAT_SLICE_*

READ_RESULT_DTYPE = np.dtype([("status", "u1"), ("match_type", "u1"), ("cand_kmer_cnt", "<u2"), ("valid_kmers", "<i4"),
                              ("read_len", "<i4"), ("log_avg", "<f4"), ("stdev", "<f4"), ("call_tid", "<u4"),
                              ("call_score", "<f4"), ("cand_off", "<u4"), ("n_cand", "<u4"), ("bin_sel", "<i4")])
CAND_DTYPE = np.dtype([("tid", "<u4"), ("score", "<f4")])

_lib = None


def load_library(path: str | None = None):
    """Loads liblmat_hip.so.  There is no fallback: a missing library is an error."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(f"{p} not found: build it with `make -C lmat_amd/csrc` (hipcc, gfx950); "
                          "lmat_amd has no CPU implementation")
    lib = C.CDLL(p)
    vp, u64, u32, i32, cp = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p
    P = C.POINTER
    sig = {
        "lmat_device_count": (i32, []),
        "lmat_ctx_create": (i32, [i32, P(Params), P(vp)]),
        "lmat_ctx_destroy": (None, [vp]),
        "lmat_last_error": (cp, [vp]),
        "lmat_set_params": (i32, [vp, P(Params)]),
        "lmat_taxonomy_load_files": (i32, [vp, cp, cp, cp, cp, cp]),
        "lmat_db_begin": (i32, [vp, i32, u64, u64]),
        "lmat_genedb_begin": (i32, [vp, i32, u64, u64]),
        "lmat_db_add_taxhisto": (i32, [vp, cp]),
        "lmat_db_finalize": (i32, [vp]),
        "lmat_db_set_build_options": (i32, [vp, i32, cp, cp, cp, u32]),
        "lmat_db_save_image": (i32, [vp, cp]),
        "lmat_db_load_image": (i32, [vp, cp, u64]),
        "lmat_ingest_create": (i32, [i32, cp, P(vp)]),
        "lmat_ingest_idmap_from_tree": (i32, [vp, cp]),
        "lmat_ingest_destroy": (None, [vp]),
        "lmat_ingest_error": (cp, [vp]),
        "lmat_ingest_set_options": (i32, [vp, i32, cp, cp, cp, u32]),
        "lmat_ingest_add_taxhisto": (i32, [vp, cp]),
        "lmat_ingest_save_image": (i32, [vp, cp]),
        "lmat_ingest_load_image": (i32, [cp, P(vp)]),
        "lmat_ingest_size": (u64, [vp]),
        "lmat_ingest_kmer_length": (i32, [vp]),
        "lmat_ingest_lookup": (i32, [vp, u64, vp, i32]),
        "lmat_db_from_ingest": (i32, [vp, vp, u64]),
        "lmat_set_label_modes": (i32, [vp, i32, i32, cp]),
        "lmat_rand_mode": (i32, [vp, i32]),
        "lmat_rand_reset": (i32, [vp, u32]),
        "lmat_rand_label": (i32, [vp, vp, u64, u64, vp]),
        "lmat_rand_get": (i32, [vp, vp, vp, vp, u32, P(u32)]),
        "lmat_nullmodel_load": (i32, [vp, cp]),
        "lmat_nullmodel_clear": (i32, [vp]),
        "lmat_db_kmer_length": (i32, [vp]),
        "lmat_db_size": (u64, [vp]),
        "lmat_db_list_count": (u64, [vp]),
        "lmat_db_arena_bytes": (u64, [vp]),
        "lmat_db_table_bytes": (u64, [vp]),
        "lmat_db_lookup": (i32, [vp, vp, u64, vp, vp, u32]),
        "lmat_synth_taxonomy": (i32, [vp, vp]),
        "lmat_synth_db_build": (i32, [vp, i32, u64, u64, u64]),
        "lmat_synth_db_build2": (i32, [vp, i32, u64, u64, u64, u32, u32]),
        "lmat_synth_db_build3": (i32, [vp, i32, u64, u64, u64, u32, u32, vp]),
        "lmat_reads_upload": (i32, [vp, vp, vp, u64, P(vp)]),
        "lmat_reads_synth": (i32, [vp, u64, vp, u32, u64, P(vp)]),
        "lmat_reads_download_ascii": (i32, [vp, vp, u64, u64, vp, vp]),
        "lmat_reads_count": (u64, [vp]),
        "lmat_reads_device_bytes": (u64, [vp]),
        "lmat_reads_free": (None, [vp, vp]),
        "lmat_classify": (i32, [vp, vp, u64, u64, vp, vp, u64, P(u64)]),
        "lmat_classify_async": (i32, [vp, vp, u64, u64]),
        "lmat_classify_async_cands": (i32, [vp, vp, u64, u64, u64]),
        "lmat_comm_available": (i32, []),
        "lmat_sync": (i32, [vp, P(C.c_float), P(u64)]),
        "lmat_last_timing": (i32, [vp, P(C.c_float), P(C.c_float), P(u64)]),
        "lmat_results_fetch": (i32, [vp, u64, u64, vp]),
        "lmat_counts_reset": (i32, [vp]),
        "lmat_counts_layout": (i32, [vp, P(u32), P(u64)]),
        "lmat_counts_device_ptr": (vp, [vp]),
        "lmat_counts_get": (i32, [vp, vp, vp, vp, u32, P(u32), vp]),
        "lmat_gather_bench": (i32, [vp, u64, u64, P(C.c_float), P(u64)]),
        "lmat_stream_create": (i32, [vp, u64, u64, u32, i32, P(vp)]),
        "lmat_stream_acquire": (i32, [vp, P(vp), P(vp)]),
        "lmat_stream_submit": (i32, [vp, u64, u64]),
        "lmat_stream_submit_from": (i32, [vp, vp, vp, u64, u64]),
        "lmat_host_alloc": (i32, [u64, P(vp)]),
        "lmat_host_free": (None, [vp]),
        "lmat_stream_next": (i32, [vp, P(vp), P(vp), P(u64), P(u64), P(u64)]),
        "lmat_stream_release": (i32, [vp]),
        "lmat_stream_destroy": (None, [vp]),
        "lmat_debug_stream_stats": (i32, [vp, vp]),
        "lmat_debug_reads_words": (i32, [vp, vp, u64, u64, vp, vp]),
        "lmat_counts_allreduce": (i32, [P(vp), i32]),
        "lmat_comm_unique_id": (i32, [vp]),
        "lmat_comm_init": (i32, [vp, vp, i32, i32]),
        "lmat_comm_allreduce_counts": (i32, [vp]),
        "lmat_comm_size": (i32, [vp]),
        "lmat_comm_destroy": (None, [vp]),
        "lmat_db_clone": (i32, [vp, vp]),
        "lmat_debug_decide": (i32, [vp, vp, vp, vp, vp, u64, vp]),
        "lmat_debug_decide_counts": (i32, [vp, vp, vp, vp, vp, u64, i32, vp]),
        "lmat_debug_decide_chain": (i32, [vp, vp, vp, vp, vp, vp, vp, u64, i32, vp, vp]),
        "lmat_debug_decide_shape": (i32, [vp, vp, vp, vp, vp, vp, u64, i32, vp, vp]),
        "lmat_synth_window": (i32, [vp, u32, u64, P(u64), vp, u32, P(u32)]),
        "lmat_debug_last_counters": (i32, [vp, vp]),
        "lmat_debug_probe_stats": (i32, [vp, vp, u64, vp]),
        "lmat_debug_div_check": (i32, [vp, vp]),
        "lmat_debug_variant_launches": (i32, [vp, vp]),
        "lmat_debug_uniform_launches": (i32, [vp, vp]),
        "lmat_debug_classify_grid": (i32, [vp, vp]),
        "lmat_synth_read_windows": (i32, [vp, vp, u32, u64, u64, vp, vp, vp, u32, u32, P(u32), P(u32)]),
        "lmat_table_address": (i32, [i32, u64, u64, P(u64), P(u32), P(u32)]),
        "lmat_format_out": (C.c_int64, [vp, vp, u64, vp, vp, vp, i32, u64, vp, u64]),
        "lmat_build_create": (i32, [vp, i32, cp, P(vp)]),
        "lmat_build_destroy": (None, [vp]),
        "lmat_build_error": (cp, [vp]),
        "lmat_build_set_options": (i32, [vp, u64, i32, u32]),
        "lmat_build_add_fasta": (i32, [vp, cp]),
        "lmat_build_add_sequence": (i32, [vp, u32, vp, u64]),
        "lmat_build_run": (i32, [vp, P(BuildStats)]),
        "lmat_build_write_taxhisto": (i32, [vp, cp]),
        "lmat_build_fetch": (i32, [vp, u64, u64, vp, vp, vp, u64]),
        "lmat_db_build_from_genomes": (i32, [vp, vp, u64]),
        "lmat_build_add_taxhisto": (i32, [vp, cp]),
        "lmat_build_merge_stats": (i32, [vp, P(MergeStats)]),
        "lmat_build_taxid_counts": (i32, [vp, vp, vp, u64, P(u64)]),
        "lmat_cov_create": (i32, [vp, vp, i32, P(vp)]),
        "lmat_cov_destroy": (None, [vp]),
        "lmat_cov_error": (cp, [vp]),
        "lmat_cov_set_options": (i32, [vp, u64, i32]),
        "lmat_cov_add_reads": (i32, [vp, vp, vp, u64, vp]),
        "lmat_cov_run": (i32, [vp, P(CovStats)]),
        "lmat_cov_summary": (i32, [vp, i32, vp, vp, vp, u64, P(u64)]),
        "lmat_cov_histogram": (i32, [vp, i32, u32, vp, vp, u64, P(u64)]),
        "lmat_export_create": (i32, [vp, P(vp)]),
        "lmat_export_destroy": (None, [vp]),
        "lmat_export_error": (cp, [vp]),
        "lmat_export_set_options": (i32, [vp, u64, i32]),
        "lmat_export_run": (i32, [vp, cp, P(ExportStats)]),
        "lmat_export_fetch": (i32, [vp, u64, u64, vp, vp, vp, u64]),
        "lmat_export_taxid_counts": (i32, [vp, vp, vp, u64, P(u64)]),
        "lmat_export_set_filter": (i32, [vp, P(ExportFilter)]),
        "lmat_export_filter_stats": (i32, [vp, P(u64), P(C.c_double)]),
        "lmat_db_from_export": (i32, [vp, vp, u64]),
        "lmat_build_add_db": (i32, [vp, vp]),
        "lmat_genebuild_create": (i32, [vp, i32, P(vp)]),
        "lmat_genedb_build_from_genes": (i32, [vp, vp, u64]),
        "lmat_table_unaddress": (i32, [i32, u64, u32, u32, P(u64)]),
        "lmat_reads_upload_pairs": (i32, [vp, vp, vp, vp, vp, u64, P(vp)]),
        "lmat_stream_submit_pairs": (i32, [vp, u64, u64]),
        "lmat_stream_submit_pairs_from": (i32, [vp, vp, vp, vp, vp, u64, u64]),
        "lmat_image_check": (i32, [cp, vp, u64]),
        "lmat_bins_create": (i32, [vp, P(vp)]),
        "lmat_bins_destroy": (None, [vp]),
        "lmat_bins_error": (cp, [vp]),
        "lmat_bins_set": (i32, [vp, vp, u32, C.c_float, i32]),
        "lmat_bins_set_from_file": (i32, [vp, cp, C.c_float, i32]),
        "lmat_bins_run": (i32, [vp, vp, u64, u64, i32]),
        "lmat_bins_counts": (i32, [vp, vp, vp]),
        "lmat_bins_fetch": (i32, [vp, u32, vp, vp, vp]),
        "lmat_debug_bins_select": (i32, [vp, vp, u64, vp]),
        "lmat_stream_set_bins": (i32, [vp, vp]),
        "lmat_stream_next_bins": (i32, [vp, P(vp), P(vp)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


EXPORTED = ["lmat_device_count", "lmat_ctx_create", "lmat_ctx_destroy", "lmat_last_error", "lmat_set_params", "lmat_taxonomy_load_files",
            "lmat_db_begin", "lmat_genedb_begin", "lmat_db_add_taxhisto", "lmat_db_finalize", "lmat_db_kmer_length", "lmat_db_size", "lmat_db_list_count", "lmat_db_arena_bytes",
            "lmat_db_set_build_options", "lmat_db_save_image", "lmat_db_load_image", "lmat_ingest_create", "lmat_ingest_idmap_from_tree", "lmat_rand_mode", "lmat_rand_reset", "lmat_rand_label", "lmat_rand_get",
            "lmat_ingest_destroy", "lmat_ingest_error", "lmat_ingest_set_options", "lmat_ingest_add_taxhisto",
            "lmat_ingest_save_image", "lmat_ingest_load_image", "lmat_ingest_size", "lmat_ingest_kmer_length",
            "lmat_ingest_lookup", "lmat_db_from_ingest", "lmat_nullmodel_load", "lmat_nullmodel_clear", "lmat_set_label_modes",
            "lmat_db_table_bytes", "lmat_db_lookup", "lmat_synth_taxonomy", "lmat_synth_db_build", "lmat_synth_db_build2", "lmat_synth_db_build3", "lmat_reads_upload",
            "lmat_reads_synth", "lmat_reads_download_ascii", "lmat_reads_count", "lmat_reads_device_bytes",
            "lmat_reads_free", "lmat_classify", "lmat_classify_async", "lmat_classify_async_cands", "lmat_comm_available", "lmat_sync", "lmat_last_timing", "lmat_results_fetch",
            "lmat_counts_reset", "lmat_counts_layout", "lmat_counts_device_ptr", "lmat_counts_get", "lmat_gather_bench",
            "lmat_table_address", "lmat_format_out", "lmat_stream_create", "lmat_stream_acquire", "lmat_stream_submit", "lmat_stream_submit_from", "lmat_host_alloc", "lmat_host_free",
            "lmat_stream_next", "lmat_stream_release", "lmat_stream_destroy", "lmat_counts_allreduce",
            "lmat_comm_unique_id", "lmat_comm_init", "lmat_comm_allreduce_counts", "lmat_comm_size", "lmat_comm_destroy", "lmat_db_clone", "lmat_debug_decide", "lmat_debug_decide_counts", "lmat_debug_decide_chain", "lmat_debug_decide_shape", "lmat_synth_window", "lmat_synth_read_windows", "lmat_debug_probe_stats", "lmat_debug_last_counters", "lmat_debug_div_check", "lmat_debug_variant_launches", "lmat_debug_uniform_launches", "lmat_debug_classify_grid",
            "lmat_build_create", "lmat_build_destroy", "lmat_build_error", "lmat_build_set_options", "lmat_build_add_fasta", "lmat_build_add_sequence",
            "lmat_build_run", "lmat_build_write_taxhisto", "lmat_build_fetch", "lmat_db_build_from_genomes",
            "lmat_build_add_taxhisto", "lmat_build_merge_stats", "lmat_build_taxid_counts",
            "lmat_cov_create", "lmat_cov_destroy", "lmat_cov_error", "lmat_cov_set_options", "lmat_cov_add_reads", "lmat_cov_run",
            "lmat_cov_summary", "lmat_cov_histogram",
            "lmat_export_create", "lmat_export_destroy", "lmat_export_error", "lmat_export_set_options", "lmat_export_run", "lmat_export_fetch",
            "lmat_export_taxid_counts", "lmat_export_set_filter", "lmat_export_filter_stats", "lmat_db_from_export", "lmat_build_add_db", "lmat_table_unaddress",
            "lmat_genebuild_create", "lmat_genedb_build_from_genes",
            "lmat_debug_stream_stats", "lmat_debug_reads_words",
            "lmat_reads_upload_pairs", "lmat_stream_submit_pairs", "lmat_stream_submit_pairs_from", "lmat_image_check",
            "lmat_bins_create", "lmat_bins_destroy", "lmat_bins_error", "lmat_bins_set", "lmat_bins_set_from_file", "lmat_bins_run", "lmat_bins_counts",
            "lmat_bins_fetch", "lmat_debug_bins_select", "lmat_stream_set_bins", "lmat_stream_next_bins"]


def image_check(path):
    """The header checks of a device image (LMATIMG2) without a context or a device -> (code, message): (0, "") for a usable one."""
    buf = C.create_string_buffer(1024)
    rc = load_library().lmat_image_check(path.encode(), buf, len(buf))
    return rc, buf.value.decode(errors="replace")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Reads:
    def __init__(self, eng, handle):
        self.eng, self.h = eng, handle

    def __len__(self):
        return int(self.eng.lib.lmat_reads_count(self.h))

    @property
    def device_bytes(self):
        return int(self.eng.lib.lmat_reads_device_bytes(self.h))

    def ascii(self, first=0, count=None):
        """-> (bases uint8 array, offsets uint64[count+1]) decoded back from the packed device records."""
        n = len(self) - first if count is None else count
        off = np.zeros(n + 1, dtype=np.uint64)
        self.eng._chk(self.eng.lib.lmat_reads_download_ascii(self.eng.ctx, self.h, first, n, None, _ptr(off)))
        bases = np.zeros(int(off[-1]) + 1, dtype=np.uint8)
        self.eng._chk(self.eng.lib.lmat_reads_download_ascii(self.eng.ctx, self.h, first, n, _ptr(bases), _ptr(off)))
        return bases[:-1], off

    def words(self, first=0, count=None):
        """-> (words uint32, rec_off uint64[count+1]): the packed records as they lie on the device, offsets from the first one."""
        n = len(self) - first if count is None else count
        ro = np.zeros(n + 1, dtype=np.uint64)
        self.eng._chk(self.eng.lib.lmat_debug_reads_words(self.eng.ctx, self.h, first, n, None, _ptr(ro)))
        w = np.zeros(max(int(ro[-1]), 1), dtype=np.uint32)
        self.eng._chk(self.eng.lib.lmat_debug_reads_words(self.eng.ctx, self.h, first, n, _ptr(w), _ptr(ro)))
        return w[:int(ro[-1])], ro

    def free(self):
        if self.h:
            self.eng.lib.lmat_reads_free(self.eng.ctx, self.h)
            self.h = None


class Ingest:
    """GPU-free ingest (lmat_ingest): make_db_table's parsing and options, canonical 16-bit lists."""

    def __init__(self, k=None, idmap=None, image=None, tree=None):
        """idmap: the 32->16 map file; or tree (no map): a database of 32-bit taxids, codes from the tree."""
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.lmat_ingest_load_image(image.encode(), C.byref(h)) if image else \
            self.lib.lmat_ingest_create(k, idmap.encode() if idmap else None, C.byref(h))
        if rc != 0:
            raise LmatError(rc, "cannot create ingest")
        self.h = h
        if not image and not idmap:
            self._chk(self.lib.lmat_ingest_idmap_from_tree(self.h, tree.encode()))

    def _chk(self, rc):
        if rc != 0:
            raise LmatError(rc, self.lib.lmat_ingest_error(self.h).decode(errors="replace"))

    def set_options(self, tid_cutoff=0, rank_map=None, human_kmers=None, adaptor_kmers=None, adaptor_tid=0):
        e = lambda s: s.encode() if s else None
        self._chk(self.lib.lmat_ingest_set_options(self.h, tid_cutoff, e(rank_map), e(human_kmers), e(adaptor_kmers), adaptor_tid))

    def add_taxhisto(self, fn):
        self._chk(self.lib.lmat_ingest_add_taxhisto(self.h, fn.encode()))

    def save_image(self, fn):
        self._chk(self.lib.lmat_ingest_save_image(self.h, fn.encode()))

    def __len__(self):
        return int(self.lib.lmat_ingest_size(self.h))

    @property
    def k(self):
        return int(self.lib.lmat_ingest_kmer_length(self.h))

    def lookup(self, kmer, cap=4096):
        out = np.zeros(cap, dtype=np.uint16)
        n = self.lib.lmat_ingest_lookup(self.h, int(kmer), _ptr(out), cap)
        return out[:max(n, 0)].tolist()

    def close(self):
        if self.h:
            self.lib.lmat_ingest_destroy(self.h)
            self.h = None


def host_alloc(nbytes):
    """Page-locked host memory (lmat_host_alloc) -> address; free with host_free."""
    lib = load_library()
    p = C.c_void_p()
    rc = lib.lmat_host_alloc(int(nbytes), C.byref(p))
    if rc != 0:
        raise LmatError(rc, "out of pinned host memory")
    return p.value


def host_free(addr):
    load_library().lmat_host_free(C.c_void_p(addr))


class Stream:
    """lmat_stream: a ring of pinned batch slots; copy in, classification and copy out of consecutive batches overlap."""

    def __init__(self, eng, max_reads, max_bases, cands_per_read=0, n_slots=3):
        self.eng, self.lib = eng, eng.lib
        self.max_reads, self.max_bases, self.n_slots = int(max_reads), int(max_bases), n_slots
        h = C.c_void_p()
        eng._chk(self.lib.lmat_stream_create(eng.ctx, self.max_reads, self.max_bases, cands_per_read, n_slots, C.byref(h)))
        self.h = h
        self.in_flight = 0
        self.bins = None
        self._bins_used = False
        self._ng = []   # per batch in flight: the group count of the bins it was submitted under

    def set_bins(self, bins):
        """Batches submitted from now on are partitioned by the groups of `bins` (a Bins of the same engine; None clears): next()
        then returns their index lists as a fourth element."""
        self.eng._chk(self.lib.lmat_stream_set_bins(self.h, bins.h if bins is not None else None))
        self.bins = bins
        self._bins_used = self._bins_used or bins is not None

    def _lists(self):
        """Of the batch next() holds: [read indices (into the batch, ascending) per group], or None for a batch submitted without bins."""
        pg, pi = C.c_void_p(), C.c_void_p()
        rc = self.lib.lmat_stream_next_bins(self.h, C.byref(pg), C.byref(pi))
        if rc == -7:   # LMAT_E_STATE
            return None
        self.eng._chk(rc)
        ng = self._ng[0]
        goff = np.ctypeslib.as_array(C.cast(pg, C.POINTER(C.c_uint64)), shape=(ng + 1,)).copy()
        total = int(goff[-1])
        idx = np.ctypeslib.as_array(C.cast(pi, C.POINTER(C.c_uint32)), shape=(max(total, 1),))[:total].copy()
        return [idx[int(goff[g]):int(goff[g + 1])] for g in range(ng)]

    def submit(self, blob, off, tag=0):
        """blob: uint8 ASCII bases, off: uint64[n + 1]; copied into the slot's pinned buffers, then queued."""
        pb, po = C.c_void_p(), C.c_void_p()
        self.eng._chk(self.lib.lmat_stream_acquire(self.h, C.byref(pb), C.byref(po)))
        n = off.size - 1
        nb = int(off[-1])
        C.memmove(pb, blob.ctypes.data, nb)
        C.memmove(po, off.ctypes.data, (n + 1) * 8)
        self.eng._chk(self.lib.lmat_stream_submit(self.h, n, tag))
        self.in_flight += 1
        self._ng.append(self.bins.n_groups if self.bins is not None else None)

    def submit_pinned(self, bases_ptr, off, n, tag=0):
        """bases_ptr: address of the caller's own pinned buffer (host_alloc); off: uint64[n + 1] numpy array.  No copy."""
        pb, po = C.c_void_p(), C.c_void_p()
        self.eng._chk(self.lib.lmat_stream_acquire(self.h, C.byref(pb), C.byref(po)))
        self.eng._chk(self.lib.lmat_stream_submit_from(self.h, bases_ptr, off.ctypes.data, n, tag))
        self.in_flight += 1
        self._ng.append(self.bins.n_groups if self.bins is not None else None)

    def submit_pairs(self, blob, off, tag=0):
        """Paired-end: blob/off hold 2n reads, mates 1 and 2 in turn (off: uint64[2n + 1]); copied into the slot, joined on the
        device into n reads mate1 N mate2."""
        n2 = off.size - 1
        if n2 % 2:   # (before a slot is taken: an acquired slot has to be submitted)
            raise ValueError("an interleaved batch holds an even number of reads")
        pb, po = C.c_void_p(), C.c_void_p()
        self.eng._chk(self.lib.lmat_stream_acquire(self.h, C.byref(pb), C.byref(po)))
        # (a batch above the stream's limits is for the engine to refuse, from its count or its offsets: nothing is copied past a slot's end)
        if n2 <= self.max_reads:
            C.memmove(po, off.ctypes.data, (n2 + 1) * 8)
            if int(off[-1]) <= self.max_bases:
                C.memmove(pb, blob.ctypes.data, int(off[-1]))
        self.eng._chk(self.lib.lmat_stream_submit_pairs(self.h, n2 // 2, tag))
        self.in_flight += 1
        self._ng.append(self.bins.n_groups if self.bins is not None else None)

    def submit_pairs_pinned(self, ptr1, off1, ptr2, off2, n, tag=0):
        """Paired-end: mates 1 are off1[0..n] in the caller's pinned buffer at ptr1, mates 2 off2[0..n] at ptr2.  No host copy."""
        pb, po = C.c_void_p(), C.c_void_p()
        self.eng._chk(self.lib.lmat_stream_acquire(self.h, C.byref(pb), C.byref(po)))
        self.eng._chk(self.lib.lmat_stream_submit_pairs_from(self.h, ptr1, off1.ctypes.data, ptr2, off2.ctypes.data, n, tag))
        self.in_flight += 1
        self._ng.append(self.bins.n_groups if self.bins is not None else None)

    def next_nocopy(self):
        """Waits for the oldest batch and releases it at once -> (n_reads, n_cands, tag), or None."""
        pr, pc = C.c_void_p(), C.c_void_p()
        n, nc, tag = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.lmat_stream_next(self.h, C.byref(pr), C.byref(pc), C.byref(n), C.byref(nc), C.byref(tag))
        if rc == 1:
            return None
        self.eng._chk(rc)
        self.eng._chk(self.lib.lmat_stream_release(self.h))
        self.in_flight -= 1
        if self._ng:   # (a batch submitted through the library directly has no entry)
            self._ng.pop(0)
        return int(n.value), int(nc.value), int(tag.value)

    def next(self):
        """-> (results copy, cands copy or None, tag) of the oldest batch, or None when nothing is in flight."""
        pr, pc = C.c_void_p(), C.c_void_p()
        n, nc, tag = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.lmat_stream_next(self.h, C.byref(pr), C.byref(pc), C.byref(n), C.byref(nc), C.byref(tag))
        if rc == 1:
            return None
        self.eng._chk(rc)
        res = np.ctypeslib.as_array(C.cast(pr, C.POINTER(C.c_uint8)), shape=(n.value * READ_RESULT_DTYPE.itemsize,)).view(READ_RESULT_DTYPE).copy() if n.value else np.zeros(0, READ_RESULT_DTYPE)
        cands = None
        if pc.value and nc.value:
            cands = np.ctypeslib.as_array(C.cast(pc, C.POINTER(C.c_uint8)), shape=(nc.value * CAND_DTYPE.itemsize,)).view(CAND_DTYPE).copy()
        lists = self._lists() if self._bins_used else None
        self.eng._chk(self.lib.lmat_stream_release(self.h))
        self.in_flight -= 1
        if self._ng:   # (a batch submitted through the library directly has no entry)
            self._ng.pop(0)
        if self._bins_used:
            return res, cands, int(tag.value), lists
        return res, cands, int(tag.value)

    STATS = ("uniform", "general", "threaded", "class_lists", "grow_reruns", "cand_cap")

    def stats(self):
        """Host bookkeeping (lmat_debug_stream_stats): queued submits by branch, grow re-runs, the largest slot capacity in pairs."""
        out = np.zeros(6, dtype=np.uint64)
        self.eng._chk(self.lib.lmat_debug_stream_stats(self.h, _ptr(out)))
        return dict(zip(self.STATS, (int(x) for x in out)))

    def drop_failed(self):
        """Releases the oldest batch after next() has raised its error: the batches behind it come next."""
        self.eng._chk(self.lib.lmat_stream_release(self.h))
        self.in_flight -= 1
        if self._ng:   # (a batch submitted through the library directly has no entry)
            self._ng.pop(0)

    def close(self):
        if self.h:
            self.lib.lmat_stream_destroy(self.h)
            self.h = None


BIN_SUBTREE, BIN_REST, BIN_LOWSCORE, BIN_NODBHITS, BIN_NONE = 1, 2, 4, 8, 0xFFFF   # LMAT_BIN_*


class BinGroup(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("n_ids", C.c_uint32), ("flags", C.c_uint32), ("low_score", C.c_float)]


class Bins:
    """lmat_bins: the reads of a classified batch pulled by called taxon on the GPU (upstream's bin/pull_reads.pl).
    A group is (ids, flags) or (ids, flags, low_score); flags are BIN_*."""

    def __init__(self, eng):
        self.eng, self.lib = eng, eng.lib
        h = C.c_void_p()
        eng._chk(self.lib.lmat_bins_create(eng.ctx, C.byref(h)))
        self.h = h
        self.n_groups = 0

    def _chk(self, rc):
        if rc != 0:
            raise LmatError(rc, self.lib.lmat_bins_error(self.h).decode(errors="replace"))

    def set(self, groups, thresh, min_kmer):
        keep = []
        arr = (BinGroup * max(len(groups), 1))()
        for i, g in enumerate(groups):
            ids = np.ascontiguousarray(np.asarray(g[0], dtype=np.uint32))
            keep.append(ids)
            arr[i].ids = ids.ctypes.data if ids.size else None
            arr[i].n_ids = ids.size
            arr[i].flags = int(g[1]) if len(g) > 1 else 0
            arr[i].low_score = float(g[2]) if len(g) > 2 else 0.0
        self._chk(self.lib.lmat_bins_set(self.h, C.cast(arr, C.c_void_p), len(groups), float(thresh), int(min_kmer)))
        self.n_groups = len(groups)

    def set_file(self, idfile, thresh, min_kmer):
        """The script's id file: every non-blank line makes a group, in file order -> the first token of each (its file's suffix)."""
        self._chk(self.lib.lmat_bins_set_from_file(self.h, os.fsencode(idfile), float(thresh), int(min_kmer)))
        names = [l.split()[0] for l in open(idfile) if l.split()]
        self.n_groups = len(names)
        return names

    def run(self, reads, first=0, count=None, want_bases=True):
        """On the records of the most recent classify launch, which must have been for exactly reads[first : first + count]
        -> {group: (read indices into `reads` uint32[n] ascending, offsets uint64[n + 1], bases uint8 or None)}"""
        n = len(reads) - first if count is None else count
        self._chk(self.lib.lmat_bins_run(self.h, reads.h, first, n, 1 if want_bases else 0))
        nr, nb = self.counts()
        out = {}
        for g in range(self.n_groups):
            idx = np.zeros(max(int(nr[g]), 1), dtype=np.uint32)
            off = np.zeros(int(nr[g]) + 1, dtype=np.uint64)
            bases = np.zeros(max(int(nb[g]), 1), dtype=np.uint8) if want_bases else None
            self._chk(self.lib.lmat_bins_fetch(self.h, g, _ptr(idx), _ptr(off), _ptr(bases)))
            out[g] = (idx[:int(nr[g])], off, bases[:int(nb[g])] if want_bases else None)
        return out

    def counts(self):
        """-> (reads per group uint64[n_groups], bases per group uint64[n_groups]) of the last run"""
        nr = np.zeros(max(self.n_groups, 1), dtype=np.uint64)
        nb = np.zeros(max(self.n_groups, 1), dtype=np.uint64)
        self._chk(self.lib.lmat_bins_counts(self.h, _ptr(nr), _ptr(nb)))
        return nr[:self.n_groups], nb[:self.n_groups]

    def select_debug(self, results):
        """The select kernel alone on given records (READ_RESULT_DTYPE) -> group per record, uint16 (BIN_NONE: none)"""
        res = np.ascontiguousarray(results, dtype=READ_RESULT_DTYPE)
        out = np.full(max(res.size, 1), BIN_NONE, dtype=np.uint16)
        self._chk(self.lib.lmat_debug_bins_select(self.h, _ptr(res), res.size, _ptr(out)))
        return out[:res.size]

    def close(self):
        if self.h:
            self.lib.lmat_bins_destroy(self.h)
            self.h = None


class Builder:
    """lmat_build: genome FASTA + taxonomy tree -> k-mers with LCA-closed taxid lists, on the GPU of `eng`.
    genes=True (and no tree): the id-set mode -- gene FASTA -> k-mers with the ascending ids of the records that hold them."""

    def __init__(self, eng, k, tree=None, genes=False):
        self.eng, self.lib = eng, eng.lib
        h = C.c_void_p()
        if genes:
            if tree is not None:
                raise ValueError("an id-set builder takes no taxonomy tree")
            eng._chk(self.lib.lmat_genebuild_create(eng.ctx, k, C.byref(h)))
        else:
            eng._chk(self.lib.lmat_build_create(eng.ctx, k, tree.encode() if tree is not None else None, C.byref(h)))
        self.h = h
        self.stats = None

    def _chk(self, rc):
        if rc != 0:
            raise LmatError(rc, self.lib.lmat_build_error(self.h).decode(errors="replace"))

    def set_options(self, budget_bytes=0, prefix_bits=-1, chunk_bases=0):
        self._chk(self.lib.lmat_build_set_options(self.h, int(budget_bytes), int(prefix_bits), int(chunk_bases)))

    def add_fasta(self, fn):
        self._chk(self.lib.lmat_build_add_fasta(self.h, fn.encode()))

    def add_sequence(self, taxid, seq):
        bs = seq.encode() if isinstance(seq, str) else bytes(seq)
        self._chk(self.lib.lmat_build_add_sequence(self.h, int(taxid), bs, len(bs)))

    def add_taxhisto(self, fn):
        """An existing tax_histo file as a further input: run() gives the merge (lmat_build_add_taxhisto)."""
        self._chk(self.lib.lmat_build_add_taxhisto(self.h, fn.encode()))

    def add_db(self, engine):
        """The database `engine` holds as a further input: exported on the GPU now, merged like a file (lmat_build_add_db)."""
        self._chk(self.lib.lmat_build_add_db(self.h, engine.ctx))

    def run(self):
        st = BuildStats()
        self._chk(self.lib.lmat_build_run(self.h, C.byref(st)))
        self.stats = st.as_dict()
        return self.stats

    @property
    def merge_stats(self):
        """lmat_merge_stats of the last run (dict)."""
        ms = MergeStats()
        self._chk(self.lib.lmat_build_merge_stats(self.h, C.byref(ms)))
        return ms.as_dict()

    def taxid_counts(self):
        """-> (taxids uint32[n] ascending, counts uint64[n]): result records whose list holds each taxid."""
        n = C.c_uint64(0)
        rc = self.lib.lmat_build_taxid_counts(self.h, None, None, 0, C.byref(n))
        if rc != 0 and n.value == 0:
            self._chk(rc)
        tids = np.zeros(max(n.value, 1), dtype=np.uint32)
        cnts = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._chk(self.lib.lmat_build_taxid_counts(self.h, _ptr(tids), _ptr(cnts), n.value, C.byref(n)))
        return tids[:n.value], cnts[:n.value]

    def write_taxhisto(self, fn):
        self._chk(self.lib.lmat_build_write_taxhisto(self.h, fn.encode()))

    def fetch(self, first=0, count=None):
        """-> (kmers uint64[count], list_off uint64[count + 1], tids uint32[list_off[-1]])"""
        n = self.stats["records_written"] - first if count is None else count
        km = np.zeros(n, dtype=np.uint64)
        off = np.zeros(n + 1, dtype=np.uint64)
        self._chk(self.lib.lmat_build_fetch(self.h, first, n, _ptr(km), _ptr(off), None, 0))
        td = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        self._chk(self.lib.lmat_build_fetch(self.h, first, n, None, None, _ptr(td), td.size))
        return km, off, td[:int(off[-1])]

    def close(self):
        if self.h:
            self.lib.lmat_build_destroy(self.h)
            self.h = None


class Export:
    """lmat_export: the finalized database of `eng` back out as tax_histo records, on its GPU."""

    def __init__(self, eng):
        self.eng, self.lib = eng, eng.lib
        h = C.c_void_p()
        eng._chk(self.lib.lmat_export_create(eng.ctx, C.byref(h)))
        self.h = h
        self.stats = None

    def _chk(self, rc):
        if rc != 0:
            raise LmatError(rc, self.lib.lmat_export_error(self.h).decode(errors="replace"))

    def set_options(self, budget_bytes=0, prefix_bits=-1):
        self._chk(self.lib.lmat_export_set_options(self.h, int(budget_bytes), int(prefix_bits)))

    def set_filter(self, taxa=(), mode=None, min_lca_depth=0, max_entries=0):
        """The taxonomic slice (lmat_export_set_filter): S = the subtrees of `taxa`; mode "any" | "all" | "none" keeps a k-mer iff any /
        every / no entry of its stored list lies in S; min_lca_depth: every entry at least that deep in the tree; max_entries: lists of at
        most that many.  All enabled tests must pass.  Everything at its default clears the filter."""
        if mode is not None and mode not in SLICE_MODES:
            raise LmatError(-1, "filter mode must be None, 'any', 'all' or 'none', not %r" % (mode,))
        t = np.ascontiguousarray(np.asarray(list(taxa), dtype=np.uint32))
        f = ExportFilter(t.ctypes.data_as(C.POINTER(C.c_uint32)) if t.size else None, int(t.size), SLICE_MODES[mode] if mode else 0, int(min_lca_depth), int(max_entries))
        self._chk(self.lib.lmat_export_set_filter(self.h, C.byref(f)))

    def clear_filter(self):
        self._chk(self.lib.lmat_export_set_filter(self.h, None))

    def filter_stats(self):
        """-> {"scanned", "kept", "dropped_taxon", "dropped_depth", "dropped_length", "wave_lists", "ms_select"} of the last run"""
        out = (C.c_uint64 * 6)()
        ms = C.c_double(0)
        self._chk(self.lib.lmat_export_filter_stats(self.h, out, C.byref(ms)))
        return dict(zip(("scanned", "kept", "dropped_taxon", "dropped_depth", "dropped_length", "wave_lists"), (int(v) for v in out)), ms_select=ms.value)

    def into(self, dst, table_bytes=0):
        """Run with the filter and make the result the finalized database of the engine `dst` (lmat_db_from_export)."""
        self._chk(self.lib.lmat_db_from_export(dst.ctx, self.h, int(table_bytes)))

    def run(self, out=None):
        st = ExportStats()
        self._chk(self.lib.lmat_export_run(self.h, out.encode() if out is not None else None, C.byref(st)))
        self.stats = st.as_dict()
        return self.stats

    def fetch(self, first=0, count=None):
        """-> (kmers uint64[count], list_off uint64[count + 1], tids uint32[list_off[-1]])"""
        n = self.stats["records"] - first if count is None else count
        km = np.zeros(n, dtype=np.uint64)
        off = np.zeros(n + 1, dtype=np.uint64)
        self._chk(self.lib.lmat_export_fetch(self.h, first, n, _ptr(km), _ptr(off), None, 0))
        td = np.zeros(max(int(off[-1]), 1), dtype=np.uint32)
        self._chk(self.lib.lmat_export_fetch(self.h, first, n, None, None, _ptr(td), td.size))
        return km, off, td[:int(off[-1])]

    def taxid_counts(self):
        """-> (taxids uint32[n] ascending, counts uint64[n]): lists that hold each taxid"""
        n = C.c_uint64(0)
        rc = self.lib.lmat_export_taxid_counts(self.h, None, None, 0, C.byref(n))
        if rc != 0 and n.value == 0:
            self._chk(rc)
        tids = np.zeros(max(n.value, 1), dtype=np.uint32)
        cnts = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._chk(self.lib.lmat_export_taxid_counts(self.h, _ptr(tids), _ptr(cnts), n.value, C.byref(n)))
        return tids[:n.value], cnts[:n.value]

    def close(self):
        if self.h:
            self.lib.lmat_export_destroy(self.h)
            self.h = None


class Coverage:
    """lmat_cov: reads with a group id each -> per group and k the distinct canonical k-mers, the sum of their multiplicities
    (reads of the group that hold the k-mer) and the histogram of the multiplicities, on the GPU of `eng`."""

    def __init__(self, eng, k_sizes):
        self.eng, self.lib = eng, eng.lib
        self.k_sizes = [int(k) for k in k_sizes]
        ks = np.asarray(self.k_sizes, dtype=np.int32)
        h = C.c_void_p()
        eng._chk(self.lib.lmat_cov_create(eng.ctx, _ptr(ks) if ks.size else None, int(ks.size), C.byref(h)))
        self.h = h
        self.stats = None

    def _chk(self, rc):
        if rc != 0:
            raise LmatError(rc, self.lib.lmat_cov_error(self.h).decode(errors="replace"))

    def set_options(self, budget_bytes=0, prefix_bits=-1):
        self._chk(self.lib.lmat_cov_set_options(self.h, int(budget_bytes), int(prefix_bits)))

    def add_reads(self, reads, groups):
        """reads: byte strings (or str); groups: one 32-bit id per read."""
        bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
        off = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            np.cumsum([len(b) for b in bs], out=off[1:])
        blob = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8)
        g = np.ascontiguousarray(np.asarray(groups, dtype=np.uint32))
        if g.size != len(bs):
            raise ValueError("one group id per read")
        self._chk(self.lib.lmat_cov_add_reads(self.h, _ptr(blob), _ptr(off), len(bs), _ptr(g)))

    def run(self):
        st = CovStats()
        self._chk(self.lib.lmat_cov_run(self.h, C.byref(st)))
        self.stats = st.as_dict()
        return self.stats

    def summary(self, k_index):
        """-> (groups uint32[n] ascending, distinct uint64[n], total uint64[n])"""
        n = C.c_uint64(0)
        rc = self.lib.lmat_cov_summary(self.h, k_index, None, None, None, 0, C.byref(n))
        if rc != 0 and n.value == 0:
            self._chk(rc)
        g = np.zeros(max(n.value, 1), dtype=np.uint32)
        d = np.zeros(max(n.value, 1), dtype=np.uint64)
        t = np.zeros(max(n.value, 1), dtype=np.uint64)
        self._chk(self.lib.lmat_cov_summary(self.h, k_index, _ptr(g), _ptr(d), _ptr(t), n.value, C.byref(n)))
        return g[:n.value], d[:n.value], t[:n.value]

    def histogram(self, k_index, group):
        """-> [(multiplicity, n_kmers), ...] ascending; [] for a group the summary does not list"""
        n = C.c_uint64(0)
        rc = self.lib.lmat_cov_histogram(self.h, k_index, int(group), None, None, 0, C.byref(n))
        if rc != 0 and n.value == 0:
            self._chk(rc)
        if n.value == 0:
            return []
        m = np.zeros(n.value, dtype=np.uint64)
        c = np.zeros(n.value, dtype=np.uint64)
        self._chk(self.lib.lmat_cov_histogram(self.h, k_index, int(group), _ptr(m), _ptr(c), n.value, C.byref(n)))
        return [(int(a), int(b)) for a, b in zip(m[:n.value], c[:n.value])]

    def report(self):
        """-> {k_index: {group: (distinct, total, [(multiplicity, n_kmers), ...])}}"""
        out = {}
        for ki in range(len(self.k_sizes)):
            g, d, t = self.summary(ki)
            out[ki] = {int(a): (int(b), int(c), self.histogram(ki, int(a))) for a, b, c in zip(g, d, t)}
        return out

    def close(self):
        if self.h:
            self.lib.lmat_cov_destroy(self.h)
            self.h = None


class Engine:
    """One context on one GPU (lmat_ctx)."""

    def __init__(self, device=0, params: Params | None = None):
        self.lib = load_library()
        self.params = params or Params.run_rl()
        ctx = C.c_void_p()
        rc = self.lib.lmat_ctx_create(device, C.byref(self.params), C.byref(ctx))
        if rc != 0:
            raise LmatError(rc, "lmat_ctx_create failed (no usable HIP device?)")
        self.ctx = ctx

    def _chk(self, rc):
        if rc != 0:
            raise LmatError(rc, self.lib.lmat_last_error(self.ctx).decode(errors="replace"))

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.lmat_ctx_destroy(self.ctx)
            self.ctx = None

    def set_params(self, p: Params):
        self.params = p
        self._chk(self.lib.lmat_set_params(self.ctx, C.byref(p)))

    # taxonomy / DB --------------------------------------------------------------
    def load_taxonomy(self, tree, depth, rank, idmap, plasmids=None):
        e = lambda s: s.encode() if s else None
        self._chk(self.lib.lmat_taxonomy_load_files(self.ctx, e(tree), e(depth), e(rank), e(idmap), e(plasmids)))

    def build_gene_db(self, files, k=20, table_bytes=0, n_kmers_hint=0):
        """A gene database (gene_label): tax_histo-format files whose lists are 32-bit gene ids; no taxonomy needed."""
        self._chk(self.lib.lmat_genedb_begin(self.ctx, k, n_kmers_hint, table_bytes))
        for f in ([files] if isinstance(files, str) else files):
            self._chk(self.lib.lmat_db_add_taxhisto(self.ctx, f.encode()))
        self._chk(self.lib.lmat_db_finalize(self.ctx))

    def build_db(self, files, k=20, table_bytes=0, tid_cutoff=0, rank_map=None, human_kmers=None, adaptor_kmers=None,
                 save_image=None, n_kmers_hint=0):
        """make_db_table's job: tax_histo files (+ its -g/-m, -j, -u options) -> device table.
        With n_kmers_hint or table_bytes the table is sized up front and the files stream through the GPU insert
        kernel in chunks (nothing but the distinct lists stays on the host; save_image is then unavailable)."""
        e = lambda s: s.encode() if s else None
        self._chk(self.lib.lmat_db_begin(self.ctx, k, n_kmers_hint, table_bytes))
        if tid_cutoff or human_kmers or adaptor_kmers:
            self._chk(self.lib.lmat_db_set_build_options(self.ctx, tid_cutoff, e(rank_map), e(human_kmers), e(adaptor_kmers), 0))
        for f in ([files] if isinstance(files, str) else files):
            self._chk(self.lib.lmat_db_add_taxhisto(self.ctx, f.encode()))
        if save_image:
            self._chk(self.lib.lmat_db_save_image(self.ctx, save_image.encode()))
        self._chk(self.lib.lmat_db_finalize(self.ctx))

    # the database from genomes (lmat_build_*) ---------------------------------------
    def _builder(self, fastas, tree, k, budget_bytes=0, prefix_bits=-1, chunk_bases=0, taxhistos=(), genes=False):
        b = Builder(self, k, tree, genes=genes)
        try:
            b.set_options(budget_bytes, prefix_bits, chunk_bases)
            for f in ([fastas] if isinstance(fastas, str) else fastas or ()):
                b.add_fasta(f)
            for f in ([taxhistos] if isinstance(taxhistos, str) else taxhistos):
                b.add_taxhisto(f)
            b.run()
        except Exception:
            b.close()
            raise
        return b

    def build_taxhisto(self, fastas, tree, k, out, **opts):
        """kmerPrefixCounter + tax_histo: genome FASTA file(s) ('>' + taxid headers) and a taxonomy tree -> the tax_histo
        binary `out`.  opts: budget_bytes, prefix_bits, chunk_bases.  -> the build's statistics (dict)."""
        b = self._builder(fastas, tree, k, **opts)
        try:
            b.write_taxhisto(out)
            return b.stats
        finally:
            b.close()

    def merge_taxhisto(self, inputs, tree, k, out, fasta=None, **opts):
        """Existing tax_histo file(s) `inputs`, merged with each other and -- with `fasta` -- with the genomes of those FASTA
        file(s), into the tax_histo binary `out`: adding genomes to a database.  opts as build_taxhisto.
        -> the build's statistics (dict) with the merge's under "merge"."""
        b = self._builder(fasta, tree, k, taxhistos=inputs, **opts)
        try:
            b.write_taxhisto(out)
            return {**b.stats, "merge": b.merge_stats}
        finally:
            b.close()

    def build_db_from_genomes(self, fastas, tree, k=20, table_bytes=0, **opts):
        """The classify table straight from genome FASTA, no file in between (needs load_taxonomy first) -> statistics."""
        b = self._builder(fastas, tree, k, **opts)
        try:
            self._chk(self.lib.lmat_db_build_from_genomes(self.ctx, b.h, int(table_bytes)))
            return b.stats
        finally:
            b.close()

    # gene databases from gene FASTA: the builder's id-set mode (lmat_genebuild_create) ----------
    def build_gene_taxhisto(self, fastas, k, out, taxhistos=(), **opts):
        """Gene FASTA file(s) ('>' + gene id headers) and/or existing gene tax_histo files -> the gene database file `out`
        (what build_gene_db and gene_label -d read).  opts as build_taxhisto.  -> statistics (dict), the merge's under "merge"."""
        b = self._builder(fastas, None, k, taxhistos=taxhistos, genes=True, **opts)
        try:
            b.write_taxhisto(out)
            return {**b.stats, "merge": b.merge_stats}
        finally:
            b.close()

    def build_gene_db_from_genes(self, fastas, k=20, table_bytes=0, taxhistos=(), **opts):
        """The gene classify table straight from gene FASTA, no file in between and no taxonomy -> statistics."""
        b = self._builder(fastas, None, k, taxhistos=taxhistos, genes=True, **opts)
        try:
            self._chk(self.lib.lmat_genedb_build_from_genes(self.ctx, b.h, int(table_bytes)))
            return b.stats
        finally:
            b.close()

    # per-group k-mer coverage (lmat_cov_*) --------------------------------------------
    def kmer_coverage(self, reads, groups, k_sizes, budget_bytes=0, prefix_bits=-1):
        """content_summ's counting: -> ({k_index: {group: (distinct, total, [(multiplicity, n_kmers), ...])}}, statistics)."""
        c = Coverage(self, k_sizes)
        try:
            c.set_options(budget_bytes, prefix_bits)
            c.add_reads(reads, groups)
            st = c.run()
            return c.report(), st
        finally:
            c.close()

    # the database back out (lmat_export_*) ----------------------------------------------
    def export_taxhisto(self, out=None, budget_bytes=0, prefix_bits=-1, taxa=(), mode=None, min_lca_depth=0, max_entries=0):
        """The loaded database as tax_histo records, ascending, lists in stored order.  With `out` the file build_db reads is
        written and the statistics (dict) returned; with out=None -> (statistics, (kmers, list_off, tids)).
        taxa / mode / min_lca_depth / max_entries: a taxonomic slice (Export.set_filter); its counters come under "filter"."""
        x = Export(self)
        try:
            x.set_options(budget_bytes, prefix_bits)
            sliced = bool(len(taxa) or mode or min_lca_depth or max_entries)
            if sliced:
                x.set_filter(taxa, mode, min_lca_depth, max_entries)
            st = x.run(out)
            if sliced:
                st["filter"] = x.filter_stats()
            return st if out else (st, x.fetch())
        finally:
            x.close()

    def db_taxid_counts(self, budget_bytes=0, prefix_bits=-1, taxa=(), mode=None, min_lca_depth=0, max_entries=0):
        """frequency_counter on the loaded database: -> {"counts": {taxid: lists that hold it}, "total_tid": n, "singletons": n};
        with the filter keywords of export_taxhisto, on that slice of it."""
        x = Export(self)
        try:
            x.set_options(budget_bytes, prefix_bits)
            if len(taxa) or mode or min_lca_depth or max_entries:
                x.set_filter(taxa, mode, min_lca_depth, max_entries)
            st = x.run("")
            t, c = x.taxid_counts()
            return {"counts": {int(a): int(b) for a, b in zip(t, c)}, "total_tid": st["entries"], "singletons": st["singletons"]}
        finally:
            x.close()

    def derive_db(self, src_engine, table_bytes=0, budget_bytes=0, prefix_bits=-1, **filter):
        """This engine's database becomes a slice of the one `src_engine` holds (needs load_taxonomy first): the filter keywords of
        export_taxhisto select it, no file in between (lmat_db_from_export).  -> the export's statistics with the counters under "filter"."""
        x = Export(src_engine)
        try:
            x.set_options(budget_bytes, prefix_bits)
            x.set_filter(**filter)
            x.into(self, table_bytes)
            return {"filter": x.filter_stats()}
        finally:
            x.close()

    def load_image(self, path, table_bytes=0):
        self._chk(self.lib.lmat_db_load_image(self.ctx, path.encode(), table_bytes))
        self._chk(self.lib.lmat_db_finalize(self.ctx))

    def save_device_image(self, path):
        """The finalized database as it lies in HBM (LMATIMG2): load_image() of another context with the same taxonomy streams it back in."""
        self._chk(self.lib.lmat_db_save_image(self.ctx, path.encode()))

    def set_label_modes(self, permissive=False, tid_cutoff=0, rank_map=None):
        """-s / -g N -m ranks; call before build_db / load_image."""
        self._chk(self.lib.lmat_set_label_modes(self.ctx, int(permissive), tid_cutoff, rank_map.encode() if rank_map else None))

    # rand_read_label (null-model generation) -------------------------------------
    def rand_mode(self, on=True):
        self._chk(self.lib.lmat_rand_mode(self.ctx, int(on)))

    def rand_reset(self, n_buckets=10):
        self._chk(self.lib.lmat_rand_reset(self.ctx, n_buckets))
        self._rand_nb = n_buckets

    def rand_label(self, reads, gc_bucket, first=0, count=None):
        n = len(reads) - first if count is None else count
        gb = np.ascontiguousarray(gc_bucket, dtype=np.uint8)
        assert gb.size == n
        self._chk(self.lib.lmat_rand_label(self.ctx, reads.h, first, n, _ptr(gb)))

    def rand_table(self):
        """-> {taxid: ([max label_prob per bucket], [hit count per bucket])}"""
        n = C.c_uint32(0)
        self._chk(self.lib.lmat_rand_get(self.ctx, None, None, None, 0, C.byref(n)))
        rows, nb = int(n.value), self._rand_nb
        tid = np.zeros(max(rows, 1), dtype=np.uint32)
        mx = np.zeros((max(rows, 1), nb), dtype=np.float32)
        ct = np.zeros((max(rows, 1), nb), dtype=np.uint32)
        self._chk(self.lib.lmat_rand_get(self.ctx, _ptr(tid), _ptr(mx), _ptr(ct), rows, C.byref(n)))
        return {int(tid[i]): (mx[i].copy(), ct[i].copy()) for i in range(rows)}

    def load_null_models(self, list_fn):
        """-n: null-model list file (gz tables resolved against $LMAT_DIR like the reference)."""
        self._chk(self.lib.lmat_nullmodel_load(self.ctx, list_fn.encode()))

    def clear_null_models(self):
        self._chk(self.lib.lmat_nullmodel_clear(self.ctx))

    def synth_taxonomy(self, branching=(3, 4, 4, 4, 4, 3)):
        b = np.asarray(branching, dtype=np.uint32)
        self._chk(self.lib.lmat_synth_taxonomy(self.ctx, _ptr(b)))

    def synth_db(self, genome_len, k=20, seed=2002, table_bytes=0, genus_block_permille=100, list_replicas=1, conserved_permille=(0, 0, 0)):
        """Synthetic database on the device: a tenth of every genome is a block shared within its genus;
        conserved_permille: the heavy tail -- blocks shared by a whole family / phylum / superkingdom (lists of 69 / 277 / 1109 taxids)."""
        cp = np.asarray(conserved_permille, dtype=np.uint32)
        assert cp.size == 3
        self._chk(self.lib.lmat_synth_db_build3(self.ctx, k, int(genome_len), seed, int(table_bytes), genus_block_permille, list_replicas, _ptr(cp)))

    @property
    def k(self):
        return int(self.lib.lmat_db_kmer_length(self.ctx))

    @property
    def db_size(self):
        return int(self.lib.lmat_db_size(self.ctx))

    @property
    def n_lists(self):
        return int(self.lib.lmat_db_list_count(self.ctx))

    @property
    def arena_bytes(self):
        return int(self.lib.lmat_db_arena_bytes(self.ctx))

    @property
    def table_bytes(self):
        return int(self.lib.lmat_db_table_bytes(self.ctx))

    def lookup(self, kmers, stride=64):
        km = np.ascontiguousarray(kmers, dtype=np.uint64)
        counts = np.zeros(km.size, dtype=np.uint32)
        tids = np.zeros((km.size, stride), dtype=np.uint32)
        self._chk(self.lib.lmat_db_lookup(self.ctx, _ptr(km), km.size, _ptr(counts), _ptr(tids), stride))
        return counts, tids

    # reads ----------------------------------------------------------------------
    def upload_reads(self, seqs) -> Reads:
        """seqs: list of str/bytes, or (uint8 blob, uint64 offsets)."""
        if isinstance(seqs, tuple):
            blob, off = seqs
        else:
            bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
            off = np.zeros(len(bs) + 1, dtype=np.uint64)
            np.cumsum([len(b) for b in bs], out=off[1:])
            blob = np.frombuffer(b"".join(bs) + b"\0", dtype=np.uint8)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        h = C.c_void_p()
        self._chk(self.lib.lmat_reads_upload(self.ctx, _ptr(blob), _ptr(off), off.size - 1, C.byref(h)))
        return Reads(self, h)

    def upload_read_pairs(self, mates1, mates2) -> Reads:
        """Paired-end reads, each (uint8 blob, uint64 offsets): read i of the result is mate i of the first, an N, mate i of the
        second, joined on the device."""
        (blob1, off1), (blob2, off2) = mates1, mates2
        blob1, blob2 = np.ascontiguousarray(blob1, dtype=np.uint8), np.ascontiguousarray(blob2, dtype=np.uint8)
        off1, off2 = np.ascontiguousarray(off1, dtype=np.uint64), np.ascontiguousarray(off2, dtype=np.uint64)
        if off1.size != off2.size:
            raise ValueError("as many mates 1 as mates 2")
        h = C.c_void_p()
        self._chk(self.lib.lmat_reads_upload_pairs(self.ctx, _ptr(blob1), _ptr(off1), _ptr(blob2), _ptr(off2), off1.size - 1, C.byref(h)))
        return Reads(self, h)

    def synth_reads(self, n, lengths=(150,), seed=3003) -> Reads:
        ln = np.asarray(lengths, dtype=np.uint32)
        h = C.c_void_p()
        self._chk(self.lib.lmat_reads_synth(self.ctx, int(n), _ptr(ln), ln.size, seed, C.byref(h)))
        return Reads(self, h)

    # classify -------------------------------------------------------------------
    def classify(self, reads: Reads, first=0, count=None, want_cands=True, cand_cap=None):
        n = len(reads) - first if count is None else count
        res = np.zeros(n, dtype=READ_RESULT_DTYPE)
        ncand = C.c_uint64(0)
        if want_cands:
            cap = cand_cap or max(64 * n, 1024)
            cands = np.zeros(cap, dtype=CAND_DTYPE)
            self._chk(self.lib.lmat_classify(self.ctx, reads.h, first, n, _ptr(res), _ptr(cands), cap, C.byref(ncand)))
            return res, cands
        self._chk(self.lib.lmat_classify(self.ctx, reads.h, first, n, _ptr(res), None, 0, C.byref(ncand)))
        return res, None

    def classify_async(self, reads: Reads, first=0, count=None):
        n = len(reads) - first if count is None else count
        self._chk(self.lib.lmat_classify_async(self.ctx, reads.h, first, n))

    def classify_async_cands(self, reads: Reads, first=0, count=None, cand_cap=0):
        """As classify_async with the -p candidate pairs written to a device-side buffer of cand_cap pairs."""
        n = len(reads) - first if count is None else count
        self._chk(self.lib.lmat_classify_async_cands(self.ctx, reads.h, first, n, int(cand_cap)))

    def sync(self):
        ms, nl = C.c_float(0), C.c_uint64(0)
        self._chk(self.lib.lmat_sync(self.ctx, C.byref(ms), C.byref(nl)))
        return float(ms.value), int(nl.value)

    def last_timing(self):
        """-> (classify_kernel ms, k4_kernel + re-run ms, launches) of the launches the last sync() waited for."""
        a, b, n = C.c_float(0), C.c_float(0), C.c_uint64(0)
        self._chk(self.lib.lmat_last_timing(self.ctx, C.byref(a), C.byref(b), C.byref(n)))
        return float(a.value), float(b.value), int(n.value)

    def fetch_results(self, first, count):
        res = np.zeros(count, dtype=READ_RESULT_DTYPE)
        self._chk(self.lib.lmat_results_fetch(self.ctx, first, count, _ptr(res)))
        return res

    def gather_bench(self, n_probes, seed=1):
        """-> (ms, bytes) of a random 64-B bucket gather over the table (probe access shape)."""
        ms, b = C.c_float(0), C.c_uint64(0)
        self._chk(self.lib.lmat_gather_bench(self.ctx, int(n_probes), seed, C.byref(ms), C.byref(b)))
        return float(ms.value), int(b.value)

    def format_out(self, res, cands, reads_ascii=None, first_index=0):
        """.out text for these results; reads_ascii = (blob, off) to echo the read, else 'X' (-a)."""
        blob, off = reads_ascii if reads_ascii is not None else (None, None)
        need = self.lib.lmat_format_out(self.ctx, _ptr(res), res.size, _ptr(cands), _ptr(blob), _ptr(off),
                                        1 if blob is not None else 0, first_index, None, 0)
        buf = C.create_string_buffer(int(need) + 1)
        self.lib.lmat_format_out(self.ctx, _ptr(res), res.size, _ptr(cands), _ptr(blob), _ptr(off),
                                 1 if blob is not None else 0, first_index, buf, need + 1)
        return buf.raw[:need].decode()

    # tallies ----------------------------------------------------------------------
    def counts_reset(self):
        self._chk(self.lib.lmat_counts_reset(self.ctx))

    def counts_layout(self):
        n, b = C.c_uint32(0), C.c_uint64(0)
        self._chk(self.lib.lmat_counts_layout(self.ctx, C.byref(n), C.byref(b)))
        return int(n.value), int(b.value)

    def counts_device_ptr(self):
        return int(self.lib.lmat_counts_device_ptr(self.ctx) or 0)

    # tallies across ranks: RCCL inside the engine (collective.cpp) ---------------------
    @staticmethod
    def comm_available() -> bool:
        """librccl and the entry points the engine uses load in this process (pre-flight before any rank enters comm_init)."""
        return bool(load_library().lmat_comm_available())

    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId: 128 bytes made by one rank and handed to the others by the launcher's own channel."""
        buf = C.create_string_buffer(128)
        rc = load_library().lmat_comm_unique_id(buf)
        if rc != 0:
            raise LmatError(rc, "cannot open librccl / make a communicator id")
        return buf.raw

    def comm_init(self, uid: bytes, n_ranks: int, rank: int):
        assert len(uid) == 128
        self._chk(self.lib.lmat_comm_init(self.ctx, C.c_char_p(uid), n_ranks, rank))

    def comm_allreduce_counts(self):
        """The merge of read_label.cpp:1760-1800 across ranks: every rank's tallies become the sum of all."""
        self._chk(self.lib.lmat_comm_allreduce_counts(self.ctx))

    def synth_window(self, species, pos):
        """-> (canonical k-mer, [taxid32...]) the synthetic database must hold for that ancestor window (host-derived)."""
        km, n = C.c_uint64(0), C.c_uint32(0)
        t = np.zeros(32, dtype=np.uint32)
        self._chk(self.lib.lmat_synth_window(self.ctx, species, int(pos), C.byref(km), _ptr(t), 32, C.byref(n)))
        return int(km.value), t[:n.value].tolist()

    def last_counters(self):
        """Reads the last launch passed from class to class (after sync()): fast -> E=512 -> middle tier -> large LDS -> global memory."""
        out = np.zeros(16, dtype=np.uint32)
        self._chk(self.lib.lmat_debug_last_counters(self.ctx, _ptr(out)))
        return {"past_fast": int(out[2]), "past_e512": int(out[3]), "past_middle": int(out[10]), "past_large": int(out[7])}

    def closure_stride_taken(self):
        """-> reads of the last launch whose closure walked its chains at a fixed stride (kernels.hip classify_one).  Counted only by
        launches made under LMAT_CLOSURE_STRIDE=2, which run the generic kernel; 0 otherwise."""
        out = np.zeros(16, dtype=np.uint32)
        self._chk(self.lib.lmat_debug_last_counters(self.ctx, _ptr(out)))
        return int(out[12])

    def variant_launches(self):
        """-> launches of the 160-k-mer fast class on this engine's device so far, by kernel: {"generic": n, "plain": n} (LMAT_PLAIN)."""
        out = np.zeros(2, dtype=np.uint64)
        self._chk(self.lib.lmat_debug_variant_launches(self.ctx, _ptr(out)))
        return {"generic": int(out[0]), "plain": int(out[1])}

    def uniform_launches(self):
        """-> how many of the "plain" launches of variant_launches() ran as the fixed-geometry variant: every read of the set of
        148 .. 151 bases at k = 20 (LMAT_UNIFORM)."""
        out = np.zeros(1, dtype=np.uint64)
        self._chk(self.lib.lmat_debug_uniform_launches(self.ctx, _ptr(out)))
        return int(out[0])

    def classify_grid(self):
        """-> the grid of the last launch that variant_launches() counted (0: none yet): wave b of it classified reads b, b + grid,
        b + 2 grid, ... of the launch."""
        out = np.zeros(1, dtype=np.uint32)
        self._chk(self.lib.lmat_debug_classify_grid(self.ctx, _ptr(out)))
        return int(out[0])

    def div_check(self):
        """-> (pairs whose fast quotient differs from the IEEE one, pairs tried, the same two for 2^26 drawn (float, 1..64) pairs): the
        divisions of the decision step on the wave."""
        out = np.zeros(4, dtype=np.uint64)
        self._chk(self.lib.lmat_debug_div_check(self.ctx, _ptr(out)))
        return tuple(int(x) for x in out)

    def probe_stats(self, kmers):
        """-> dict: where the lookups of these k-mers end (home bucket / absent at once / overflow hit / overflow miss, overflow buckets read)."""
        km = np.ascontiguousarray(kmers, dtype=np.uint64)
        out = np.zeros(5, dtype=np.uint64)
        self._chk(self.lib.lmat_debug_probe_stats(self.ctx, _ptr(km), km.size, _ptr(out)))
        return dict(zip(("home_hit", "absent_one_request", "overflow_hit", "overflow_miss", "overflow_buckets_read"), (int(x) for x in out)))

    def synth_read_windows(self, lengths, seed, r, cap=512, stride=32):
        """-> (kmers uint64[n], counts uint32[n], tids uint32[n, stride]) read r of synth_reads(lengths, seed) must find (host-derived)."""
        ln = np.asarray(lengths, dtype=np.uint32)
        km = np.zeros(cap, dtype=np.uint64)
        ct = np.zeros(cap, dtype=np.uint32)
        td = np.zeros((cap, stride), dtype=np.uint32)
        n, rl = C.c_uint32(0), C.c_uint32(0)
        self._chk(self.lib.lmat_synth_read_windows(self.ctx, _ptr(ln), ln.size, seed, int(r), _ptr(km), _ptr(td), _ptr(ct), cap, stride,
                                                   C.byref(n), C.byref(rl)))
        return km[:n.value], ct[:n.value], td[:n.value]

    def debug_decide(self, tables, stdevs):
        """tables: list of [(taxid32, score), ...]; stdevs: one per table -> results array (call_tid, call_score, match_type)."""
        off = np.zeros(len(tables) + 1, dtype=np.uint64)
        np.cumsum([len(t) for t in tables], out=off[1:])
        tids = np.array([t for tb in tables for t, _ in tb], dtype=np.uint32)
        sc = np.array([s for tb in tables for _, s in tb], dtype=np.float32)
        sd = np.ascontiguousarray(stdevs, dtype=np.float32)
        res = np.zeros(len(tables), dtype=READ_RESULT_DTYPE)
        self._chk(self.lib.lmat_debug_decide(self.ctx, _ptr(tids), _ptr(sc), _ptr(off), _ptr(sd), len(tables), _ptr(res)))
        return res

    def debug_decide_counts(self, tids, counts, off, cand, on_the_wave):
        """tids / counts: flat uint32 arrays, off: uint64[n + 1], cand: uint32[n] -> results array of the chosen decision path."""
        tids = np.ascontiguousarray(tids, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        cand = np.ascontiguousarray(cand, dtype=np.uint32)
        res = np.zeros(cand.size, dtype=READ_RESULT_DTYPE)
        self._chk(self.lib.lmat_debug_decide_counts(self.ctx, _ptr(tids), _ptr(counts), _ptr(off), _ptr(cand), cand.size, int(on_the_wave), _ptr(res)))
        return res

    def debug_decide_chain(self, tids, counts, off, cand, kept, eligible, with_cands=False):
        """debug_decide_counts on the wave for tables shaped as a closure with one eligible id leaves them: kept[i] slots the lists
        kept, eligible[i] the one whose ancestors fill the rest -> (results, took): took[i] = 1 where the closed form decided table i."""
        tids = np.ascontiguousarray(tids, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        cand = np.ascontiguousarray(cand, dtype=np.uint32)
        kept = np.ascontiguousarray(kept, dtype=np.uint32)
        eligible = np.ascontiguousarray(eligible, dtype=np.uint32)
        assert kept.size == cand.size and eligible.size == cand.size and off.size == cand.size + 1
        res = np.zeros(cand.size, dtype=READ_RESULT_DTYPE)
        took = np.zeros(cand.size, dtype=np.uint8)
        self._chk(self.lib.lmat_debug_decide_chain(self.ctx, _ptr(tids), _ptr(counts), _ptr(off), _ptr(cand), _ptr(kept), _ptr(eligible),
                                                   cand.size, int(with_cands), _ptr(res), _ptr(took)))
        return res, took

    def debug_decide_shape(self, tids, counts, off, cand, shape, with_cands=False):
        """debug_decide_counts on the wave with the closure's word per table as the classify kernel forms it: shape[i] = kept << 8 |
        1 << 17 (the closure finished), | eligible | 1 << 16 (it found one eligible id and registered its chain), or 0 -> (results,
        took): took[i] = 0 where the general code decided table i, 1 the closed form for one lineage, 2 the one for a dominant lineage,
        3 the one for tied ids at the top (offered by | 1 << 18 beside bit 17)."""
        tids = np.ascontiguousarray(tids, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        cand = np.ascontiguousarray(cand, dtype=np.uint32)
        shape = np.ascontiguousarray(shape, dtype=np.uint32)
        assert shape.size == cand.size and off.size == cand.size + 1
        res = np.zeros(cand.size, dtype=READ_RESULT_DTYPE)
        took = np.zeros(cand.size, dtype=np.uint8)
        self._chk(self.lib.lmat_debug_decide_shape(self.ctx, _ptr(tids), _ptr(counts), _ptr(off), _ptr(cand), _ptr(shape), cand.size,
                                                   int(with_cands), _ptr(res), _ptr(took)))
        return res, took

    def clone_db_from(self, src: "Engine"):
        self._chk(self.lib.lmat_db_clone(self.ctx, src.ctx))

    def counts(self):
        n, _ = self.counts_layout()
        tid = np.zeros(n, dtype=np.uint32)
        cnt = np.zeros(n, dtype=np.uint64)
        sc = np.zeros(n, dtype=np.float64)
        nz = C.c_uint32(0)
        nm = np.zeros(3, dtype=np.uint64)
        self._chk(self.lib.lmat_counts_get(self.ctx, _ptr(tid), _ptr(cnt), _ptr(sc), n, C.byref(nz), _ptr(nm)))
        k = int(nz.value)
        return {int(t): (int(c), float(s)) for t, c, s in zip(tid[:k], cnt[:k], sc[:k])}, [int(x) for x in nm]
