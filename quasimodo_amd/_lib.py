"""ctypes loader for libqmvt.so (built in-tree by quasimodo_amd/csrc/Makefile)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_SO = os.environ.get("QM_LIBQMVT") or os.path.join(_CSRC, "libqmvt.so")   # override only for A/B builds of the kernels

QM_N_SCALARS = 8
SCALAR_NAMES = ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R", "sorted", "n_records", "truth_unique")
ERRORS = {-1: "QM_E_INVAL", -2: "QM_E_NODEVICE", -3: "QM_E_HIP", -4: "QM_E_NOMEM", -5: "QM_E_RANGE",
          -6: "QM_E_STATE", -7: "QM_E_IO", -8: "QM_E_NONCANON", -9: "QM_E_LIMIT", -10: "QM_E_UNSORTED", -11: "QM_E_COMM"}
QM_E_UNSORTED = -10
QM_BATCH_ALLELES = 1
QM_ABI_VERSION = 6
QM_N_MOTIFS = 96
QM_MOTIF_OTHER = 96
QM_MOTIF_REF_MISMATCH = 97
QM_MOTIF_COLS = 98
QM_TRUTH_GROUP_MAX = 5
QM_TRUTH_REGIONS = 32
QM_AFP_NO_AF = 0
QM_AFP_OUTSIDE = 1
QM_AFP_N_GRID = 2
QM_AFP_EXTRA = 3
QM_AFP_MAX_CELLS = 8192
QM_STRATA_MAX = 32
QM_STRATA_LDS_SEGMENTS = 4096
QM_STRATA_MAX_SEGMENTS = 1 << 22
QM_STRATA_RECORDS = 1
QM_STRATA_TRUTH = 2
QM_BOOT_MAX_WINDOWS = 4096
QM_BOOT_MAX_REP = 16384
QM_BOOT_RECORDS = 1
QM_BOOT_TRUTH = 2
QM_VOTE_GROUP_MAX = 32
QM_VOTE_SLOTS = 33
QM_NM_MAX_RADIUS = 64
QM_NM_R_CLASSES = 6
QM_NM_T_CLASSES = 5
QM_NM_NONE = 255
QM_SF_MAX_QUAL_BINS = 256
QM_SF_MAX_AF_BINS = 64
QM_SF_MAX_CELLS = 4096
QM_SF_MAX_QUAL_STEP = 65536
QM_SF_TP, QM_SF_FP, QM_SF_U = 0, 1, 2
QM_SF_COUNTED, QM_SF_NO_AF, QM_SF_NO_BIN, QM_SF_TRUTH = 0, 1, 2, 3
QM_SF_EXTRA = 4
QM_CX_MAX_HALF_WINDOW = 1024
QM_CX_MAX_GC_BINS = 15
QM_CX_NONE = 255
QM_CX_RECORDS = 1
QM_CX_TRUTH = 2
QM_NORM_R_COLS = 12
QM_NORM_T_COLS = 5
QM_NORM_COLUMNS = 2
QM_ATOM_R_COLS = 13
QM_ATOM_T_COLS = 6
QM_ATOM_COLUMNS = 2
QM_TYPE_MAX_BINS = 16
QM_TYPE_MAX_ROWS = 84
QM_TYPE_COLUMNS = 2
QM_TYPE_SNV, QM_TYPE_MNP, QM_TYPE_INS, QM_TYPE_DEL, QM_TYPE_CPX = range(5)
QM_TYPE_X_NOKEY, QM_TYPE_X_NOVAR, QM_TYPE_X_LONGPAIR, QM_TYPE_X_NOSHAPE = range(4)
QM_HAP_R_COLS = 16
QM_HAP_T_COLS = 8
QM_HAP_MAX_GAP = 32
QM_HAP_DEFAULT_GAP = 10
QM_HAP_MAX_WINDOW = 256
QM_HAP_MAX_ITEMS = 8
QM_HAP_COLUMNS = 2
QM_HAPSUB_COLS = 8
QM_HAPSUB_COLUMNS = 2
QM_HAPSUB_NARROW_HASH = 4
QM_RROC_NORM = 1
QM_RROC_ATOM = 2
QM_LADDER_SUBSETS = 1
QM_LADDER_COLUMNS = 2
QM_LADDER_COLS = 18

# every symbol include/qmvt.h declares
EXPORTS = (
    "qm_abi_version", "qm_kernels_id", "qm_build_id", "qm_init", "qm_destroy", "qm_last_error", "qm_truth_load", "qm_truth_size", "qm_truth_count",
    "qm_classify_batch", "qm_batch_create", "qm_batch_destroy", "qm_batch_upload", "qm_truth_synth", "qm_batch_synth",
    "qm_batch_run", "qm_batch_finish", "qm_batch_set_timing", "qm_batch_timings", "qm_batch_get_cls", "qm_batch_get_idx",
    "qm_batch_get_roc", "qm_batch_get_scalars", "qm_batch_get_global", "qm_batch_get_columns", "qm_batch_device_bytes",
    "qm_fp_overlap", "qm_vcf_count_lines", "qm_vcf_scan", "qm_truth_scan", "qm_vcf_write", "qm_vcf_split_write",
    "qm_truth_size_ext", "qm_truth_synth_ext", "qm_batch_create_ext", "qm_classify_batch_ext",
    "qm_dict_create", "qm_dict_destroy", "qm_dict_size", "qm_allele_code", "qm_allele_spell", "qm_vcf_scan_ext", "qm_truth_scan_ext",
    "qm_bench_synth", "qm_truth_release", "qm_batch_n_truth",
    "qm_bw_probe", "qm_bgzf_write", "qm_bgzf_write_tbi", "qm_extract_files", "qm_extract_files_ex", "qm_batch_global_device", "qm_batch_path_stats", "qm_path_stats_total", "qm_batch_upload_async", "qm_batch_get_masks", "qm_patterns_create", "qm_patterns_destroy", "qm_patterns_info", "qm_vcf_hostpath",
    "qm_mummer2vcf", "qm_free",
    "qm_comm_create", "qm_comm_make_id", "qm_comm_create_rank", "qm_allreduce_counters", "qm_comm_collectives", "qm_comm_destroy",
    "qm_genome_load", "qm_genome_release", "qm_batch_motifs", "qm_batch_get_motifs", "qm_extract_files_motifs",
    "qm_batch_truth_hits", "qm_batch_get_truth_hits", "qm_batch_get_intruth_mask", "qm_batch_truth_regions", "qm_extract_files_truthside",
    "qm_vcf_scan_af", "qm_batch_upload_af", "qm_batch_af_profile", "qm_batch_get_af_profile", "qm_extract_files_profile",
    "qm_strata_load", "qm_strata_info", "qm_strata_segments", "qm_strata_release", "qm_batch_strata", "qm_batch_get_strata",
    "qm_extract_files_strata",
    "qm_batch_boot", "qm_batch_get_boot", "qm_boot_draws", "qm_extract_files_boot",
    "qm_batch_votes", "qm_batch_get_votes", "qm_batch_get_vote_keys", "qm_batch_vote_groups", "qm_batch_vote_timings", "qm_extract_files_votes",
    "qm_batch_nearmiss", "qm_batch_get_nearmiss", "qm_batch_get_nearmiss_cls", "qm_batch_get_nearmiss_truth", "qm_batch_nearmiss_timings", "qm_extract_files_nearmiss",
    "qm_batch_surface", "qm_batch_get_surface", "qm_batch_surface_timings", "qm_extract_files_surface",
    "qm_genome_context", "qm_batch_context", "qm_batch_get_context", "qm_batch_context_timings",
    "qm_extract_files_context",
    "qm_batch_normalize", "qm_batch_get_normalize", "qm_batch_get_normalized", "qm_batch_normalize_timings", "qm_truth_normalized", "qm_truth_entries", "qm_extract_files_normalize",
    "qm_batch_atomize", "qm_batch_get_atomize", "qm_batch_get_atomized", "qm_batch_atomize_timings", "qm_truth_atoms", "qm_extract_files_atomize",
    "qm_dict_shapes", "qm_batch_types", "qm_batch_get_types", "qm_batch_get_typed", "qm_batch_types_timings", "qm_extract_files_types",
    "qm_batch_haplotypes", "qm_batch_get_haplotypes", "qm_batch_get_haplotyped", "qm_batch_haplotype_timings", "qm_truth_sites", "qm_extract_files_haplotypes",
    "qm_batch_hapsubsets", "qm_batch_get_hapsubsets", "qm_batch_get_hapsubsetted", "qm_batch_hapsubset_timings",
    "qm_extract_files_hapsubsets",
    "qm_batch_rescue_roc", "qm_batch_get_rescue_roc", "qm_batch_rescue_roc_timings", "qm_extract_files_rescue_roc",
    "qm_batch_ladder", "qm_batch_get_ladder", "qm_batch_get_laddered", "qm_batch_ladder_timings", "qm_extract_files_ladder",
    "qm_batch_ladder_types", "qm_batch_get_ladder_types", "qm_batch_ladder_types_timings", "qm_extract_files_ladder_types",
)


class BenchResult(C.Structure):
    _fields_ = [("records", C.c_int64), ("seconds_per_step", C.c_double), ("classifications_per_s", C.c_double),
                ("classify_ms", C.c_float), ("finalize_ms", C.c_float), ("compact_ms", C.c_float), ("reserved", C.c_int32),
                ("kept", C.c_int64), ("tp_lines", C.c_int64), ("fp_lines", C.c_int64), ("device_bytes", C.c_int64)]


class QmvtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "QM_E_?"), code, message))
        self.code = code


class SynthCfg(C.Structure):
    _fields_ = [("genome_len", C.c_int64), ("seed", C.c_uint64), ("truth_seed", C.c_uint64), ("truth_n", C.c_int64),
                ("shuffled", C.c_int32), ("indel_pct", C.c_int32)]


class TruthSideArgs(C.Structure):
    """include/qmvt.h qm_truthside_args"""
    _fields_ = [("fn_out", C.POINTER(C.c_char_p)), ("group", C.c_void_p), ("n_groups", C.c_int32), ("reserved", C.c_int32),
                ("regions", C.c_void_p), ("fp_regions", C.c_void_p), ("missed_out", C.POINTER(C.c_char_p))]


class ProfileArgs(C.Structure):
    """include/qmvt.h qm_profile_args"""
    _fields_ = [("want", C.c_void_p), ("window", C.c_int32), ("n_pos_bins", C.c_int32), ("n_af_bins", C.c_int32), ("reserved", C.c_int32),
                ("grid", C.c_void_p), ("extra", C.c_void_p), ("points_out", C.POINTER(C.c_char_p))]


class StrataArgs(C.Structure):
    """include/qmvt.h qm_strata_args"""
    _fields_ = [("strata_id", C.c_int32), ("reserved", C.c_int32), ("want", C.c_void_p), ("rec", C.c_void_p), ("tru", C.c_void_p)]


class BootArgs(C.Structure):
    """include/qmvt.h qm_boot_args"""
    _fields_ = [("window", C.c_int32), ("n_win", C.c_int32), ("n_rep", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64),
                ("want", C.c_void_p), ("cnt", C.c_void_p), ("rep", C.c_void_p)]


class VotesArgs(C.Structure):
    """include/qmvt.h qm_votes_args"""
    _fields_ = [("group", C.c_void_p), ("n_groups", C.c_int32), ("reserved", C.c_int32), ("tp_votes", C.c_void_p), ("fp_votes", C.c_void_p),
                ("private_tp", C.c_void_p), ("private_fp", C.c_void_p), ("consensus_k", C.c_void_p), ("consensus_out", C.POINTER(C.c_char_p))]


class NearmissArgs(C.Structure):
    """include/qmvt.h qm_nearmiss_args"""
    _fields_ = [("want", C.c_void_p), ("radius", C.c_int32), ("reserved", C.c_int32), ("rec", C.c_void_p), ("tru", C.c_void_p),
                ("fp_why_out", C.POINTER(C.c_char_p)), ("fn_why_out", C.POINTER(C.c_char_p))]


class SurfaceArgs(C.Structure):
    """include/qmvt.h qm_surface_args"""
    _fields_ = [("want", C.c_void_p), ("q_step", C.c_int32), ("nq", C.c_int32), ("na", C.c_int32), ("reserved", C.c_int32),
                ("S", C.c_void_p), ("extra", C.c_void_p)]


class NormalizeArgs(C.Structure):
    """include/qmvt.h qm_normalize_args"""
    _fields_ = [("genome_id", C.c_void_p), ("rec", C.c_void_p), ("tru", C.c_void_p), ("rescued_out", C.POINTER(C.c_char_p))]


class AtomizeArgs(C.Structure):
    """include/qmvt.h qm_atomize_args"""
    _fields_ = [("want", C.c_void_p), ("rec", C.c_void_p), ("tru", C.c_void_p), ("atoms_out", C.POINTER(C.c_char_p))]


class HapsubArgs(C.Structure):
    """include/qmvt.h qm_hapsub_args"""
    _fields_ = [("genome_id", C.c_void_p), ("gap", C.c_int32), ("reserved", C.c_int32), ("rec", C.c_void_p), ("tru", C.c_void_p),
                ("sites_out", C.POINTER(C.c_char_p)), ("genome_seq", C.POINTER(C.c_char_p)), ("genome_len", C.c_void_p),
                ("sub", C.c_void_p), ("subsets_out", C.POINTER(C.c_char_p))]


class RescueRocArgs(C.Structure):
    """include/qmvt.h qm_rescue_roc_args"""
    _fields_ = [("genome_id", C.c_void_p), ("want", C.c_void_p), ("roc_n", C.c_void_p), ("roc_a", C.c_void_p), ("base", C.c_void_p)]


class LadderArgs(C.Structure):
    """include/qmvt.h qm_ladder_args"""
    _fields_ = [("genome_id", C.c_void_p), ("gap", C.c_int32), ("subsets", C.c_int32), ("want", C.c_void_p), ("rec", C.c_void_p),
                ("tru", C.c_void_p), ("ladder_out", C.POINTER(C.c_char_p))]


class LadderTypesArgs(C.Structure):
    """include/qmvt.h qm_ladder_types_args"""
    _fields_ = [("genome_id", C.c_void_p), ("gap", C.c_int32), ("subsets", C.c_int32), ("want", C.c_void_p), ("edges", C.c_void_p),
                ("n_bins", C.c_int32), ("reserved", C.c_int32), ("rec", C.c_void_p), ("tru", C.c_void_p)]


class HaplotypesArgs(C.Structure):
    """include/qmvt.h qm_haplotypes_args"""
    _fields_ = [("genome_id", C.c_void_p), ("gap", C.c_int32), ("reserved", C.c_int32), ("rec", C.c_void_p), ("tru", C.c_void_p),
                ("sites_out", C.POINTER(C.c_char_p)), ("genome_seq", C.POINTER(C.c_char_p)), ("genome_len", C.c_void_p)]


class TypesArgs(C.Structure):
    """include/qmvt.h qm_types_args"""
    _fields_ = [("edges", C.c_void_p), ("n_bins", C.c_int32), ("reserved", C.c_int32), ("want", C.c_void_p), ("rec", C.c_void_p), ("tru", C.c_void_p)]


class ContextArgs(C.Structure):
    """include/qmvt.h qm_context_args"""
    _fields_ = [("w", C.c_int32), ("ng", C.c_int32), ("genome_id", C.c_void_p), ("rec", C.c_void_p), ("tru", C.c_void_p), ("gen", C.c_void_p)]


class FileJob(C.Structure):
    _fields_ = [("vcf_path", C.c_char_p), ("truth_path", C.c_char_p), ("mode", C.c_int32), ("pure", C.c_int32),
                ("filtered_out", C.c_char_p), ("tp_out", C.c_char_p), ("fp_out", C.c_char_p)]


class FileStats(C.Structure):
    _fields_ = [("scalars", C.c_int64 * QM_N_SCALARS), ("n_lines", C.c_int64), ("n_refused", C.c_int64), ("genomediff", C.c_int64),
                ("header_kept", C.c_int64), ("header_kept_tp", C.c_int64), ("host_decided", C.c_int64), ("r_hostile", C.c_int64)]


class VcfCols(C.Structure):
    _fields_ = [("n_lines", C.c_int64), ("n_data", C.c_int64), ("n_host", C.c_int64), ("n_refused", C.c_int64),
                ("first_refused_line", C.c_int64), ("n_nokey_kept", C.c_int64), ("n_r_hostile", C.c_int64), ("first_r_hostile_line", C.c_int64)]


def library_path():
    return _SO


_KSRC = ("qmvt_kernels.hip", "qmvt_dev.h")
_ASRC = _KSRC + ("qmvt_walk.h", "qmvt_classify_pair.hip", "qmvt_classify_pair.h", "qmvt_motif.hip", "qmvt_motif.h", "qmvt_truthside.hip", "qmvt_truthside.h", "qmvt_afprofile.hip", "qmvt_afprofile.h", "qmvt_strata.hip", "qmvt_strata.h", "qmvt_boot.hip", "qmvt_boot.h", "qmvt_votes.hip", "qmvt_votes.h", "qmvt_nearmiss.hip", "qmvt_nearmiss.h", "qmvt_surface.hip", "qmvt_surface.h", "qmvt_context.hip", "qmvt_context.h", "qmvt_norm.hip", "qmvt_norm.h", "qmvt_atom.hip", "qmvt_atom.h", "qmvt_types.hip", "qmvt_types.h", "qmvt_haplo.hip", "qmvt_haplo.h", "qmvt_rroc.hip", "qmvt_rroc.h", "qmvt_ladder.hip", "qmvt_ladder.h", "qmvt_ltypes.hip", "qmvt_ltypes.h", "qmvt_batch.h", "qmvt_api.cpp", "qmvt_finish.cpp", "qmvt_comm.cpp", "qmvt_host.cpp", "qmvt_pipeline.cpp", os.path.join("..", "..", "include", "qmvt.h"), "Makefile")


def _sha16(files):
    import hashlib
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(_CSRC, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def source_kernels_id():
    """sha256 (first 16 hex digits) of the device code's SOURCES in the tree (the Makefile compiles the same figure in)."""
    return _sha16(_KSRC)


def source_build_id():
    """The same over every source of the library."""
    return _sha16(_ASRC)


def embedded_ids(path=None):
    """(kernels id, build id) compiled into a libqmvt.so, read from the file without loading it; (None, None) when the file
    or the marker is missing."""
    import re
    try:
        with open(path or _SO, "rb") as fh:
            m = re.search(rb"@\(#\)qmvt-ids kernels=([0-9a-z]+) build=([0-9a-z]+);", fh.read())
    except OSError:
        return None, None
    return (m.group(1).decode(), m.group(2).decode()) if m else (None, None)


def kernel_source_id():
    """The id of the device code of the LOADED library (qm_kernels_id: compiled in at build time): what a profile of the
    kernels belongs to.  profiles/traffic.json carries the id of the build its PMC passes ran on; bench.py quotes that
    traffic only for the same id.  "unknown" for builds that did not go through the Makefile (QM_LIBQMVT A/B builds)."""
    L = lib()
    return L.qm_kernels_id().decode()


def build_library(force=False):
    """Compile libqmvt.so for gfx950 with hipcc (cross-compiles without a GPU).  Rebuilt whenever the ids compiled into the
    binary differ from the sources in the tree (content, not time stamps: a stale binary that travelled with the tree is
    replaced), when it is missing, or on request."""
    default = os.path.join(_CSRC, "libqmvt.so")
    stale = force or not os.path.exists(default) or embedded_ids(default) != (source_kernels_id(), source_build_id())
    if stale:
        if _lib is not None and _SO == default:
            raise QmvtError(-6, "libqmvt.so is stale but already loaded in this process; rebuild before importing the engine")
        subprocess.check_call(["make", "-s", "-C", _CSRC, "libqmvt.so"])
        if embedded_ids(default) != (source_kernels_id(), source_build_id()):
            raise QmvtError(-7, "libqmvt.so does not carry the ids of the sources it was just built from")
    return _SO


_lib = None


def lib():
    """The loaded library.  Missing .so is a hard error: there is no Python/CPU substitute."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise QmvtError(-2, "libqmvt.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "or `make -C quasimodo_amd/csrc`" % _SO)
    L = C.CDLL(_SO)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.qm_abi_version.restype = i32
    L.qm_kernels_id.restype = C.c_char_p
    L.qm_build_id.restype = C.c_char_p
    L.qm_last_error.restype = C.c_char_p
    L.qm_last_error.argtypes = [vp]
    L.qm_init.argtypes = [i32, C.POINTER(vp)]
    L.qm_destroy.argtypes = [vp]
    L.qm_destroy.restype = None
    L.qm_truth_load.argtypes = [vp, vp, vp, vp, i64, C.POINTER(i32)]
    L.qm_truth_synth.argtypes = [vp, i64, i64, C.c_uint64, C.POINTER(i32)]
    L.qm_truth_size.argtypes = [vp, i32, C.POINTER(i64)]
    L.qm_truth_size_ext.argtypes = [vp, i32, C.POINTER(i64)]
    L.qm_truth_synth_ext.argtypes = [vp, i64, i64, C.c_uint64, i32, C.POINTER(i32)]
    L.qm_batch_create_ext.argtypes = [vp, i32, vp, vp, i32, C.c_uint, C.POINTER(vp)]
    L.qm_classify_batch_ext.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, C.c_uint, vp, vp, vp, vp, vp]
    L.qm_truth_count.argtypes = [vp]
    L.qm_truth_release.argtypes = [vp, i32]
    L.qm_batch_n_truth.argtypes = [vp]
    L.qm_classify_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.qm_batch_create.argtypes = [vp, i32, vp, vp, i32, C.POINTER(vp)]
    L.qm_batch_destroy.argtypes = [vp]
    L.qm_batch_destroy.restype = None
    L.qm_batch_upload.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.qm_batch_synth.argtypes = [vp, C.POINTER(SynthCfg)]
    L.qm_bench_synth.argtypes = [vp, C.POINTER(SynthCfg), i32, i64, i32, i32, C.POINTER(BenchResult)]
    L.qm_batch_run.argtypes = [vp, vp, vp]
    L.qm_batch_finish.argtypes = [vp, vp]
    L.qm_batch_set_timing.argtypes = [vp, i32]
    L.qm_batch_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_batch_get_cls.argtypes = [vp, i32, vp]
    L.qm_batch_get_idx.argtypes = [vp, i32, vp]
    L.qm_batch_get_roc.argtypes = [vp, vp]
    L.qm_batch_get_scalars.argtypes = [vp, vp]
    L.qm_batch_get_global.argtypes = [vp, vp]
    L.qm_batch_get_columns.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.qm_batch_device_bytes.argtypes = [vp]
    L.qm_batch_device_bytes.restype = i64
    L.qm_fp_overlap.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.qm_vcf_count_lines.argtypes = [C.c_char_p, C.c_size_t]
    L.qm_vcf_count_lines.restype = i64
    L.qm_vcf_scan.argtypes = [C.c_char_p, C.c_size_t, i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(VcfCols)]
    L.qm_truth_scan.argtypes = [C.c_char_p, C.c_size_t, i32, i64, vp, vp, vp, vp]
    L.qm_truth_scan.restype = i64
    L.qm_vcf_scan_ext.argtypes = [C.c_char_p, C.c_size_t, i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(VcfCols), vp]
    L.qm_truth_scan_ext.argtypes = [C.c_char_p, C.c_size_t, i32, i64, vp, vp, vp, vp, vp]
    L.qm_truth_scan_ext.restype = i64
    L.qm_dict_create.argtypes = []
    L.qm_dict_create.restype = vp
    L.qm_dict_destroy.argtypes = [vp]
    L.qm_dict_destroy.restype = None
    L.qm_dict_size.argtypes = [vp]
    L.qm_dict_size.restype = i64
    L.qm_allele_code.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.qm_allele_code.restype = i32
    L.qm_allele_spell.argtypes = [vp, i32, C.c_char_p, C.c_size_t]
    L.qm_allele_spell.restype = i64
    L.qm_extract_files.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double)]
    L.qm_extract_files_ex.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp]
    L.qm_batch_global_device.argtypes = [vp, C.POINTER(vp)]
    L.qm_batch_path_stats.argtypes = [vp, vp]
    L.qm_path_stats_total.argtypes = [vp, vp]
    L.qm_mummer2vcf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_uint, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.qm_free.argtypes = [vp]
    L.qm_free.restype = None
    L.qm_comm_create.argtypes = [C.POINTER(vp), i32, C.POINTER(vp)]
    L.qm_comm_make_id.argtypes = [vp]
    L.qm_comm_create_rank.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    L.qm_allreduce_counters.argtypes = [vp, vp, vp]
    L.qm_comm_collectives.argtypes = [vp, vp]
    L.qm_comm_collectives.restype = i64
    L.qm_comm_destroy.argtypes = [vp]
    L.qm_comm_destroy.restype = None
    L.qm_batch_upload_async.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.qm_batch_get_masks.argtypes = [vp, i32, vp, vp]
    L.qm_bgzf_write.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, i32]
    L.qm_bgzf_write_tbi.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, i32]
    L.qm_bw_probe.argtypes = [vp, i64, i32, C.POINTER(C.c_double)]
    L.qm_patterns_create.argtypes = [C.c_char_p, C.c_size_t, i32, i32]
    L.qm_patterns_create.restype = vp
    L.qm_patterns_destroy.argtypes = [vp]
    L.qm_patterns_destroy.restype = None
    L.qm_patterns_info.argtypes = [vp, vp]
    L.qm_vcf_hostpath.argtypes = [vp, C.c_char_p, C.c_size_t, i64, vp, vp, vp, vp, vp, vp, vp]
    L.qm_vcf_write.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, i64, vp, vp, vp, i32]
    L.qm_vcf_split_write.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, i32, i32, C.POINTER(C.c_int64)]
    L.qm_genome_load.argtypes = [vp, C.c_char_p, i64, C.POINTER(i32)]
    L.qm_genome_release.argtypes = [vp, i32]
    L.qm_batch_motifs.argtypes = [vp, vp, vp]
    L.qm_batch_get_motifs.argtypes = [vp, vp]
    L.qm_extract_files_motifs.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                          vp, vp]
    L.qm_batch_truth_hits.argtypes = [vp, vp]
    L.qm_batch_get_truth_hits.argtypes = [vp, i32, vp, i64]
    L.qm_batch_get_intruth_mask.argtypes = [vp, i32, vp]
    L.qm_batch_truth_regions.argtypes = [vp, i32, vp, vp, vp, vp]
    L.qm_extract_files_truthside.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                             C.POINTER(TruthSideArgs)]
    L.qm_vcf_scan_af.argtypes = [C.c_char_p, C.c_size_t, i64, vp, vp, vp, vp]
    L.qm_batch_upload_af.argtypes = [vp, i32, vp]
    L.qm_batch_af_profile.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp]
    L.qm_batch_get_af_profile.argtypes = [vp, vp, vp]
    L.qm_extract_files_profile.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                           vp, vp, C.POINTER(ProfileArgs)]
    L.qm_strata_load.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i32)]
    L.qm_strata_info.argtypes = [vp, i32, vp]
    L.qm_strata_segments.argtypes = [vp, i32, vp, vp]
    L.qm_strata_release.argtypes = [vp, i32]
    L.qm_batch_strata.argtypes = [vp, i32, C.c_uint, vp]
    L.qm_batch_get_strata.argtypes = [vp, vp, vp]
    L.qm_extract_files_strata.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                          C.POINTER(StrataArgs)]
    L.qm_batch_boot.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint, vp]
    L.qm_batch_get_boot.argtypes = [vp, vp, vp]
    L.qm_boot_draws.argtypes = [C.c_uint64, C.c_int32, C.c_int32, vp]
    L.qm_extract_files_boot.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                        C.POINTER(BootArgs)]
    L.qm_batch_votes.argtypes = [vp, i32, vp, vp, vp]
    L.qm_batch_get_votes.argtypes = [vp, vp, vp, vp, vp, vp]
    L.qm_batch_get_vote_keys.argtypes = [vp, i32, vp, vp, i64, C.POINTER(i64)]
    L.qm_batch_vote_groups.argtypes = [vp]
    L.qm_batch_vote_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_extract_files_votes.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                         C.POINTER(VotesArgs)]
    L.qm_batch_nearmiss.argtypes = [vp, i32, vp]
    L.qm_batch_get_nearmiss.argtypes = [vp, vp, vp]
    L.qm_batch_get_nearmiss_cls.argtypes = [vp, i32, vp]
    L.qm_batch_get_nearmiss_truth.argtypes = [vp, i32, vp]
    L.qm_batch_nearmiss_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_extract_files_nearmiss.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                            C.POINTER(NearmissArgs)]
    L.qm_batch_surface.argtypes = [vp, i32, i32, i32, vp]
    L.qm_batch_get_surface.argtypes = [vp, vp, vp]
    L.qm_batch_surface_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_extract_files_surface.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                           C.POINTER(SurfaceArgs)]
    L.qm_genome_context.argtypes = [vp, i32, C.c_int32, C.c_int32, vp, vp]
    L.qm_batch_context.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_uint, vp]
    L.qm_batch_get_context.argtypes = [vp, vp, vp, vp]
    L.qm_batch_context_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_extract_files_context.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                           C.POINTER(ContextArgs)]
    L.qm_extract_files_normalize.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                             C.POINTER(NormalizeArgs)]
    L.qm_batch_normalize.argtypes = [vp, vp, C.c_uint, vp]
    L.qm_batch_get_normalize.argtypes = [vp, vp, vp]
    L.qm_batch_get_normalized.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.qm_batch_normalize_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_truth_normalized.argtypes = [vp, i32, i32, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.qm_truth_entries.argtypes = [vp, i32, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.qm_extract_files_atomize.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                           C.POINTER(AtomizeArgs)]
    L.qm_batch_atomize.argtypes = [vp, C.c_uint, vp]
    L.qm_batch_get_atomize.argtypes = [vp, vp, vp]
    L.qm_batch_get_atomized.argtypes = [vp, i32, vp, vp, vp]
    L.qm_batch_atomize_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_truth_atoms.argtypes = [vp, i32, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.qm_dict_shapes.argtypes = [vp, i64, i64, vp, vp, vp]
    L.qm_dict_shapes.restype = i64
    L.qm_batch_types.argtypes = [vp, vp, i32, vp, vp, vp, i64, C.c_uint, vp]
    L.qm_batch_get_types.argtypes = [vp, vp, vp]
    L.qm_batch_get_typed.argtypes = [vp, i32, vp]
    L.qm_batch_types_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_batch_haplotypes.argtypes = [vp, vp, i32, C.c_uint, vp]
    L.qm_batch_get_haplotypes.argtypes = [vp, vp, vp]
    L.qm_batch_get_haplotyped.argtypes = [vp, i32, vp, vp, vp]
    L.qm_batch_haplotype_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_batch_hapsubsets.argtypes = [vp, C.c_uint, vp]
    L.qm_batch_get_hapsubsets.argtypes = [vp, vp]
    L.qm_batch_get_hapsubsetted.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.qm_batch_hapsubset_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_batch_rescue_roc.argtypes = [vp, C.c_uint, vp]
    L.qm_batch_get_rescue_roc.argtypes = [vp, vp, vp, vp]
    L.qm_batch_rescue_roc_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_batch_ladder.argtypes = [vp, C.c_uint, vp]
    L.qm_batch_get_ladder.argtypes = [vp, vp, vp]
    L.qm_batch_get_laddered.argtypes = [vp, i32, vp, vp]
    L.qm_batch_ladder_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_batch_ladder_types.argtypes = [vp, vp]
    L.qm_batch_get_ladder_types.argtypes = [vp, vp, vp, C.POINTER(C.c_int)]
    L.qm_batch_ladder_types_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.qm_extract_files_haplotypes.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                              C.POINTER(HaplotypesArgs)]
    L.qm_truth_sites.argtypes = [vp, i32, i32, i32, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
    L.qm_extract_files_hapsubsets.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                              C.POINTER(HapsubArgs)]
    L.qm_extract_files_rescue_roc.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                              C.POINTER(RescueRocArgs)]
    L.qm_extract_files_ladder.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                          C.POINTER(LadderArgs)]
    L.qm_extract_files_ladder_types.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                                C.POINTER(LadderTypesArgs)]
    L.qm_extract_files_types.argtypes = [vp, i32, C.POINTER(FileJob), i32, C.c_uint, i32, C.POINTER(FileStats), vp, C.POINTER(C.c_double), vp, i32, vp,
                                         C.POINTER(TypesArgs)]
    _lib = L
    return L


def check(rc, ctx=None):
    if rc < 0:
        raise QmvtError(rc, lib().qm_last_error(ctx).decode("utf-8", "replace"))
    return rc
