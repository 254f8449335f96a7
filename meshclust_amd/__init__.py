"""meshclust_amd -- MI355X-native engine for MeShClust's data-parallel hot path.

The product is native code built in-tree by ``meshclust_amd/csrc/Makefile``:

* ``lib/libmcgpu.so``      gfx950 HIP kernels behind the C-ABI of ``include/meshclust_amd.h``
* ``lib/libmeshclust.so``  the host driver (reference control flow) + in-process C API
* ``bin/meshclust``        drop-in CLI for the reference's ``bin/meshclust``

This module is a thin ctypes view of those libraries for tests and ``bench.py``.  It never
computes anything itself: if the libraries are missing or no GPU is present, the calls fail
loudly (``ImportError`` / ``MCError``); there is no CPU fallback.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_DIR = os.path.join(HERE, "lib")
BIN = os.path.join(HERE, "bin", "meshclust")
GPU_LIB = os.environ.get("MC_GPU_LIB", os.path.join(LIB_DIR, "libmcgpu.so"))
HOST_LIB = os.path.join(LIB_DIR, "libmeshclust.so")
HEADER = os.path.join(ROOT, "include", "meshclust_amd.h")

FEAT_ALIGN, FEAT_LD, FEAT_MANHATTAN = 1, 2, 4
FEAT_INTERSECTION, FEAT_PEARSON, FEAT_KULCZYNSKI2 = 16, 32, 1024
COMBO_SQUARED, COMBO_SELF = 1, 2
ASSIGN_NONE = 0xFFFFFFFF
MC_STRAND_PLUS, MC_STRAND_MINUS = 1, 2
ASSIGN_MAX_TOP = 8  # MC_ASSIGN_MAX_TOP
ERR_ARG, ERR_UNSUPPORTED = 1, 6
ERR_STATE = 3
CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X = 1, 2, 7, 8  # MC_CIGAR_*: mc_nw_align_strands' words are run << 4 | op
PILEUP_CH = 8  # MC_PILEUP_CH: counters per row of mc_nw_pileup_strands' table
MSA_GAP = ord("-")  # MC_MSA_GAP: the gap byte of mc_nw_msa_rows
MSA_CH = 8  # MC_MSA_CH: counters per column of mc_nw_msa_counts
CROSS_RES = 8  # MC_CROSS_RES: values per candidate of mc_nw_msa_crossover
QUAL_MAX = 93  # MC_QUAL_MAX: the largest Phred value mc_load_qualities takes
QGRAM_NA = 0xFFFFFFFF  # MC_QGRAM_NA: mc_qgram_common's "not available"
FAMILIES = ("kmer", "keys", "pairs", "scan", "finalize", "mean_shift", "nw", "layout")


class MCError(RuntimeError):
    pass


def build(jobs=8):
    """Compile libmcgpu / libmeshclust / bin/meshclust for gfx950 (hipcc cross-compiles)."""
    subprocess.run(["make", "-s", "-j%d" % jobs, "-C", os.path.join(HERE, "csrc")], check=True)


class Classifier(C.Structure):
    _fields_ = [
        ("n_single", C.c_int32),
        ("lookup", C.c_uint16 * 8),
        ("is_sim", C.c_int32 * 8),
        ("mins", C.c_double * 8),
        ("maxs", C.c_double * 8),
        ("n_combo", C.c_int32),
        ("combo_kind", C.c_int32 * 8),
        ("combo_len", C.c_int32 * 8),
        ("combo_idx", (C.c_int32 * 4) * 8),
        ("weights", C.c_double * 9),
    ]


class ScanResult(C.Structure):
    _fields_ = [
        ("is_min", C.c_int32),
        ("has_best", C.c_int32),
        ("best_pos", C.c_uint64),
        ("best_val", C.c_double),
        ("n_flagged", C.c_uint64),
        ("new_centre", C.c_uint32),
        ("n_members", C.c_uint32),
        ("nw_pairs", C.c_uint64),
        ("nw_cells", C.c_uint64),
    ]


_gpu = None
_host = None


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def gpu_lib():
    global _gpu
    if _gpu is None:
        if not os.path.exists(GPU_LIB):
            raise ImportError("libmcgpu.so not built (run meshclust_amd.build()); no CPU fallback exists")
        lib = C.CDLL(GPU_LIB)
        lib.mc_last_error.restype = C.c_char_p
        lib.mc_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.mc_ctx_destroy.argtypes = [C.c_void_p]
        for name in ("mc_load_sequences", "mc_load_packed", "mc_kmer_max", "mc_kmer_build", "mc_get_histograms", "mc_distance_keys",
                     "mc_pair_features", "mc_set_classifier", "mc_classify_pairs", "mc_nw_identity",
                     "mc_nw_identity_raw", "mc_set_order", "mc_kill", "mc_cluster_begin", "mc_scan",
                     "mc_mean_shift", "mc_update_iteration", "mc_timers", "mc_classify_values", "mc_mean_shift_select", "mc_accumulate",
                     "mc_scan_part", "mc_scan_commit", "mc_comm_unique_id", "mc_comm_create", "mc_comm_allgather",
                     "mc_comm_stats", "mc_comm_destroy", "mc_sync", "mc_assign", "mc_assign_strands",
                     "mc_revcomp_rows", "mc_assign_top", "mc_revcomp_sequences", "mc_nw_identity_strands",
                     "mc_nw_align_strands", "mc_nw_align_profile", "mc_nw_pileup_strands", "mc_nw_pileup_profile",
                     "mc_kmer_max_strands", "mc_kmer_build_strands", "mc_orient_pairs", "mc_qgram_common"):
            getattr(lib, name).restype = C.c_int
        lib.mc_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
        lib.mc_comm_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.mc_comm_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.mc_comm_destroy.argtypes = [C.c_void_p, C.c_int]
        lib.mc_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_double,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mc_assign_strands.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_double, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mc_revcomp_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.mc_assign_top.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_double, C.c_int,
                                      C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mc_revcomp_sequences.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.mc_nw_identity_strands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
        lib.mc_qgram_common.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        lib.mc_nw_align_strands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                            C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mc_nw_align_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.mc_nw_pileup_strands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mc_nw_pileup_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.mc_kmer_max_strands.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        lib.mc_kmer_build_strands.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        lib.mc_orient_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.mc_load_qualities.restype = C.c_int
        lib.mc_load_qualities.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        lib.mc_nw_qpileup_strands.restype = C.c_int
        lib.mc_nw_qpileup_strands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        for name in ("mc_nw_msa_begin", "mc_nw_msa_rows", "mc_nw_msa_end", "mc_nw_msa_profile"):
            getattr(lib, name).restype = C.c_int
        lib.mc_nw_msa_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mc_nw_msa_rows.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.mc_nw_msa_end.argtypes = [C.c_void_p]
        lib.mc_nw_msa_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.mc_nw_msa_counts.restype = C.c_int
        lib.mc_nw_msa_counts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        lib.mc_nw_msa_counts_profile.restype = C.c_int
        lib.mc_nw_msa_counts_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.mc_nw_msa_sites.restype = C.c_int
        lib.mc_nw_msa_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.c_void_p]
        lib.mc_nw_msa_sites_profile.restype = C.c_int
        lib.mc_nw_msa_sites_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.mc_nw_msa_crossover.restype = C.c_int
        lib.mc_nw_msa_crossover.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        lib.mc_nw_msa_crossover_profile.restype = C.c_int
        lib.mc_nw_msa_crossover_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        lib.mc_derep.restype = C.c_int
        lib.mc_derep.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        lib.mc_derep_profile.restype = C.c_int
        lib.mc_derep_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        for name in ("mc_set_align_band", "mc_nw_band_plan", "mc_nw_band_profile"):
            getattr(lib, name).restype = C.c_int
        lib.mc_set_align_band.argtypes = [C.c_void_p, C.c_int]
        lib.mc_nw_band_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.mc_nw_band_profile.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _bind_steps(lib)
        _gpu = lib
    return _gpu


def _bind_steps(lib):
    """Argument types of the get_close / mean-shift step API, on any library with the C-ABI of
    include/meshclust_amd.h."""
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.mc_set_order.argtypes = [vp, vp, u64]
    lib.mc_kill.argtypes = [vp, u64]
    lib.mc_cluster_begin.argtypes = [vp, u32]
    lib.mc_scan.argtypes = [vp, u32, u64, u64, vp, u64, C.POINTER(ScanResult)]
    lib.mc_scan_part.argtypes = [vp, u32, u64, u64, u32, u32, vp, u64, C.POINTER(ScanResult)]
    lib.mc_scan_commit.argtypes = [vp, vp, u64, C.POINTER(ScanResult)]
    lib.mc_align_part.argtypes = [vp, u32, u64, u64, u32, u32, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.mc_scan_ident.argtypes = [vp, u32, u64, u64, vp, vp, u64, C.POINTER(ScanResult)]
    lib.mc_mean_shift_range.argtypes = [vp, vp, u32, vp, vp, C.c_int, u32, u32, vp]
    for name in ("mc_set_order", "mc_kill", "mc_cluster_begin", "mc_scan", "mc_scan_part", "mc_scan_commit",
                 "mc_align_part", "mc_scan_ident", "mc_mean_shift_range", "mc_mean_shift"):
        getattr(lib, name).restype = C.c_int
    lib.mc_last_error.restype = C.c_char_p


def load_engine_lib(path):
    """Another library with libmcgpu's C-ABI (the tests' CPU oracle engine), for ``Engine(lib=...)``.
    Loaded with ctypes' default RTLD_LOCAL: its mc_* names stay its own."""
    lib = C.CDLL(path)
    lib.mc_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.mc_ctx_destroy.argtypes = [C.c_void_p]
    _bind_steps(lib)
    return lib


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise ImportError("libmeshclust.so not built (run meshclust_amd.build())")
        gpu_lib()
        lib = C.CDLL(HOST_LIB)
        lib.mcl_parse.restype = C.c_void_p
        lib.mcl_parse.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_char_p, C.c_int]
        lib.mcl_parse_q.restype = C.c_void_p
        lib.mcl_parse_q.argtypes = lib.mcl_parse.argtypes
        lib.mcl_qualities.restype = None
        lib.mcl_qualities.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        lib.mcl_num_seqs.restype = C.c_uint64
        lib.mcl_num_seqs.argtypes = [C.c_void_p]
        lib.mcl_view.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4
        lib.mcl_header.restype = C.c_char_p
        lib.mcl_header.argtypes = [C.c_void_p, C.c_uint64]
        lib.mcl_free.argtypes = [C.c_void_p]
        lib.mcl_run.restype = C.c_int
        lib.mcl_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_char_p,
                                C.c_char_p, C.c_int]
        lib.mcl_run_sharded.restype = C.c_int
        lib.mcl_run_sharded.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_char_p,
                                        C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        lib.mcl_tune_host_heap.restype = C.c_int
        lib.mcl_assign.restype = C.c_int
        lib.mcl_assign.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                   C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        lib.mcl_assign_strands.restype = C.c_int
        lib.mcl_assign_strands.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                           C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        lib.mcl_assign_top.restype = C.c_int
        lib.mcl_assign_top.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                       C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
        lib.mcl_assign_identity.restype = C.c_int
        lib.mcl_assign_identity.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                            C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double,
                                            C.c_char_p, C.c_int]
        lib.mcl_assign_paf.restype = C.c_int
        lib.mcl_assign_paf.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                       C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double,
                                       C.c_char_p, C.c_char_p, C.c_int]
        lib.mcl_assign_consensus.restype = C.c_int
        lib.mcl_assign_consensus.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                             C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double,
                                             C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        lib.mcl_assign_qconsensus.restype = C.c_int
        lib.mcl_assign_qconsensus.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                              C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double,
                                              C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        lib.mcl_assign_msa.restype = C.c_int
        lib.mcl_assign_msa.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                       C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double,
                                       C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
        lib.mcl_assign_profile.restype = C.c_int
        lib.mcl_assign_profile.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                           C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double,
                                           C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        lib.mcl_assign_band.restype = C.c_int
        lib.mcl_assign_band.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                        C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_double,
                                        C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p,
                                        C.c_int]
        lib.mcl_assign_variants.restype = C.c_int
        lib.mcl_assign_variants.argtypes = lib.mcl_assign_band.argtypes[:-2] + [C.c_char_p, C.c_char_p, C.c_char_p, C.c_double,
                                                                                C.c_longlong, C.c_char_p, C.c_int]
        lib.mcl_assign_chimeras.restype = C.c_int
        lib.mcl_assign_chimeras.argtypes = lib.mcl_assign_variants.argtypes[:-2] + [C.c_char_p, C.c_longlong, C.c_char_p, C.c_int]
        lib.mcl_derep.restype = C.c_int
        lib.mcl_derep.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int,
                                  C.c_longlong, C.c_char_p, C.c_int]
        lib.mcl_derep_host.restype = C.c_int
        lib.mcl_derep_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
        _host = lib
    return _host


def tune_host_heap():
    """Opt in (process-global): keep large freed host blocks in the heap, so repeated parses and
    clusterings in this process touch no new pages (what bin/meshclust does for itself)."""
    return bool(host_lib().mcl_tune_host_heap())


def _check(rc, what, lib=None):
    if rc != 0:
        e = MCError("%s failed (%d): %s" % (what, rc, (lib or gpu_lib()).mc_last_error().decode()))
        e.code = rc
        raise e


def _scan_dict(r):
    return {name: getattr(r, name) for name, _ in ScanResult._fields_}


class Engine:
    """One libmcgpu context on one GPU (``mc_ctx``).  ``lib``: another library with the same C-ABI
    (``load_engine_lib``) to drive instead of libmcgpu -- the loading, histogram, classifier and
    step calls then go to it."""

    def __init__(self, device=0, lib=None):
        self.lib = lib if lib is not None else gpu_lib()
        self.ctx = C.c_void_p()
        self._ck(self.lib.mc_ctx_create(device, C.byref(self.ctx)), "mc_ctx_create")
        self.n = 0
        self.width = 0
        self.B = 0

    def _ck(self, rc, what):
        _check(rc, what, self.lib)

    def close(self):
        if self.ctx:
            self.lib.mc_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_sequences(self, codes, seq_off, seg, seg_off):
        codes = np.ascontiguousarray(codes, np.uint8)
        seq_off = np.ascontiguousarray(seq_off, np.uint64)
        seg = np.ascontiguousarray(seg, np.int32).reshape(-1)
        seg_off = np.ascontiguousarray(seg_off, np.uint64)
        if seg.size == 0:
            seg = np.zeros(2, np.int32)
        self.n = len(seq_off) - 1
        self._ck(self.lib.mc_load_sequences(self.ctx, _p(codes), _p(seq_off), C.c_uint64(self.n), _p(seg),
                                          _p(seg_off)), "mc_load_sequences")

    def load_packed(self, seqs, segs):
        """seqs: list of uint8 one-digit arrays; segs: per sequence [[s, e], ...].  Packs them the
        way the host parser does (2-bit words, records word-aligned, exception bytes) and loads
        them with mc_load_packed."""
        lens = [len(x) for x in seqs]
        seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        pk_off = np.concatenate([[0], np.cumsum([(l + 15) // 16 for l in lens])]).astype(np.uint64)
        packed = np.zeros(max(1, int(pk_off[-1])), np.uint32)
        exc_pos, exc_val = [], []
        for i, x in enumerate(seqs):
            x = np.asarray(x, np.uint8)
            pad = np.zeros((len(x) + 15) // 16 * 16, np.uint32)
            pad[:len(x)] = x & 3
            w = (pad.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64)
            packed[int(pk_off[i]):int(pk_off[i + 1])] = w.astype(np.uint32)
            bad = np.nonzero(x > 3)[0]
            exc_pos.extend((int(seq_off[i]) + bad).tolist())
            exc_val.extend(x[bad].tolist())
        seg = np.array([v for s in segs for pair in s for v in pair], np.int32)
        seg_off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.uint64)
        if seg.size == 0:
            seg = np.zeros(2, np.int32)
        ep = np.array(exc_pos, np.uint64)
        ev = np.array(exc_val, np.uint8)
        self.n = len(seqs)
        self._ck(self.lib.mc_load_packed(self.ctx, _p(packed), _p(pk_off), _p(seq_off), C.c_uint64(self.n),
                                       _p(ep) if len(ep) else None, _p(ev) if len(ev) else None, C.c_uint64(len(ep)),
                                       _p(seg), _p(seg_off)), "mc_load_packed")

    def kmer_max(self, k):
        out = C.c_uint64()
        self._ck(self.lib.mc_kmer_max(self.ctx, k, C.byref(out)), "mc_kmer_max")
        return out.value

    def kmer_build(self, k, width):
        self._ck(self.lib.mc_kmer_build(self.ctx, k, width), "mc_kmer_build")
        self.width, self.B = width, 4 ** k

    def kmer_max_strands(self, k, strands=MC_STRAND_PLUS | MC_STRAND_MINUS):
        """mc_kmer_max_strands: the largest bin of the forward rows (strands 1) or of the canonical
        rows row[i] + row[rc(i)] - 1 (strands 3)."""
        out = C.c_uint64()
        self._ck(self.lib.mc_kmer_max_strands(self.ctx, k, strands, C.byref(out)), "mc_kmer_max_strands")
        return out.value

    def kmer_build_strands(self, k, width, strands=MC_STRAND_PLUS | MC_STRAND_MINUS):
        """mc_kmer_build_strands: strands 1 is kmer_build; strands 3 leaves the canonical rows as the
        engine's histograms and keeps the forward rows for orient_pairs."""
        self._ck(self.lib.mc_kmer_build_strands(self.ctx, k, width, strands), "mc_kmer_build_strands")
        self.width, self.B = width, 4 ** k

    def orient_pairs(self, a, b, sad=True):
        """mc_orient_pairs on the forward rows: strand[p] = 1 iff sum |row_a - row_b[rc]| <
        sum |row_a - row_b| -> (strand, sad[m, 2] = (plus, minus) or None).  Pass pairs grouped by b."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        assert len(a) == len(b)
        strand = np.zeros(len(a), np.uint8)
        sums = np.zeros((len(a), 2), np.uint64) if sad else None
        self._ck(self.lib.mc_orient_pairs(self.ctx, _p(a), _p(b), C.c_uint64(len(a)), _p(strand),
                                          _p(sums) if sad else None), "mc_orient_pairs")
        return strand, sums

    def histograms(self):
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[self.width]
        h = np.zeros((self.n, self.B), dt)
        m = np.zeros(self.n, np.uint64)
        self._ck(self.lib.mc_get_histograms(self.ctx, _p(h), _p(m)), "mc_get_histograms")
        return h, m

    def distance_keys(self, pivots, ids):
        pivots = np.ascontiguousarray(pivots, np.uint32)
        ids = np.ascontiguousarray(ids, np.uint32)
        keys = np.zeros((len(pivots), len(ids)), np.uint16)
        self._ck(self.lib.mc_distance_keys(self.ctx, _p(pivots), C.c_uint32(len(pivots)), _p(ids),
                                         C.c_uint64(len(ids)), _p(keys)), "mc_distance_keys")
        return keys

    def pair_features(self, a, b, flags):
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        fl = np.ascontiguousarray(flags, np.uint16)
        raw = np.zeros((len(a), len(fl)), np.float64)
        self._ck(self.lib.mc_pair_features(self.ctx, _p(a), _p(b), C.c_uint64(len(a)), _p(fl), len(fl), _p(raw)),
               "mc_pair_features")
        return raw

    def set_classifier(self, cls):
        self._ck(self.lib.mc_set_classifier(self.ctx, C.byref(cls)), "mc_set_classifier")

    def classify_pairs(self, a, b):
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        sim = np.zeros(len(a), np.uint8)
        c0 = np.zeros(len(a))
        s = np.zeros(len(a))
        self._ck(self.lib.mc_classify_pairs(self.ctx, _p(a), _p(b), C.c_uint64(len(a)), _p(sim), _p(c0), _p(s)),
               "mc_classify_pairs")
        return sim, c0, s

    def assign(self, centres, queries, sim=0.0):
        """mc_assign: every query scored against every centre (point ids) on the device ->
        (best centre index or ASSIGN_NONE, its combo 0 or -1.0, similar centres per query,
        [candidate pairs, fall-backs to the full scorer, device time in us])."""
        centres = np.ascontiguousarray(centres, np.uint32)
        queries = np.ascontiguousarray(queries, np.uint32)
        m = len(queries)
        best = np.full(m, ASSIGN_NONE, np.uint32)
        val = np.full(m, -1.0)
        nsim = np.zeros(m, np.uint32)
        stats = np.zeros(3, np.uint64)
        self._ck(self.lib.mc_assign(self.ctx, _p(centres), len(centres), _p(queries), m, float(sim), _p(best), _p(val),
                                  _p(nsim), _p(stats)), "mc_assign")
        return best, val, nsim, stats

    def assign_strands(self, centres, queries, sim=0.0, strands=MC_STRAND_PLUS | MC_STRAND_MINUS):
        """mc_assign_strands: assign() on the strand set ``strands`` (MC_STRAND_PLUS, MC_STRAND_MINUS
        or both) -> (best, best_val, strand (0 plus, 1 minus), n_similar, stats).  With both strands
        the minus strand wins a query only with a strictly larger combo 0; n_similar adds up."""
        centres = np.ascontiguousarray(centres, np.uint32)
        queries = np.ascontiguousarray(queries, np.uint32)
        m = len(queries)
        best = np.full(m, ASSIGN_NONE, np.uint32)
        val = np.full(m, -1.0)
        strand = np.zeros(m, np.uint8)
        nsim = np.zeros(m, np.uint32)
        stats = np.zeros(3, np.uint64)
        self._ck(self.lib.mc_assign_strands(self.ctx, _p(centres), len(centres), _p(queries), m, float(sim), int(strands),
                                          _p(best), _p(val), _p(strand), _p(nsim), _p(stats)), "mc_assign_strands")
        return best, val, strand, nsim, stats

    def assign_top(self, centres, queries, sim=0.0, strands=MC_STRAND_PLUS, k=ASSIGN_MAX_TOP):
        """mc_assign_top: the ``k`` (1 .. ASSIGN_MAX_TOP) best similar centres of every query on the
        strand set ``strands`` -> (hit (M, k), hit_val (M, k), hit_strand (M, k), n_similar, stats).
        A row is ordered by combo 0 descending, then plus before minus, then centre index ascending;
        its unused slots hold ASSIGN_NONE, -1.0 and 0.  n_similar is not capped at k."""
        centres = np.ascontiguousarray(centres, np.uint32)
        queries = np.ascontiguousarray(queries, np.uint32)
        m, kk = len(queries), max(int(k), 0)
        hit = np.full((m, kk), ASSIGN_NONE, np.uint32)
        val = np.full((m, kk), -1.0)
        strand = np.zeros((m, kk), np.uint8)
        nsim = np.zeros(m, np.uint32)
        stats = np.zeros(3, np.uint64)
        self._ck(self.lib.mc_assign_top(self.ctx, _p(centres), len(centres), _p(queries), m, float(sim), int(strands), int(k),
                                      _p(hit), _p(val), _p(strand), _p(nsim), _p(stats)), "mc_assign_top")
        return hit, val, strand, nsim, stats

    def revcomp_rows(self, ids):
        """mc_revcomp_rows: the histogram rows of the points ``ids`` permuted to the other strand
        (row[rc(i)]: the histograms of the reverse-complemented records), shape (len(ids), 4^k)."""
        ids = np.ascontiguousarray(ids, np.uint32)
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[self.width]
        rows = np.zeros((len(ids), self.B), dt)
        self._ck(self.lib.mc_revcomp_rows(self.ctx, _p(ids), len(ids), _p(rows)), "mc_revcomp_rows")
        return rows

    def classify_values(self, raw):
        """raw: (m, n_single) precomputed single-feature values -> (similar, combo0, sum)."""
        raw = np.ascontiguousarray(raw, np.float64)
        m = raw.shape[0]
        sim = np.zeros(m, np.uint8)
        c0 = np.zeros(m)
        s = np.zeros(m)
        self._ck(self.lib.mc_classify_values(self.ctx, _p(raw), C.c_uint64(m), _p(sim), _p(c0), _p(s)),
               "mc_classify_values")
        return sim, c0, s

    def mean_shift(self, centres, member_off, members, delta):
        centres = np.ascontiguousarray(centres, np.uint32)
        member_off = np.ascontiguousarray(member_off, np.uint64)
        members = np.ascontiguousarray(members, np.uint32)
        out = np.zeros(len(centres), np.uint32)
        self._ck(self.lib.mc_mean_shift(self.ctx, _p(centres), len(centres), _p(member_off), _p(members), delta, _p(out)),
               "mc_mean_shift")
        return out

    def update_iteration(self, centres, member_off, members, delta):
        """mc_update_iteration: (new centres, merge pairs' similar flags, their combo 0 values)."""
        centres = np.ascontiguousarray(centres, np.uint32)
        member_off = np.ascontiguousarray(member_off, np.uint64)
        members = np.ascontiguousarray(members, np.uint32)
        C_ = len(centres)
        m = sum(min(delta, C_ - 1 - i) for i in range(C_))
        out = np.zeros(C_, np.uint32)
        sim = np.zeros(max(m, 1), np.uint8)
        c0 = np.zeros(max(m, 1))
        n = C.c_uint64(0)
        self._ck(self.lib.mc_update_iteration(self.ctx, _p(centres), C_, _p(member_off), _p(members), delta, _p(out),
                                            _p(sim), _p(c0), C.byref(n)), "mc_update_iteration")
        assert n.value == m
        return out, sim[:m], c0[:m]

    # ---- the step API: every call returns its return code first (nothing raises), so a driver
    # can run the same script on two engines and compare the codes as well
    def set_order(self, order):
        """mc_set_order: order[pos] = point id, a permutation of all points -> rc."""
        order = np.ascontiguousarray(order, np.uint32)
        return self.lib.mc_set_order(self.ctx, _p(order), len(order))

    def kill(self, pos):
        """mc_kill of one static position -> rc."""
        return self.lib.mc_kill(self.ctx, int(pos))

    def cluster_begin(self, first):
        """mc_cluster_begin: the next step starts the cluster {first} -> rc."""
        return self.lib.mc_cluster_begin(self.ctx, int(first))

    def scan(self, centre, S, E, cap=None):
        """mc_scan -> (rc, result dict of the mc_scan_result fields, flagged positions).  ``cap``:
        capacity of the flagged buffer (default: the window)."""
        cap = max(int(E) - int(S) + 1, 1) if cap is None else int(cap)
        fl = np.zeros(max(cap, 1), np.uint32)
        r = ScanResult()
        rc = self.lib.mc_scan(self.ctx, int(centre), int(S), int(E), _p(fl), cap, C.byref(r))
        return rc, _scan_dict(r), fl[:min(int(r.n_flagged), cap)].copy() if rc == 0 else fl[:0]

    def scan_part(self, centre, S, E, part, nparts, cap=None):
        """mc_scan_part -> (rc, result dict, this part's similar positions)."""
        cap = max(int(E) - int(S) + 1, 1) if cap is None else int(cap)
        fl = np.zeros(max(cap, 1), np.uint32)
        r = ScanResult()
        rc = self.lib.mc_scan_part(self.ctx, int(centre), int(S), int(E), int(part), int(nparts), _p(fl), cap, C.byref(r))
        return rc, _scan_dict(r), fl[:min(int(r.n_flagged), cap)].copy() if rc == 0 else fl[:0]

    def scan_commit(self, flagged):
        """mc_scan_commit of the merged (ascending) positions -> (rc, result dict)."""
        fl = np.ascontiguousarray(flagged, np.uint32)
        r = ScanResult()
        rc = self.lib.mc_scan_commit(self.ctx, _p(fl) if len(fl) else None, len(fl), C.byref(r))
        return rc, _scan_dict(r)

    def align_part(self, centre, S, E, part, nparts, cap=None):
        """mc_align_part -> (rc, this part's identities, pairs, cells of the whole window)."""
        cap = max(int(E) - int(S) + 1, 1) if cap is None else int(cap)
        ident = np.zeros(max(cap, 1))
        n, pairs, cells = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = self.lib.mc_align_part(self.ctx, int(centre), int(S), int(E), int(part), int(nparts), _p(ident), cap,
                                    C.byref(n), C.byref(pairs), C.byref(cells))
        return rc, ident[:min(n.value, cap)].copy() if rc == 0 else ident[:0], pairs.value, cells.value

    def scan_ident(self, centre, S, E, ident, cap=None):
        """mc_scan_ident: mc_scan's alignment-mode step with the window's identities given ->
        (rc, result dict, flagged positions)."""
        cap = max(int(E) - int(S) + 1, 1) if cap is None else int(cap)
        ident = np.ascontiguousarray(ident, np.float64)
        fl = np.zeros(max(cap, 1), np.uint32)
        r = ScanResult()
        rc = self.lib.mc_scan_ident(self.ctx, int(centre), int(S), int(E), _p(ident), _p(fl), cap, C.byref(r))
        return rc, _scan_dict(r), fl[:min(int(r.n_flagged), cap)].copy() if rc == 0 else fl[:0]

    def mean_shift_range(self, centres, member_off, members, delta, j0, j1):
        """mc_mean_shift_range: the new centres of j0 <= j < j1 -> (rc, new centres)."""
        centres = np.ascontiguousarray(centres, np.uint32)
        member_off = np.ascontiguousarray(member_off, np.uint64)
        members = np.ascontiguousarray(members, np.uint32)
        out = np.zeros(max(int(j1) - int(j0), 1), np.uint32)
        rc = self.lib.mc_mean_shift_range(self.ctx, _p(centres), len(centres), _p(member_off), _p(members), int(delta),
                                          int(j0), int(j1), _p(out))
        return rc, out[:max(int(j1) - int(j0), 0)]

    def mean_shift_select(self, centres, member_off, members, delta, keep):
        centres = np.ascontiguousarray(centres, np.uint32)
        member_off = np.ascontiguousarray(member_off, np.uint64)
        members = np.ascontiguousarray(members, np.uint32)
        keep = np.ascontiguousarray(keep, np.uint8)
        out = np.zeros(len(centres), np.uint32)
        self._ck(self.lib.mc_mean_shift_select(self.ctx, _p(centres), len(centres), _p(member_off), _p(members), delta,
                                             _p(keep), _p(out)), "mc_mean_shift_select")
        return out

    def nw_identity(self, a, b):
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        ident = np.zeros(len(a))
        ln = np.zeros(len(a), np.int32)
        ids = np.zeros(len(a), np.int32)
        self._ck(self.lib.mc_nw_identity(self.ctx, _p(a), _p(b), C.c_uint64(len(a)), _p(ident), _p(ln), _p(ids)),
               "mc_nw_identity")
        return ident, ln, ids

    def revcomp_sequences(self, ids):
        """mc_revcomp_sequences: the minus-strand strings of the points ``ids`` (the expanded byte
        string reversed, digits d -> 3 - d, A <-> T, C <-> G, anything else unchanged), concatenated
        -> (bytes uint8, off uint64 of len(ids) + 1)."""
        ids = np.ascontiguousarray(ids, np.uint32)
        off = np.zeros(len(ids) + 1, np.uint64)
        self._ck(self.lib.mc_revcomp_sequences(self.ctx, _p(ids), len(ids), None, _p(off)), "mc_revcomp_sequences")
        out = np.zeros(int(off[-1]), np.uint8)
        self._ck(self.lib.mc_revcomp_sequences(self.ctx, _p(ids), len(ids), _p(out), _p(off)), "mc_revcomp_sequences")
        return out, off

    def nw_identity_strands(self, a, b, a_minus=None):
        """mc_nw_identity_strands: nw_identity with a strand per pair; where ``a_minus[i]`` is
        non-zero seq1 is the minus-strand string of point a[i] -> (ident, len, ids)."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        am = None if a_minus is None else np.ascontiguousarray(a_minus, np.uint8)
        assert am is None or len(am) == len(a)
        ident = np.zeros(len(a))
        ln = np.zeros(len(a), np.int32)
        ids = np.zeros(len(a), np.int32)
        self._ck(self.lib.mc_nw_identity_strands(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(len(a)), _p(ident), _p(ln),
                                               _p(ids)), "mc_nw_identity_strands")
        return ident, ln, ids

    def qgram_common(self, a, b, q, a_minus=None):
        """mc_qgram_common: the multiset q-gram intersection of nw_identity_strands' pairs (uint32;
        QGRAM_NA where a string holds a byte outside 0..3 or is shorter than q)."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        am = None if a_minus is None else np.ascontiguousarray(a_minus, np.uint8)
        assert len(a) == len(b) and (am is None or len(am) == len(a))
        out = np.zeros(len(a), np.uint32)
        self._ck(self.lib.mc_qgram_common(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(len(a)), int(q), _p(out)), "mc_qgram_common")
        return out

    def nw_align_strands(self, a, b, a_minus=None, cigar=True):
        """mc_nw_align_strands: the alignments behind nw_identity_strands -> (cigar, cig_off, score,
        len, ids).  ``cigar``: uint32 words run << 4 | op (CIGAR_I 1, CIGAR_D 2, CIGAR_EQ 7,
        CIGAR_X 8), pair i's at cig_off[i] .. cig_off[i + 1], in alignment order; ``len`` the
        alignment columns, ``ids`` the '=' columns.  ``cigar=False``: offsets and integers only
        (cigar is None)."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        am = None if a_minus is None else np.ascontiguousarray(a_minus, np.uint8)
        assert len(b) == len(a) and (am is None or len(am) == len(a))
        m = len(a)
        off = np.zeros(m + 1, np.uint64)
        sc = np.zeros(m, np.int32)
        ln = np.zeros(m, np.int32)
        ids = np.zeros(m, np.int32)
        if not cigar:
            self._ck(self.lib.mc_nw_align_strands(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(m), None, C.c_uint64(0), _p(off),
                                                _p(sc), _p(ln), _p(ids)), "mc_nw_align_strands")
            return None, off, sc, ln, ids
        cap = 0  # a word per base at most: the lengths, from mc_revcomp_sequences' offsets (no device work)
        for x in (a, b):
            self._ck(self.lib.mc_revcomp_sequences(self.ctx, _p(x), m, None, _p(off)), "mc_revcomp_sequences")
            cap += int(off[-1])
        words = np.zeros(cap, np.uint32)
        self._ck(self.lib.mc_nw_align_strands(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(m), _p(words), C.c_uint64(cap), _p(off),
                                            _p(sc), _p(ln), _p(ids)), "mc_nw_align_strands")
        return words[:int(off[-1])], off, sc, ln, ids

    def nw_align_profile(self, reset=False):
        """mc_nw_align_profile -> (forward ms, traceback ms, choice bytes) since the last reset."""
        out = np.zeros(3)
        self._ck(self.lib.mc_nw_align_profile(self.ctx, _p(out), 1 if reset else 0), "mc_nw_align_profile")
        return float(out[0]), float(out[1]), float(out[2])

    def set_align_band(self, mode):
        """mc_set_align_band: 0 (the default) the full choice record, 1 the certified band for nw_align_strands,
        nw_pileup_strands, nw_qpileup_strands and nw_msa_begin; their results do not change."""
        self._ck(self.lib.mc_set_align_band(self.ctx, int(mode)), "mc_set_align_band")

    def nw_band_plan(self, a, b, a_minus=None):
        """mc_nw_band_plan: the width search alone -> (w, score): the planned band width of every pair
        (-1: the full record) and its exact score."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        am = None if a_minus is None else np.ascontiguousarray(a_minus, np.uint8)
        assert len(b) == len(a) and (am is None or len(am) == len(a))
        w = np.zeros(len(a), np.int32)
        sc = np.zeros(len(a), np.int32)
        self._ck(self.lib.mc_nw_band_plan(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(len(a)), _p(w), _p(sc)), "mc_nw_band_plan")
        return w, sc

    def nw_band_profile(self, reset=False):
        """mc_nw_band_profile -> (pairs banded, pairs full, search launches, search ms, sum of the planned w)
        since the last reset."""
        out = np.zeros(5)
        self._ck(self.lib.mc_nw_band_profile(self.ctx, _p(out), 1 if reset else 0), "mc_nw_band_profile")
        return int(out[0]), int(out[1]), int(out[2]), float(out[3]), int(out[4])

    def nw_pileup_strands(self, a, b, a_minus, targets, table=True):
        """mc_nw_pileup_strands: nw_align_strands' alignments piled up per centre column ->
        (table[rows, 8], row_off, score, len, ids).  ``targets``: the distinct centres (every b among
        them); target t of L bytes owns rows row_off[t] .. row_off[t + 1] (L + 1 of them): channels
        0..3 the reads' digits over the column, 4 any other read byte, 5 deletions, 6 reads with an
        insertion before it, 7 the bases they insert.  ``table=False``: the offsets only (table is
        None, nothing is aligned)."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        am = None if a_minus is None else np.ascontiguousarray(a_minus, np.uint8)
        tg = np.ascontiguousarray(targets, np.uint32)
        assert len(b) == len(a) and (am is None or len(am) == len(a))
        m, nt = len(a), len(tg)
        off = np.zeros(nt + 1, np.uint64)
        sc = np.zeros(m, np.int32)
        ln = np.zeros(m, np.int32)
        ids = np.zeros(m, np.int32)
        self._ck(self.lib.mc_nw_pileup_strands(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(m), _p(tg), C.c_uint32(nt), _p(off), None,
                                             C.c_uint64(0), None, None, None), "mc_nw_pileup_strands")
        if not table:
            return None, off, sc, ln, ids
        rows = int(off[-1])
        tab = np.zeros((rows, PILEUP_CH), np.uint32)
        self._ck(self.lib.mc_nw_pileup_strands(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(m), _p(tg), C.c_uint32(nt), _p(off),
                                             _p(tab), C.c_uint64(rows), _p(sc), _p(ln), _p(ids)), "mc_nw_pileup_strands")
        return tab, off, sc, ln, ids

    def load_qualities(self, q):
        """mc_load_qualities: a Phred value (0 .. QUAL_MAX) per byte of the loaded sequences, at their
        offsets; the next load of sequences drops them."""
        q = np.ascontiguousarray(q, np.uint8)
        self._ck(self.lib.mc_load_qualities(self.ctx, _p(q), C.c_uint64(len(q))), "mc_load_qualities")

    def nw_qpileup_strands(self, a, b, a_minus, targets):
        """mc_nw_qpileup_strands: nw_pileup_strands with the loaded qualities summed beside the counts
        -> (table[rows, 8], wtable[rows, 8], row_off, score, len, ids).  ``wtable``: per column the
        qualities of the reads' bases by channel 0..4, channel 5 the deletions (the smaller quality
        of the two read bases around the gap), 6 the insertions (the smallest quality of the inserted
        bases), 7 zero; a minus pair's qualities run backwards."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        am = None if a_minus is None else np.ascontiguousarray(a_minus, np.uint8)
        tg = np.ascontiguousarray(targets, np.uint32)
        assert len(b) == len(a) and (am is None or len(am) == len(a))
        m, nt = len(a), len(tg)
        off = np.zeros(nt + 1, np.uint64)
        sc = np.zeros(m, np.int32)
        ln = np.zeros(m, np.int32)
        ids = np.zeros(m, np.int32)
        self._ck(self.lib.mc_nw_qpileup_strands(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(m), _p(tg), C.c_uint32(nt), _p(off), None,
                                              None, C.c_uint64(0), None, None, None), "mc_nw_qpileup_strands")
        rows = int(off[-1])
        tab = np.zeros((rows, PILEUP_CH), np.uint32)
        wtab = np.zeros((rows, PILEUP_CH), np.uint32)
        self._ck(self.lib.mc_nw_qpileup_strands(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(m), _p(tg), C.c_uint32(nt), _p(off),
                                              _p(tab), _p(wtab), C.c_uint64(rows), _p(sc), _p(ln), _p(ids)), "mc_nw_qpileup_strands")
        return tab, wtab, off, sc, ln, ids

    def nw_pileup_profile(self, reset=False):
        """mc_nw_pileup_profile -> (forward ms, traceback ms, pile-up ms) since the last reset."""
        out = np.zeros(3)
        self._ck(self.lib.mc_nw_pileup_profile(self.ctx, _p(out), 1 if reset else 0), "mc_nw_pileup_profile")
        return float(out[0]), float(out[1]), float(out[2])

    def nw_msa_begin(self, a, b, a_minus, targets):
        """mc_nw_msa_begin: nw_align_strands' alignments laid out in common columns per centre ->
        (row_off, width, block_width, score, len, ids).  ``targets``: the distinct centres (every b
        among them); target t of L bytes owns rows row_off[t] .. row_off[t + 1] (L + 1 of them);
        ``width[r]`` is the longest insertion any of its pairs has before centre base r (row L: after the
        last), ``block_width[t]`` = L + the sum of its widths, the length of every row of its block.
        The plan stays with the engine until the next begin, nw_msa_end or a load of sequences."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        am = None if a_minus is None else np.ascontiguousarray(a_minus, np.uint8)
        tg = np.ascontiguousarray(targets, np.uint32)
        assert len(b) == len(a) and (am is None or len(am) == len(a))
        m, nt = len(a), len(tg)
        off = np.zeros(nt + 1, np.uint64)
        self._ck(self.lib.mc_revcomp_sequences(self.ctx, _p(tg), C.c_uint64(nt), None, _p(off)), "mc_revcomp_sequences")
        width = np.zeros(int(off[-1]) + nt, np.uint32)  # (the targets' lengths, no device work: L + 1 rows each)
        bw = np.zeros(nt, np.uint64)
        sc = np.zeros(m, np.int32)
        ln = np.zeros(m, np.int32)
        ids = np.zeros(m, np.int32)
        self._ck(self.lib.mc_nw_msa_begin(self.ctx, _p(a), _p(b), _p(am), C.c_uint64(m), _p(tg), C.c_uint32(nt), _p(off), _p(width),
                                        _p(bw), _p(sc), _p(ln), _p(ids)), "mc_nw_msa_begin")
        return off, width, bw, sc, ln, ids

    def nw_msa_rows(self, first, count, rows=True):
        """mc_nw_msa_rows: rows first .. first + count of the plan (row k < nt: target k's centre row;
        row nt + i: pair i's) -> (bytes, off): row k's characters are bytes[off[k] .. off[k + 1]), gaps
        MSA_GAP.  ``rows=False``: the offsets only (bytes is None, no device work)."""
        off = np.zeros(count + 1, np.uint64)
        self._ck(self.lib.mc_nw_msa_rows(self.ctx, C.c_uint64(first), C.c_uint64(count), None, C.c_uint64(0), _p(off)), "mc_nw_msa_rows")
        if not rows:
            return None, off
        out = np.zeros(int(off[-1]), np.uint8)
        self._ck(self.lib.mc_nw_msa_rows(self.ctx, C.c_uint64(first), C.c_uint64(count), _p(out), C.c_uint64(len(out)), _p(off)),
                 "mc_nw_msa_rows")
        return out, off

    def nw_msa_end(self):
        """mc_nw_msa_end: drop the plan and free its device buffers."""
        self._ck(self.lib.mc_nw_msa_end(self.ctx), "mc_nw_msa_end")

    def nw_msa_profile(self, reset=False):
        """mc_nw_msa_profile -> (forward ms, traceback ms, width + column ms, render ms) since the last reset."""
        out = np.zeros(4)
        self._ck(self.lib.mc_nw_msa_profile(self.ctx, _p(out), 1 if reset else 0), "mc_nw_msa_profile")
        return tuple(float(x) for x in out)

    def nw_msa_counts(self, first, count, weights=False, counts=True):
        """mc_nw_msa_counts: the column profile of targets first .. first + count of the plan ->
        (col_off, counts[columns, 8]) or, with ``weights`` (qualities loaded), (col_off, counts, wcounts).
        Target t's columns are col_off[t] .. col_off[t + 1].  counts: channels 0..4 the rows' bytes by
        class (A C G T other), 5 the rows with a gap, 6 the centre position or insertion site r, 7 zero
        for a centre column and the 1-based slot for an inserted one; the centre row is not counted.
        wcounts: the qualities summed over the same bytes (channel 5 of a centre column: the deletions'
        weights as in nw_qpileup_strands; channels 6 and 7 zero).  ``counts=False``: (col_off,) only, no
        device work."""
        off = np.zeros(count + 1, np.uint64)
        self._ck(self.lib.mc_nw_msa_counts(self.ctx, C.c_uint32(first), C.c_uint32(count), _p(off), None, None, C.c_uint64(0)),
                 "mc_nw_msa_counts")
        if not counts:
            return (off,)
        cols = int(off[-1])
        tab = np.zeros((cols, MSA_CH), np.uint32)
        wtab = np.zeros((cols, MSA_CH), np.uint32) if weights else None
        self._ck(self.lib.mc_nw_msa_counts(self.ctx, C.c_uint32(first), C.c_uint32(count), _p(off), _p(tab), _p(wtab), C.c_uint64(cols)),
                 "mc_nw_msa_counts")
        return (off, tab, wtab) if weights else (off, tab)

    def nw_msa_counts_profile(self, reset=False):
        """mc_nw_msa_counts_profile -> device ms of nw_msa_counts' kernels since the last reset."""
        out = np.zeros(1)
        self._ck(self.lib.mc_nw_msa_counts_profile(self.ctx, _p(out), 1 if reset else 0), "mc_nw_msa_counts_profile")
        return float(out[0])

    def nw_msa_sites(self, site_off, sites, first, count, quals=False, alleles=True):
        """mc_nw_msa_sites: what pairs first .. first + count of the plan carry at chosen columns of
        their targets' blocks -> (off, alleles) or, with ``quals`` (qualities loaded), (off, alleles,
        quals).  Target t's sites are sites[site_off[t] .. site_off[t + 1]), strictly ascending
        columns of its block; pair k's bytes are alleles[off[k] .. off[k + 1]): its nw_msa_rows row at
        those columns, gaps MSA_GAP.  quals: the weight the pair adds to that column of nw_msa_counts'
        wcounts.  ``alleles=False``: (off,) only, no device work."""
        so = np.ascontiguousarray(site_off, np.uint64)
        st = np.ascontiguousarray(sites, np.uint32)
        off = np.zeros(count + 1, np.uint64)
        self._ck(self.lib.mc_nw_msa_sites(self.ctx, _p(so), _p(st), C.c_uint64(first), C.c_uint64(count), None, None, C.c_uint64(0),
                                        _p(off)), "mc_nw_msa_sites")
        if not alleles:
            return (off,)
        n = int(off[-1])
        al = np.zeros(n, np.uint8)
        ql = np.zeros(n, np.uint8) if quals else None
        self._ck(self.lib.mc_nw_msa_sites(self.ctx, _p(so), _p(st), C.c_uint64(first), C.c_uint64(count), _p(al), _p(ql), C.c_uint64(n),
                                        _p(off)), "mc_nw_msa_sites")
        return (off, al, ql) if quals else (off, al)

    def nw_msa_sites_profile(self, reset=False):
        """mc_nw_msa_sites_profile -> device ms of nw_msa_sites' kernels since the last reset."""
        out = np.zeros(1)
        self._ck(self.lib.mc_nw_msa_sites_profile(self.ctx, _p(out), 1 if reset else 0), "mc_nw_msa_sites_profile")
        return float(out[0])

    def nw_msa_crossover(self, x, y):
        """mc_nw_msa_crossover: for candidates (x[c], y[c]), two pairs of the plan that align the same read,
        -> (nc, CROSS_RES) int32: ids_x, ids_y, best_xy (x left of the cut, y right) with its smallest and
        largest cut, best_yx (y left, x right) with its smallest and largest cut.  Cuts are positions in
        the read as written, 0 .. its length."""
        x = np.ascontiguousarray(x, np.uint64)
        y = np.ascontiguousarray(y, np.uint64)
        if x.shape != y.shape or x.ndim != 1:
            raise ValueError("nw_msa_crossover: x and y are two lists of one length")
        out = np.zeros((len(x), CROSS_RES), np.int32)
        self._ck(self.lib.mc_nw_msa_crossover(self.ctx, _p(x), _p(y), C.c_uint64(len(x)), _p(out)), "mc_nw_msa_crossover")
        return out

    def nw_msa_crossover_profile(self, reset=False):
        """mc_nw_msa_crossover_profile -> device ms of nw_msa_crossover's kernel since the last reset."""
        out = np.zeros(1)
        self._ck(self.lib.mc_nw_msa_crossover_profile(self.ctx, _p(out), 1 if reset else 0), "mc_nw_msa_crossover_profile")
        return float(out[0])

    def derep(self, ids, strands=MC_STRAND_PLUS):
        """mc_derep: the duplicates among the points ``ids`` (equal expanded byte strings; with
        ``strands=MC_STRAND_PLUS | MC_STRAND_MINUS`` also a string and its minus-strand string) -> (rep uint32,
        minus uint8): rep[i] the smallest position of the list whose point is a duplicate of ids[i]'s,
        minus[i] 0 where the two strings are equal as written (this wins), else 1.  Exact; on the GPU only."""
        ids = np.ascontiguousarray(ids, np.uint32)
        rep = np.zeros(len(ids), np.uint32)
        minus = np.zeros(len(ids), np.uint8)
        self._ck(self.lib.mc_derep(self.ctx, _p(ids), C.c_uint64(len(ids)), int(strands), _p(rep), _p(minus)), "mc_derep")
        return rep, minus

    def derep_profile(self, reset=False):
        """mc_derep_profile -> dict since the last reset: device ms of the fingerprint and of the compare
        kernel, pairs compared, compare rounds, collisions (pairs whose compare said "not equal")."""
        out = np.zeros(5)
        self._ck(self.lib.mc_derep_profile(self.ctx, _p(out), 1 if reset else 0), "mc_derep_profile")
        return {"fingerprint_ms": float(out[0]), "compare_ms": float(out[1]), "pairs": int(out[2]), "rounds": int(out[3]),
                "collisions": int(out[4])}

    def nw_identity_raw(self, a_cat, a_off, b_cat, b_off):
        a_cat = np.ascontiguousarray(a_cat, np.uint8)
        b_cat = np.ascontiguousarray(b_cat, np.uint8)
        a_off = np.ascontiguousarray(a_off, np.uint64)
        b_off = np.ascontiguousarray(b_off, np.uint64)
        m = len(a_off) - 1
        ident = np.zeros(m)
        ln = np.zeros(m, np.int32)
        ids = np.zeros(m, np.int32)
        sc = np.zeros(m, np.int32)
        self._ck(self.lib.mc_nw_identity_raw(self.ctx, _p(a_cat), _p(a_off), _p(b_cat), _p(b_off), C.c_uint64(m),
                                           _p(ident), _p(ln), _p(ids), _p(sc)), "mc_nw_identity_raw")
        return ident, ln, ids, sc

    def sync(self):
        """Wait for all work on this context's GPU (mc_sync)."""
        self._ck(self.lib.mc_sync(self.ctx), "mc_sync")

    def timers(self, reset=False):
        out = np.zeros(2 * len(FAMILIES))
        self._ck(self.lib.mc_timers(self.ctx, _p(out), len(out), 1 if reset else 0), "mc_timers")
        return {f: (out[2 * i], int(out[2 * i + 1])) for i, f in enumerate(FAMILIES)}


def assign_files(engine, model, centres, reads, out, unassigned=None, threads=8, both_strands=False, top=None, hits=None,
                 identity=False, min_identity=None, paf=None, consensus=None, pileup=None, quality=False, msa=None, profile=None,
                 band=False, variants=None, alleles=None, haplotypes=None, min_allele_frac=0.2, min_allele_count=2,
                 chimeras=None, min_chimera_gain=3):
    """Place the reads of the FASTA or FASTQ file(s) ``reads`` into the clustering saved by
    ``meshclust --save-model model --save-centres centres`` (mcl_assign: mc_assign on the
    engine's GPU).  Writes the TSV ``out`` (read, centre or *, cluster index or -1, combo 0,
    similar centres) and, if given, the unassigned reads as FASTA; returns the stats dict.
    ``both_strands``: meshclust-assign's --both-strands (mcl_assign_strands): every read is scored
    as written and reverse-complemented, the TSV gains a strand column (+, -, * unassigned) and
    the stats ``strands`` and ``assigned_minus``.
    ``top`` and ``hits`` (given together): meshclust-assign's --top K --hits FILE (mcl_assign_top): the
    file ``hits`` gets one line per hit of the ``top`` best similar centres of every read (read, rank,
    centre, cluster index, combo 0, and the strand with ``both_strands``); the TSV does not change,
    the stats gain ``top`` and ``hits``.
    ``identity`` / ``min_identity``: meshclust-assign's --identity and --min-identity X
    (mcl_assign_identity): every reported (read, centre, strand) is aligned, the TSV and the hits file
    gain a last column with the identity (* for an unassigned read); with ``min_identity`` a read goes
    to the first of its hits that aligns at that identity or more, else it is unassigned.  The stats
    gain ``identity_pairs``, ``identity_cells``, ``rejected`` and the ``identity`` phase.
    ``paf``: meshclust-assign's --paf FILE (mcl_assign_paf; implies ``identity``): one PAF line with a
    CIGAR (cg:Z:, = X I D) per aligned pair; the stats gain ``paf_pairs`` and ``cigar_ops``.
    ``consensus`` / ``pileup``: meshclust-assign's --consensus FILE and --pileup FILE (mcl_assign_consensus;
    either implies ``identity``): every assigned read is piled up on its centre (mc_nw_pileup_strands);
    ``consensus`` gets every centre's consensus as FASTA, ``pileup`` the per-column counts of the centres
    with reads; the stats gain ``consensus_pairs``, ``consensus_centres``, ``consensus_passes``,
    ``realigned_centres`` and ``insertion_sites``.
    ``quality``: meshclust-assign's --quality (mcl_assign_qconsensus; with ``consensus`` and/or ``pileup``, every
    reads file FASTQ): the pile-up is weighed by base quality (mc_nw_qpileup_strands), ``consensus`` is written
    as FASTQ with a quality per base, the ``pileup`` rows gain wA wC wG wT wN wdel, the stats ``quality``.
    ``msa``: meshclust-assign's --msa FILE (mcl_assign_msa; implies ``identity``): the assigned reads of every centre
    laid out in common columns (mc_nw_msa_begin / mc_nw_msa_rows) as aligned FASTA, a pass of its own that changes
    no other output; the stats gain, last, ``msa_pairs``, ``msa_centres``, ``msa_columns``, ``msa_bytes`` and the
    ``msa`` phase.
    ``profile``: meshclust-assign's --profile FILE (mcl_assign_profile; implies ``identity``): that alignment counted
    per column (mc_nw_msa_counts; one mc_nw_msa_begin shared with ``msa``) as a TSV, one line per column of every
    centre with reads: centre, column, centre_pos, slot, base, depth, A, C, G, T, N, gap, and with ``quality`` (then
    accepted beside ``profile`` alone) wA wC wG wT wN wgap; the stats gain, last, ``profile_centres``,
    ``profile_columns`` and the ``profile`` phase.
    ``band``: meshclust-assign's --band (mcl_assign_band; with ``paf``, ``consensus``, ``pileup``, ``msa`` or
    ``profile``): the alignments record the certified band alone (mc_set_align_band 1 for the run); no output
    file changes, the stats gain, last, ``band_pairs``, ``band_full``, ``band_launches`` and ``band_w_sum``.
    ``variants`` / ``alleles`` / ``haplotypes``: meshclust-assign's --variants FILE, --alleles FILE and --haplotypes FILE
    (mcl_assign_variants; each implies ``identity``; they share ``msa``'s and ``profile``'s mc_nw_msa_begin): the
    ``profile`` lines of every centre's variant sites -- the columns whose second most frequent allele (A, C, G, T or
    gap) is seen ``min_allele_count`` times or more and in ``min_allele_frac`` of the rows or more --, one line per
    assigned read with its characters at its centre's sites (mc_nw_msa_sites; with ``quality`` their weights too),
    and per centre with a site its distinct allele strings: centre, rank, count, depth, alleles.  ``quality`` and
    ``band`` are accepted beside any of the three.  The stats gain, last, ``variant_centres``, ``variant_sites``,
    ``allele_bytes`` and the ``variants`` phase.
    ``chimeras``: meshclust-assign's --chimeras FILE (mcl_assign_chimeras; needs ``top`` of 2 or more, implies
    ``identity``): after every other output, every read's hits are aligned again in plans of their own and its best
    hit is compared with every later hit of another centre (mc_nw_msa_crossover): one line per read with such a hit
    -- read, left_centre, right_centre, left_strand, right_strand, cut_first, cut_last, ids_left, ids_right, best, gain,
    read_len, flag -- for the second parent of largest gain; flag is Y where the gain is ``min_chimera_gain`` or more
    (default 3: a convention, not tuned on real data).  ``band`` is accepted beside it.  The stats gain, last,
    ``chimera_candidates``, ``chimeras`` and the ``chimeras`` phase."""
    import json
    lib = host_lib()
    files = [reads] if isinstance(reads, str) else list(reads)
    arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
    buf = C.create_string_buffer(1 << 14)
    enc = lambda x: x.encode() if x else None
    if chimeras is not None:
        rc = lib.mcl_assign_chimeras(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                     enc(unassigned), 1 if both_strands else 0, int(top or 0), enc(hits), 1,
                                     -1.0 if min_identity is None else float(min_identity), enc(paf), enc(consensus), enc(pileup),
                                     1 if quality else 0, enc(msa), enc(profile), 1 if band else 0, enc(variants), enc(alleles),
                                     enc(haplotypes), float(min_allele_frac), int(min_allele_count), enc(chimeras),
                                     int(min_chimera_gain), buf, len(buf))
    elif variants is not None or alleles is not None or haplotypes is not None:
        rc = lib.mcl_assign_variants(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                     enc(unassigned), 1 if both_strands else 0, int(top or 0), enc(hits), 1,
                                     -1.0 if min_identity is None else float(min_identity), enc(paf), enc(consensus), enc(pileup),
                                     1 if quality else 0, enc(msa), enc(profile), 1 if band else 0, enc(variants), enc(alleles),
                                     enc(haplotypes), float(min_allele_frac), int(min_allele_count), buf, len(buf))
    elif band:
        rc = lib.mcl_assign_band(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                 unassigned.encode() if unassigned else None, 1 if both_strands else 0, int(top or 0),
                                 hits.encode() if hits else None, 1, -1.0 if min_identity is None else float(min_identity),
                                 paf.encode() if paf else None, consensus.encode() if consensus else None,
                                 pileup.encode() if pileup else None, 1 if quality else 0, msa.encode() if msa else None,
                                 profile.encode() if profile else None, 1, buf, len(buf))
    elif profile is not None:
        rc = lib.mcl_assign_profile(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                    unassigned.encode() if unassigned else None, 1 if both_strands else 0, int(top or 0),
                                    hits.encode() if hits else None, 1, -1.0 if min_identity is None else float(min_identity),
                                    paf.encode() if paf else None, consensus.encode() if consensus else None,
                                    pileup.encode() if pileup else None, 1 if quality else 0, msa.encode() if msa else None,
                                    profile.encode(), buf, len(buf))
    elif msa is not None:
        rc = lib.mcl_assign_msa(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                unassigned.encode() if unassigned else None, 1 if both_strands else 0, int(top or 0),
                                hits.encode() if hits else None, 1, -1.0 if min_identity is None else float(min_identity),
                                paf.encode() if paf else None, consensus.encode() if consensus else None,
                                pileup.encode() if pileup else None, 1 if quality else 0, msa.encode(), buf, len(buf))
    elif quality:
        rc = lib.mcl_assign_qconsensus(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                       unassigned.encode() if unassigned else None, 1 if both_strands else 0, int(top or 0),
                                       hits.encode() if hits else None, 1, -1.0 if min_identity is None else float(min_identity),
                                       paf.encode() if paf else None, consensus.encode() if consensus else None,
                                       pileup.encode() if pileup else None, 1, buf, len(buf))
    elif consensus is not None or pileup is not None:
        rc = lib.mcl_assign_consensus(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                      unassigned.encode() if unassigned else None, 1 if both_strands else 0, int(top or 0),
                                      hits.encode() if hits else None, 1, -1.0 if min_identity is None else float(min_identity),
                                      paf.encode() if paf else None, consensus.encode() if consensus else None,
                                      pileup.encode() if pileup else None, buf, len(buf))
    elif paf is not None:
        rc = lib.mcl_assign_paf(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                unassigned.encode() if unassigned else None, 1 if both_strands else 0, int(top or 0),
                                hits.encode() if hits else None, 1, -1.0 if min_identity is None else float(min_identity),
                                paf.encode(), buf, len(buf))
    elif identity or min_identity is not None:
        rc = lib.mcl_assign_identity(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                     unassigned.encode() if unassigned else None, 1 if both_strands else 0, int(top or 0),
                                     hits.encode() if hits else None, 1 if identity else 0,
                                     -1.0 if min_identity is None else float(min_identity), buf, len(buf))
    elif top is not None or hits is not None:
        rc = lib.mcl_assign_top(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                unassigned.encode() if unassigned else None, 1 if both_strands else 0, int(top or 0),
                                hits.encode() if hits else None, buf, len(buf))
    elif both_strands:
        rc = lib.mcl_assign_strands(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                                    unassigned.encode() if unassigned else None, 1, buf, len(buf))
    else:
        rc = lib.mcl_assign(engine.ctx, model.encode(), centres.encode(), arr, len(files), threads, out.encode(),
                            unassigned.encode() if unassigned else None, buf, len(buf))
    st = json.loads(buf.value.decode() or "{}")
    if rc != 0 or "error" in st:
        raise MCError("mcl_assign failed (%d): %s" % (rc, st.get("error", st)))
    return st


def derep_files(engine, reads, out, table=None, both_strands=False, min_size=1, threads=8):
    """meshclust-derep on the engine's GPU (mcl_derep: mc_derep over all reads of the FASTA or FASTQ file(s)
    ``reads``).  ``out`` gets one FASTA record per class of identical reads -- with ``both_strands`` a read and its
    reverse complement are identical too --, the class's first read in input order, its header extended by
    ``;size=N``, most abundant first (ties: the earlier first read); classes of fewer than ``min_size`` reads are
    left out.  ``table``, if given, gets one line per read in input order: read, representative, strand (+ or -),
    size.  Returns the stats dict: reads, uniques, written, largest, minus, strands, compare_pairs, rounds,
    collisions, phases_ms."""
    import json
    lib = host_lib()
    files = [reads] if isinstance(reads, str) else list(reads)
    arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
    buf = C.create_string_buffer(1 << 12)
    rc = lib.mcl_derep(engine.ctx, arr, len(files), threads, out.encode(), table.encode() if table else None,
                       1 if both_strands else 0, int(min_size), buf, len(buf))
    st = json.loads(buf.value.decode() or "{}")
    if rc != 0 or "error" in st:
        e = MCError("mcl_derep failed (%d): %s" % (rc, st.get("error", st)))
        e.code = rc
        raise e
    return st


def derep_host(codes, seq_off, ids, strands=MC_STRAND_PLUS):
    """derep_host of libmeshclust (host/derep.hpp): mc_derep's contract computed on the CPU from the expanded
    bytes ``codes`` and their offsets -> (rep, minus).  No fallback of ``Engine.derep``: the benchmark's host route."""
    codes = np.ascontiguousarray(codes, np.uint8)
    seq_off = np.ascontiguousarray(seq_off, np.uint64)
    ids = np.ascontiguousarray(ids, np.uint32)
    rep = np.zeros(len(ids), np.uint32)
    minus = np.zeros(len(ids), np.uint8)
    if len(ids) and int(ids.max()) + 1 >= len(seq_off):
        raise ValueError("derep_host: id out of range")
    rc = host_lib().mcl_derep_host(_p(codes), _p(seq_off), _p(ids), C.c_uint64(len(ids)), int(strands), _p(rep), _p(minus))
    if rc != 0:
        raise MCError("mcl_derep_host failed (%d)" % rc)
    return rep, minus


class Dataset:
    """Parsed FASTA / FASTQ files held by libmeshclust (one parse, many GPU runs).  A file whose
    first non-empty line starts with '@' is FASTQ; ``qualities=True`` (mcl_parse_q) keeps its
    qualities for ``qualities()``."""

    def __init__(self, files, threads=8, qualities=False):
        self.lib = host_lib()
        self.h = None
        arr = (C.c_char_p * len(files))(*[f.encode() for f in files])
        err = C.create_string_buffer(1024)
        self.h = (self.lib.mcl_parse_q if qualities else self.lib.mcl_parse)(arr, len(files), threads, err, 1024)
        if not self.h:
            raise MCError("parse failed: " + err.value.decode())
        self.n = self.lib.mcl_num_seqs(self.h)

    def qualities(self):
        """mcl_qualities -> the Phred values (uint8, 0..93), one per expanded byte at seq_off (0 for
        the records of FASTA files); None if the dataset was parsed without ``qualities=True``."""
        q, n = C.c_void_p(), C.c_uint64()
        self.lib.mcl_qualities(self.h, C.byref(q), C.byref(n))
        if not q.value:
            return None
        return np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()

    def records(self):
        """[(header, codes uint8, [[start, end], ...])] as parsed (ChromListMaker +
        Chromosome::help + ChromosomeOneDigit encoding)."""
        ptr = [C.c_void_p() for _ in range(4)]
        self.lib.mcl_view(self.h, *[C.byref(p) for p in ptr])
        n = self.n

        def arr(p, ct, count):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(count,)) if count else np.zeros(0)

        seq_off = arr(ptr[1], C.c_uint64, n + 1).copy()
        seg_off = arr(ptr[3], C.c_uint64, n + 1).copy()
        codes = arr(ptr[0], C.c_uint8, int(seq_off[-1])).copy()
        seg = arr(ptr[2], C.c_int32, 2 * int(seg_off[-1])).copy()
        out = []
        for i in range(n):
            s = seg[2 * int(seg_off[i]):2 * int(seg_off[i + 1])]
            out.append((self.lib.mcl_header(self.h, i).decode(), codes[int(seq_off[i]):int(seq_off[i + 1])],
                        [[int(s[j]), int(s[j + 1])] for j in range(0, len(s), 2)]))
        return out

    def label_identities(self, engine, a, b, both_strands=False):
        """mcl_label_identities: the identities the trainer labels the pairs (a[i], b[i]) with (its
        only alignment seam); ``both_strands``: max(identity(a, b), identity(rc(a), b)), what a
        ``--both-strands`` run trains on.  The dataset's sequences must be loaded in ``engine``."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        assert len(a) == len(b)
        out = np.zeros(len(a))
        err = C.create_string_buffer(1024)
        self.lib.mcl_label_identities.restype = C.c_int
        self.lib.mcl_label_identities.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int,
                                                  C.c_void_p, C.c_char_p, C.c_int]
        rc = self.lib.mcl_label_identities(self.h, engine.ctx, _p(a), _p(b), len(a), 1 if both_strands else 0, _p(out),
                                           err, 1024)
        if rc != 0:
            raise MCError("mcl_label_identities failed (%d): %s" % (rc, err.value.decode()))
        return out

    def qscreen_common(self, a, b, q, a_minus=None):
        """mcl_qscreen_common: host/qscreen.hpp's count of the pairs, the host twin of
        Engine.qgram_common, from the parsed 2-bit words."""
        a = np.ascontiguousarray(a, np.uint32)
        b = np.ascontiguousarray(b, np.uint32)
        am = None if a_minus is None else np.ascontiguousarray(a_minus, np.uint8)
        assert len(a) == len(b) and (am is None or len(am) == len(a))
        out = np.zeros(len(a), np.uint32)
        self.lib.mcl_qscreen_common.restype = C.c_int
        self.lib.mcl_qscreen_common.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        if self.lib.mcl_qscreen_common(self.h, _p(a), _p(b), _p(am), len(a), int(q), _p(out)) != 0:
            raise MCError("mcl_qscreen_common: pair id out of range")
        return out

    def run(self, engine, args=(), upload=True, clstr=None, comm=None):
        """Run the full pipeline (reference options in ``args``); returns the stats dict.
        ``comm`` (meshclust_amd.dist.RcclShardComm or TorchShardComm) shares the clustering
        over its ranks."""
        import json
        argv = [b"meshclust"] + [a.encode() for a in args]
        arr = (C.c_char_p * len(argv))(*argv)
        buf = C.create_string_buffer(1 << 16)
        if comm is not None:
            rc = self.lib.mcl_run_sharded(self.h, engine.ctx, len(argv), arr, 1 if upload else 0,
                                          clstr.encode() if clstr else None, buf, len(buf), comm.rank, comm.world,
                                          C.cast(comm.callback, C.c_void_p), comm.user)
        else:
            rc = self.lib.mcl_run(self.h, engine.ctx, len(argv), arr, 1 if upload else 0,
                                  clstr.encode() if clstr else None, buf, len(buf))
        st = json.loads(buf.value.decode() or "{}")
        if rc != 0 or "error" in st:  # incl. the reference's exit(0) stops (no partition)
            raise MCError("mcl_run failed (%d): %s" % (rc, st))
        if upload:  # the engine now holds this dataset's sequences (histograms() sizes its arrays by n)
            engine.n = self.n
        engine.width, engine.B = st.get("width", engine.width), 4 ** st["k"] if "k" in st else engine.B
        return st

    def __del__(self):
        try:
            self.lib.mcl_free(self.h)
        except Exception:
            pass
