"""ctypes binding of librbl_hip.so (include/rbl_hip.h).

The library is the only compute path: if it is missing this module raises ImportError —
there is no CPU fallback anywhere in the product.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RBL_LIB: a diagnostics build of the same library (tools/build_variant.sh)
LIB_PATH = os.environ.get("RBL_LIB") or os.path.join(_HERE, "librbl_hip.so")

RBL_OK = 0
RBL_WARN_NOT_CONVERGED = 1
RBL_WARN_QR_SHIFTED = 2
RBL_ERR_INVALID = -1
RBL_ERR_HIP = -2
RBL_ERR_OOM = -3
RBL_ERR_RCCL = -4
RBL_ERR_STATE = -5
RBL_ERR_NUMERIC = -6

RBL_MAX_BLOCK = 512          # the largest block width b of any entry point

RBL_OPT_TIMERS = 0
RBL_OPT_REORTH_ORDER = 1
RBL_OPT_SPMM_KERNEL = 2
RBL_OPT_DEVICE_BLOCKS = 3
RBL_OPT_SPLIT_HALO = 4
RBL_OPT_KEEP_CSR = 5
RBL_OPT_FUSE = 6
RBL_OPT_HALO_OVERLAP = 7
RBL_OPT_RELABEL = 8
RBL_OPT_HALO_PUSH = 9
RBL_OPT_CLOC_DERIVE = 10
RBL_OPT_UPD32 = 11
RBL_OPT_UPD32_SHADOW = 12
# rbl_path_stats entries
RBL_PATH_SPMM = 0
RBL_PATH_SPMM_LOC_FUSED = 1
RBL_PATH_LOC_SEPARATE = 2
RBL_PATH_LOC_GRAM = 3
RBL_PATH_LOCFIX_EDGES = 4
RBL_PATH_LOCFIX_REST = 5
RBL_PATH_SPMM_TWO_WAVE = 6
RBL_PATH_RITZ_PIECES = 7
RBL_PATH_CLOC_3TERM = 8
RBL_PATH_CLOC_REORTH = 9
RBL_PATH_UPD32_TAKEN = 10
RBL_PATH_UPD32_REFUSED = 11
RBL_PATH_UPD32_SHADOW_READ = 12
RBL_PATH_UPD32_SHADOW_CONV = 13
RBL_PATH_UPD32_SHADOW_BYTES = 14
RBL_PATH_NSTATS = 15
RBL_BUILD_VARIANTS = 1
# a rectangular B (rbl_set_matrix_normal): what rbl_spmm_kernel_for / rbl_matrix_format report
RBL_SPMM_KERNEL_RECT = 8
RBL_MATRIX_FORMAT_RECT = 5
# an implicit kernel matrix (rbl_set_matrix_kernel): the kernels, the largest d, and what
# rbl_spmm_kernel_for / rbl_matrix_format report
RBL_KERNEL_RBF = 0
RBL_KERNEL_LAPLACE = 1
RBL_KERNEL_POLY = 2
RBL_KERNOP_MAX_DIM = 256
RBL_SPMM_KERNEL_KERNOP = 9
RBL_MATRIX_FORMAT_KERNOP = 6
# rbl_kernel_hadamard: the weight Phi (kappa, d kappa / d gamma, the factor of d kappa / d log s_k)
RBL_KWEIGHT_VALUE = 0
RBL_KWEIGHT_DGAMMA = 1
RBL_KWEIGHT_DSCALE = 2
# rbl_kernel_knn: the largest k
RBL_KNN_MAX = 64
# rbl_kernel_pchol: the largest rank
RBL_PCHOL_MAX_RANK = 256
# rbl_kmeans_run / rbl_kmeans_seed: the largest number of clusters
RBL_KMEANS_MAX_CLUSTERS = 256
# rbl_cheb_diag: the block drawn when X is NULL
RBL_PROBE_GAUSS = 0
RBL_PROBE_SIGN = 1
# rbl_solve: the per-column status
RBL_SOLVE_CONVERGED = 0
RBL_SOLVE_MAX_ITER = 1
RBL_SOLVE_NOT_POSDEF = 2
# rbl_thick_restart: the most columns keep_blocks * b the in-place compression keeps
RBL_COMPRESS_MAX_COLS = 512

_p = C.c_void_p
_i64 = C.c_int64
_u64 = C.c_uint64
_pd = C.POINTER(C.c_double)
_pi64 = C.POINTER(C.c_int64)
_pi32 = C.POINTER(C.c_int32)
_pu8 = C.POINTER(C.c_uint8)

# name -> (restype, argtypes); the complete export list of include/rbl_hip.h
SIGNATURES = {
    "rbl_abi_version": (C.c_int, []),
    "rbl_build_flags": (C.c_int, []),
    "rbl_create": (C.c_int, [C.POINTER(_p), C.c_int]),
    "rbl_get_unique_id": (C.c_int, [_pu8]),
    "rbl_create_dist": (C.c_int, [C.POINTER(_p), C.c_int, C.c_int, C.c_int, _pu8]),
    "rbl_local_group_create": (C.c_int, [C.POINTER(_p), C.c_int]),
    "rbl_local_group_free": (C.c_int, [_p]),
    "rbl_create_local": (C.c_int, [C.POINTER(_p), C.c_int, _p, C.c_int]),
    "rbl_create_shm": (C.c_int, [C.POINTER(_p), C.c_int, C.c_int, C.c_int, C.c_char_p]),
    "rbl_free": (C.c_int, [_p]),
    "rbl_last_error": (C.c_char_p, [_p]),
    "rbl_comm_info": (C.c_int, [_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "rbl_rccl_version": (C.c_int, [C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    "rbl_set_option": (C.c_int, [_p, C.c_int, _i64]),
    "rbl_device_memory": (C.c_int, [_p, _pi64, _pi64]),
    "rbl_set_matrix_csc": (C.c_int, [_p, _i64, _i64, _pi64, _pi64, _pd, C.c_int]),
    "rbl_set_matrix_csr_rows": (C.c_int, [_p, _i64, _i64, _i64, _pi64, _pi64, _pd, C.c_int]),
    "rbl_set_matrix_dense": (C.c_int, [_p, _i64, _i64, _i64, _pd, _i64]),
    "rbl_set_matrix_normal": (C.c_int, [_p, _i64, _i64, _i64, _pi64, _pi64, _pd, C.c_int, C.c_int]),
    "rbl_rect_info": (C.c_int, [_p, _pi64, _pi64, _pi64]),
    "rbl_get_matrix_rect": (C.c_int, [_p, C.c_int, _pi64, _pi32, _pd]),
    "rbl_apply_rect": (C.c_int, [_p, C.c_int, C.c_int, _pd, _pd]),
    "rbl_left_vectors": (C.c_int, [_p, C.c_int, _pd, _pd, _pd]),
    "rbl_set_rect_shift": (C.c_int, [_p, _pd, _pd]),
    "rbl_get_rect_shift": (C.c_int, [_p, _pd, _pd]),
    "rbl_apply_rect_shifted": (C.c_int, [_p, C.c_int, C.c_int, _pd, _pd]),
    "rbl_set_matrix_kernel": (C.c_int, [_p, _i64, C.c_int, _pd, _i64, C.c_int, C.c_double, C.c_double,
                                        C.c_int]),
    "rbl_set_kernel_scale": (C.c_int, [_p, _pd, C.c_double]),
    "rbl_kernel_info": (C.c_int, [_p, _pi64, C.POINTER(C.c_int), C.POINTER(C.c_int), _pd, _pd,
                                  C.POINTER(C.c_int), C.POINTER(C.c_int), _pd]),
    "rbl_bench_kernel_pass": (C.c_int, [_p, C.c_int, C.c_int, _pd]),
    "rbl_kernel_cross": (C.c_int, [_p, _i64, _pd, _i64, C.c_int, C.c_int, _pd, _i64, _pd, _i64]),
    "rbl_kernel_cross_splits": (C.c_int, [_i64, _i64, C.c_int]),
    "rbl_bench_kernel_cross": (C.c_int, [_p, _i64, _pd, _i64, C.c_int, C.c_int, C.c_int, C.c_int, _pd]),
    "rbl_kernel_knn": (C.c_int, [_p, _i64, _pd, _i64, C.c_int, C.c_int, _pi32, _i64, _pd, _i64]),
    "rbl_bench_kernel_knn": (C.c_int, [_p, _i64, _pd, _i64, C.c_int, C.c_int, C.c_int, _pd]),
    "rbl_kernel_pchol": (C.c_int, [_p, C.c_int, C.c_double, _pd, _i64, _pi32, _pd, C.POINTER(C.c_int)]),
    "rbl_bench_kernel_pchol": (C.c_int, [_p, C.c_int, C.c_int, _pd]),
    "rbl_kernel_hadamard": (C.c_int, [_p, C.c_int, C.c_int, _pd, _i64, _pd, _i64, C.c_int, _pd, _i64, _pd, _i64]),
    "rbl_bench_kernel_hadamard": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, C.c_int, _pd]),
    "rbl_kmeans_set_points": (C.c_int, [_p, _i64, C.c_int, _pd, _i64]),
    "rbl_kmeans_clear": (C.c_int, [_p]),
    "rbl_kmeans_seed": (C.c_int, [_p, C.c_int, _pd, _pi32]),
    "rbl_kmeans_run": (C.c_int, [_p, C.c_int, _pd, _i64, C.c_int, C.c_double, _pi32, _pd, _i64, _pi64, _pd,
                                 C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "rbl_bench_kmeans_iter": (C.c_int, [_p, C.c_int, _pd, _i64, C.c_int, _pd]),
    "rbl_gen_matrix_hashwindow": (C.c_int, [_p, _i64, _i64, C.c_double, _u64, C.c_int, _pd]),
    "rbl_gen_matrix_circuit": (C.c_int, [_p, _i64, _i64, C.c_double, _u64, C.c_int, _pd]),
    "rbl_gen_matrix_rmat": (C.c_int, [_p, _i64, C.c_int, _i64, C.c_double, C.c_double, C.c_double,
                                      _u64, C.c_int, _pd]),
    "rbl_matrix_info": (C.c_int, [_p, _pi64, _pi64, _pi64, _pi64]),
    "rbl_get_matrix_csr": (C.c_int, [_p, _pi64, _pi32, _pd]),
    "rbl_row_ids": (C.c_int, [_p, _pi64]),
    "rbl_apply": (C.c_int, [_p, C.c_int, _pd, _pd]),
    "rbl_spmm_kernel_for": (C.c_int, [_p, C.c_int]),
    "rbl_matrix_format": (C.c_int, [_p]),
    "rbl_start": (C.c_int, [_p, C.c_int, C.c_int, C.c_int, _pd, _u64]),
    "rbl_step": (C.c_int, [_p, C.c_int, C.c_int, _pd, _pd]),
    "rbl_step_async": (C.c_int, [_p, C.c_int, C.c_int]),
    "rbl_comm_selftest": (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    "rbl_fetch": (C.c_int, [_p, C.c_int, C.c_int, _pd, _pd, _pi32]),
    "rbl_ritz": (C.c_int, [_p, C.c_int, C.c_int, _pd, _pd]),
    "rbl_get_block": (C.c_int, [_p, C.c_int, _pd]),
    "rbl_num_blocks": (C.c_int, [_p]),
    "rbl_set_filter": (C.c_int, [_p, C.c_int, C.c_double, C.c_double, C.c_double]),
    "rbl_set_filter_series": (C.c_int, [_p, C.c_int, C.c_double, C.c_double, _pd]),
    "rbl_apply_filter": (C.c_int, [_p, C.c_int, _pd, _pd]),
    "rbl_bench_series_pass": (C.c_int, [_p, _i64, C.c_int, _pd, _pd]),
    "rbl_cheb_moments": (C.c_int, [_p, C.c_int, C.c_int, C.c_double, C.c_double, _pd, _u64, _pd]),
    "rbl_bench_moment_pass": (C.c_int, [_p, _i64, C.c_int, C.c_int, _pd]),
    "rbl_cheb_diag": (C.c_int, [_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _pd, _pd, _u64,
                                C.c_int, _pd, _pd]),
    "rbl_bench_diag_pass": (C.c_int, [_p, _i64, C.c_int, C.c_int, C.c_int, _pd]),
    "rbl_set_lowrank": (C.c_int, [_p, C.c_int, _pd, _pd]),
    "rbl_get_lowrank": (C.c_int, [_p, C.POINTER(C.c_int), _pd, _pd]),
    "rbl_bench_lowrank_pass": (C.c_int, [_p, _i64, C.c_int, C.c_int, C.c_int, _pd, _pd]),
    "rbl_set_precond_lowrank": (C.c_int, [_p, C.c_int, _pd, _pd]),
    "rbl_clear_precond": (C.c_int, [_p]),
    "rbl_solve": (C.c_int, [_p, C.c_int, _pd, _pd, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                            _pi32, _pi32, _pd, _pd]),
    "rbl_bench_cg_pass": (C.c_int, [_p, _i64, C.c_int, C.c_int, C.c_int, _pd]),
    "rbl_ritz_project": (C.c_int, [_p, C.c_int, C.c_int, _pd, _pd]),
    "rbl_ritz_finish": (C.c_int, [_p, C.c_int, _pd, _pd, _pd, _pd]),
    "rbl_ritz_finish_cols": (C.c_int, [_p, C.c_int, C.c_int, _pd, _pd, _pd, _pd]),
    "rbl_restart": (C.c_int, [_p, C.c_int, _pd]),
    "rbl_lock": (C.c_int, [_p, C.c_int, C.c_int, _pd]),
    "rbl_num_locked": (C.c_int, [_p]),
    "rbl_get_locked": (C.c_int, [_p, _pd]),
    "rbl_reorth_last": (C.c_int, [_p, C.c_int, C.c_int]),
    "rbl_thick_restart": (C.c_int, [_p, C.c_int, C.c_int, _pd, _pd]),
    "rbl_bench_compress_pass": (C.c_int, [_p, _i64, C.c_int, C.c_int, C.c_int, C.c_int, _pd, _pd]),
    "rbl_num_stages": (C.c_int, []),
    "rbl_stage_name": (C.c_char_p, [C.c_int]),
    "rbl_timers": (C.c_int, [_p, _pd, C.c_int]),
    "rbl_reset_timers": (C.c_int, [_p]),
    "rbl_comm_stats": (C.c_int, [_p, _pi64, C.c_int, C.c_int]),
    "rbl_path_stats": (C.c_int, [_p, _pi64, C.c_int, C.c_int]),
    "rbl_upd32_gate_values": (C.c_int, [_p, _pd, C.c_int]),
    "rbl_shadow_valid": (C.c_int, [_p]),
    "rbl_get_shadow_block": (C.c_int, [_p, C.c_int, C.POINTER(C.c_float)]),
    "rbl_allgather_host":(C.c_int, [_p, _pi64, _pi64, C.c_int]),
    "rbl_synchronize": (C.c_int, [_p]),
    "rbl_plan_row_partition": (C.c_int, [_i64, _pi64, C.c_int, _pi64]),
    "rbl_plan_halo": (C.c_int, [_i64, _pi64, _pi64, C.c_int, C.c_int, _pi64, _pi64, _pi64]),
    "rbl_hashwindow_rows_host": (C.c_int, [_i64, _i64, C.c_double, _u64, C.c_int, _pd, _i64,
                                           _i64, _pi64, _pi64, _pd]),
    "rbl_plan_shadow_fits": (C.c_int, [_u64, _u64, _u64]),
}


class RBLError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"librbl_hip error {code}: {msg}")
        self.code = code


def load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"librbl_hip.so not built at {LIB_PATH}; run __graft_entry__.build() "
                          "(the HIP library is the only compute path — no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = load()
# compiled with -DRBL_VARIANTS (tools/build_variant.sh): the measured-and-rejected variants and
# their A/B switches are in this copy (tests/test_gpu_variants.py runs only then)
VARIANTS = bool(lib.rbl_build_flags() & RBL_BUILD_VARIANTS)


def dptr(a: np.ndarray | None):
    if a is None:
        return None
    assert a.dtype == np.float64 and (a.flags.c_contiguous or a.flags.f_contiguous)
    return a.ctypes.data_as(_pd)


def i64ptr(a: np.ndarray | None):
    if a is None:
        return None
    assert a.dtype == np.int64 and a.flags.c_contiguous
    return a.ctypes.data_as(_pi64)


def i32ptr(a: np.ndarray | None):
    if a is None:
        return None
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(_pi32)


def u8ptr(a: np.ndarray):
    assert a.dtype == np.uint8 and a.flags.c_contiguous
    return a.ctypes.data_as(_pu8)


def stage_names() -> list[str]:
    return [lib.rbl_stage_name(s).decode() for s in range(lib.rbl_num_stages())]


def plan_row_partition(rowptr: np.ndarray, nranks: int) -> np.ndarray:
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    out = np.zeros(nranks + 1, dtype=np.int64)
    st = lib.rbl_plan_row_partition(len(rowptr) - 1, i64ptr(rowptr), nranks, i64ptr(out))
    if st != RBL_OK:
        raise RBLError(st, "rbl_plan_row_partition")
    return out


def plan_shadow_fits(free_bytes: int, total_bytes: int, needed_bytes: int) -> bool:
    """The fit rule of RBL_OPT_UPD32_SHADOW (rbl_plan_shadow_fits; no GPU needed)."""
    return bool(lib.rbl_plan_shadow_fits(int(free_bytes), int(total_bytes), int(needed_bytes)))


def plan_halo(rowptr, colind, bounds, index_base=0):
    rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
    colind = np.ascontiguousarray(colind, dtype=np.int64)
    bounds = np.ascontiguousarray(bounds, dtype=np.int64)
    P = len(bounds) - 1
    lo = np.zeros(P, dtype=np.int64)
    hi = np.zeros(P, dtype=np.int64)
    st = lib.rbl_plan_halo(len(rowptr) - 1, i64ptr(rowptr), i64ptr(colind), index_base, P,
                           i64ptr(bounds), i64ptr(lo), i64ptr(hi))
    if st != RBL_OK:
        raise RBLError(st, "rbl_plan_halo")
    return lo, hi


def hashwindow_rows_host(n, halfwidth, density, seed, plant, row_begin, row_end):
    """Host twin of the device generator (same bits): returns (rowptr, colind, val) 0-based."""
    plant = np.ascontiguousarray(plant if plant is not None else np.zeros(0), dtype=np.float64)
    m = row_end - row_begin
    rowptr = np.zeros(m + 1, dtype=np.int64)
    pp = dptr(plant) if plant.size else None
    st = lib.rbl_hashwindow_rows_host(n, halfwidth, density, seed, plant.size, pp, row_begin,
                                      row_end, i64ptr(rowptr), None, None)
    if st != RBL_OK:
        raise RBLError(st, "rbl_hashwindow_rows_host")
    nnz = int(rowptr[-1])
    col = np.zeros(nnz, dtype=np.int64)
    val = np.zeros(nnz, dtype=np.float64)
    st = lib.rbl_hashwindow_rows_host(n, halfwidth, density, seed, plant.size, pp, row_begin,
                                      row_end, i64ptr(rowptr), i64ptr(col), dptr(val))
    if st != RBL_OK:
        raise RBLError(st, "rbl_hashwindow_rows_host")
    return rowptr, col, val
