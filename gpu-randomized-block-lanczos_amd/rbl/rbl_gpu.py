"""Host driver mirroring the reference's ``RBL_gpu(A, k, b)`` (Julia/RBL_gpu.jl:205-221).

The host keeps the loop control, the block-tridiagonal T_j and its LAPACK ``dsbev``
(Julia/common.jl), exactly as the north star asks; every n-sized operation — SpMM, local and
partial reorthogonalisation, tall-skinny QR, Ritz projection — runs in librbl_hip.so on the
MI355X.  Per step only the two b x b blocks A_i, B_{i+1} cross PCIe.

Semantics follow the GPU reference loop (RBL_gpu.jl:134-203):
  * max Krylov size 1200 (RBL_gpu.jl:211), step i runs while i*b < kryl_sz (:162);
  * partial reorth at even i (:164), local reorth every step (:167);
  * eigensolve + convergence test when i*b > k and i % 4 == 0 (:186-191), absolute 1e-7;
  * D returned in descending |lambda| (:202), V = [Q_1..Q_m] S in fp64 (RBL.jl:61-71, P3);
    each column of S (so each Ritz vector) signed so its largest coefficient is positive —
    LAPACK's eigenvector signs are arbitrary and differ between dsbev, dsbevd and the top-k
    path, so this makes V independent of the host eigensolver (parity is up to sign anyway).
Non-convergence (the reference's BoundsError) returns the last Ritz pairs
with ``info.converged = False`` and status RBL_WARN_NOT_CONVERGED.
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import RBLError, dptr, i32ptr, i64ptr, lib, u8ptr
from .host import (TBand, dsbev, eig_topk, fix_signs,
                   residual_norms, sort_eig_abs, speculation_depth)

KRYL_SZ_GPU = 1200          # RBL_gpu.jl:211
RESIDUAL_TOL = 1e-7         # RBL_gpu.jl:189


class LocalGroup:
    """In-process rank group (rbl_local_group_create): the multi-rank code path with a
    host-staged transport instead of RCCL, so it runs with several ranks on one GPU."""

    def __init__(self, nranks: int):
        import ctypes as C
        self._h = C.c_void_p()
        st = lib.rbl_local_group_create(C.byref(self._h), nranks)
        if st < 0:
            raise RBLError(st, "rbl_local_group_create")
        self.nranks = nranks

    def close(self) -> None:
        if self._h:
            lib.rbl_local_group_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One librbl_hip context: one GPU, or one rank of a row-partitioned job."""

    def __init__(self, device: int = 0, nranks: int = 1, rank: int = 0,
                 unique_id: bytes | None = None, group: "LocalGroup | None" = None,
                 shm_path: str | None = None):
        """nranks == 1: a single-GPU context.  nranks > 1 with `unique_id`: one rank of an RCCL
        job (one process per GPU).  `group`: one rank of an in-process LocalGroup (each rank
        driven by its own thread; ranks may share a GPU).  `shm_path`: one rank of a
        process-per-rank job over the shared-memory transport (rbl_create_shm; ranks may share
        a GPU; every rank passes the same path, unique per job)."""
        import ctypes as C
        self._h = C.c_void_p()
        if group is not None:
            nranks = group.nranks
            st = lib.rbl_create_local(C.byref(self._h), device, group._h, rank)
        elif shm_path is not None:
            st = lib.rbl_create_shm(C.byref(self._h), device, nranks, rank, shm_path.encode())
        elif nranks == 1:
            st = lib.rbl_create(C.byref(self._h), device)
        else:
            uid = np.frombuffer(unique_id, dtype=np.uint8).copy()
            st = lib.rbl_create_dist(C.byref(self._h), device, nranks, rank, u8ptr(uid))
        self.nranks, self.rank, self.device = nranks, rank, device
        self._check(st, "rbl_create")
        self.b = None

    # -- plumbing -------------------------------------------------------------------------
    def _check(self, st: int, what: str) -> int:
        if st < 0:
            msg = lib.rbl_last_error(self._h).decode() if self._h else ""
            raise RBLError(st, f"{what}: {msg}")
        return st

    def close(self) -> None:
        if self._h:
            lib.rbl_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, opt: int, value: int) -> None:
        self._check(lib.rbl_set_option(self._h, opt, int(value)), "rbl_set_option")

    # -- matrix ---------------------------------------------------------------------------
    def set_matrix(self, A) -> None:
        """Upload A: a SciPy sparse matrix (any format) or a dense NumPy array
        (RBL_gpu(A::Matrix{Float64}): panel GEMM on fp64 MFMA; with several ranks each keeps
        the rows of the even split).  The sparse arrays passed are A's rows (CSR): for the
        symmetric A of RBL_gpu.jl:209 they are exactly Julia's SparseMatrixCSC arrays; for any
        other A the device then computes A Q, as cuSPARSE does on the CSC matrix (benchmark.jl:58
        runs an unsymmetric sprandn) and as julia/RBL_hip.jl does by transposing first.
        A ``rbl.kernelop.KernelMatrix`` uploads its points, scale and nugget (set_matrix_kernel)."""
        from .kernelop import KernelMatrix
        if isinstance(A, KernelMatrix):
            self.set_matrix_kernel(A.X, A.kind, A.gamma, A.coef0, A.degree)
            if A.scale is not None or A.nugget != 0.0:
                self.set_kernel_scale(A.scale, A.nugget)
            return
        if isinstance(A, np.ndarray):
            n = A.shape[0]
            if A.ndim != 2 or A.shape[1] != n:
                raise ValueError("dense A must be square")
            P, r = self.nranks, self.rank
            r0, r1 = (n * r) // P, (n * (r + 1)) // P
            self.set_matrix_dense_rows(n, r0, r1, A[r0:r1])
            return
        A = sp.csr_matrix(A)
        A.sort_indices()
        n = A.shape[1]
        rowptr = A.indptr.astype(np.int64)
        colind = A.indices.astype(np.int64)
        nzval = A.data.astype(np.float64)
        self._check(lib.rbl_set_matrix_csc(self._h, n, A.nnz, i64ptr(rowptr), i64ptr(colind),
                                           dptr(nzval), 0), "rbl_set_matrix_csc")

    def set_matrix_dense_rows(self, n, row_begin, row_end, A_rows) -> None:
        """Rows [row_begin,row_end) of a dense symmetric n x n matrix (rbl_set_matrix_dense)."""
        M = np.asfortranarray(A_rows, dtype=np.float64)
        if M.shape != (row_end - row_begin, n):
            raise ValueError("A_rows must be (row_end - row_begin) x n")
        self._check(lib.rbl_set_matrix_dense(self._h, n, row_begin, row_end, dptr(M),
                                             max(M.shape[0], 1)), "rbl_set_matrix_dense")

    def set_matrix_rows(self, n, row_begin, row_end, rowptr, colind, val, index_base=0) -> None:
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        colind = np.ascontiguousarray(colind, dtype=np.int64)
        val = np.ascontiguousarray(val, dtype=np.float64)
        self._check(lib.rbl_set_matrix_csr_rows(self._h, n, row_begin, row_end, i64ptr(rowptr),
                                                i64ptr(colind), dptr(val), index_base),
                    "rbl_set_matrix_csr_rows")

    # -- rectangular sparse B: the implicit normal operator B^T B ----------------------------
    def set_matrix_normal(self, B) -> None:
        """Upload a rectangular sparse B (m x n, any SciPy sparse format) for its singular
        triplets (rbl_set_matrix_normal): the Krylov operator is B^T B, applied as B^T (B Q) and
        never formed.  CSR arrays go over as they stand with layout 0, CSC arrays with layout 1
        (other formats are converted to CSR); the other orientation is built on the device.
        One rank, fp64 basis."""
        if not sp.issparse(B) or B.ndim != 2:
            raise ValueError("set_matrix_normal: B must be a 2-D SciPy sparse matrix")
        if B.format not in ("csr", "csc"):
            B = B.tocsr()
        if not B.has_canonical_format:      # sorted, no duplicates (a copy: B is the caller's)
            B = B.copy()
            B.sum_duplicates()
        m, n = B.shape
        ptr = np.ascontiguousarray(B.indptr, dtype=np.int64)
        ind = np.ascontiguousarray(B.indices, dtype=np.int64)
        val = np.ascontiguousarray(B.data, dtype=np.float64)
        self._check(lib.rbl_set_matrix_normal(self._h, m, n, B.nnz, i64ptr(ptr), i64ptr(ind),
                                              dptr(val), 0, 0 if B.format == "csr" else 1),
                    "rbl_set_matrix_normal")

    def rect_info(self):
        """(m, n, nnz) of the rectangular B held (rbl_rect_info)."""
        v = [np.zeros(1, np.int64) for _ in range(3)]
        self._check(lib.rbl_rect_info(self._h, *[i64ptr(x) for x in v]), "rbl_rect_info")
        return tuple(int(x[0]) for x in v)

    def get_matrix_rect(self, trans: bool = False):
        """One device orientation as (rowptr, ind, val), 0-based: B's CSR, or with trans B^T's."""
        m, n, nnz = self.rect_info()
        rows = n if trans else m
        rowptr = np.zeros(rows + 1, np.int64)
        ind = np.zeros(max(nnz, 1), np.int32)
        val = np.zeros(max(nnz, 1), np.float64)
        self._check(lib.rbl_get_matrix_rect(self._h, int(bool(trans)), i64ptr(rowptr), i32ptr(ind),
                                            dptr(val)), "rbl_get_matrix_rect")
        return rowptr, ind[:nnz], val[:nnz]

    def apply_rect(self, X: np.ndarray, trans: bool = False) -> np.ndarray:
        """Y = B X (X: n x b), or with trans Y = B^T X (X: m x b): one pass of the gather pair."""
        m, n, _ = self.rect_info()
        rin, rout = (m, n) if trans else (n, m)
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] != rin:
            raise ValueError(f"apply_rect: X must have {rin} rows")
        Y = np.zeros((rout, X.shape[1]), order="F")
        self._check(lib.rbl_apply_rect(self._h, int(bool(trans)), X.shape[1], dptr(X), dptr(Y)),
                    "rbl_apply_rect")
        return Y

    def set_rect_shift(self, u, v) -> None:
        """Rank-one shift C = B - u v^T of the rectangular B held (rbl_set_rect_shift): u of
        length m, v of length n, both copied to the device; ``None, None`` clears it.  While set,
        apply / start / step / ritz_project run on C^T C and left_vectors returns C V / sigma."""
        if u is None and v is None:
            self._check(lib.rbl_set_rect_shift(self._h, None, None), "rbl_set_rect_shift")
            return
        m, n, _ = self.rect_info()
        u = None if u is None else np.ascontiguousarray(u, dtype=np.float64).ravel()
        v = None if v is None else np.ascontiguousarray(v, dtype=np.float64).ravel()
        if (u is not None and u.size != m) or (v is not None and v.size != n):
            raise ValueError(f"set_rect_shift: u must have {m} entries and v {n}")
        self._check(lib.rbl_set_rect_shift(self._h, dptr(u), dptr(v)), "rbl_set_rect_shift")

    def get_rect_shift(self):
        """(u, v) of the shift set (rbl_get_rect_shift); RBLError (RBL_ERR_STATE) when none is."""
        m, n, _ = self.rect_info()
        u, v = np.zeros(m), np.zeros(n)
        self._check(lib.rbl_get_rect_shift(self._h, dptr(u), dptr(v)), "rbl_get_rect_shift")
        return u, v

    def apply_rect_shifted(self, X: np.ndarray, trans: bool = False) -> np.ndarray:
        """Y = C X (X: n x b), or with trans Y = C^T X (X: m x b), C = B - u v^T: one pass of the
        shifted pair.  Without a shift the bits of apply_rect."""
        m, n, _ = self.rect_info()
        rin, rout = (m, n) if trans else (n, m)
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] != rin:
            raise ValueError(f"apply_rect_shifted: X must have {rin} rows")
        Y = np.zeros((rout, X.shape[1]), order="F")
        self._check(lib.rbl_apply_rect_shifted(self._h, int(bool(trans)), X.shape[1], dptr(X),
                                               dptr(Y)), "rbl_apply_rect_shifted")
        return Y

    # -- implicit kernel matrix: K_ij = kappa(x_i, x_j) from the points alone -----------------
    def set_matrix_kernel(self, X, kind="rbf", gamma: float = 1.0, coef0: float = 0.0,
                          degree: int = 3) -> None:
        """The kernel matrix over the rows of X (n x d) as the operator (rbl_set_matrix_kernel):
        kind "rbf" exp(-gamma |x-y|^2), "laplace" exp(-gamma |x-y|), "poly" (gamma x^T y +
        coef0)^degree, or the RBL_KERNEL_* id.  K is never formed.  One rank, fp64 basis."""
        from .kernelop import KINDS
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[0] < 1:
            raise ValueError("set_matrix_kernel: X must be an n x d array with n >= 1")
        if isinstance(kind, str):
            if kind not in KINDS:
                raise ValueError("set_matrix_kernel: kind must be 'rbf', 'laplace' or 'poly'")
            kind = KINDS[kind]
        X = np.asfortranarray(X)
        n, d = X.shape
        self._check(lib.rbl_set_matrix_kernel(self._h, n, d, dptr(X), n, int(kind), float(gamma),
                                              float(coef0), int(degree)), "rbl_set_matrix_kernel")

    def set_kernel_scale(self, scale=None, nugget: float = 0.0) -> None:
        """The operator becomes diag(scale) K diag(scale) + nugget I for the kernel matrix held
        (rbl_set_kernel_scale); ``None, 0.0`` clears both."""
        if scale is not None:
            scale = np.ascontiguousarray(scale, dtype=np.float64).ravel()
            if scale.size != self.kernel_info()["n"]:
                raise ValueError(f"set_kernel_scale: scale must have n = {self.kernel_info()['n']} entries")
        self._check(lib.rbl_set_kernel_scale(self._h, dptr(scale), float(nugget)), "rbl_set_kernel_scale")

    def kernel_info(self) -> dict:
        """n, d, kind (RBL_KERNEL_*), gamma, coef0, degree, has_scale and nugget of the kernel
        matrix held (rbl_kernel_info); RBLError (RBL_ERR_STATE) when the matrix is of another kind."""
        import ctypes as C
        n = C.c_int64(0)
        d, kind, degree, has = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        g, c0, nug = np.zeros(1), np.zeros(1), np.zeros(1)
        self._check(lib.rbl_kernel_info(self._h, C.byref(n), C.byref(d), C.byref(kind), dptr(g), dptr(c0),
                                        C.byref(degree), C.byref(has), dptr(nug)), "rbl_kernel_info")
        return {"n": n.value, "d": d.value, "kind": kind.value, "gamma": float(g[0]),
                "coef0": float(c0[0]), "degree": degree.value, "has_scale": bool(has.value),
                "nugget": float(nug[0])}

    def bench_kernel_pass(self, b: int, reps: int = 5) -> float:
        """Milliseconds per application of the kernel matrix held to a device-resident block of b
        columns (rbl_bench_kernel_pass)."""
        ms = np.zeros(1)
        self._check(lib.rbl_bench_kernel_pass(self._h, int(b), int(reps), dptr(ms)), "rbl_bench_kernel_pass")
        return float(ms[0])

    def _cross_points(self, what, Z):
        from .kernelop import _new_points
        info = self.kernel_info()
        return np.asfortranarray(_new_points(what, Z, info["d"])), info["n"]

    def kernel_cross(self, Z, W, trans: bool = False) -> np.ndarray:
        """The cross-kernel product of the kernel matrix held (points X, scale s) with the m new
        points Z (m x d) (rbl_kernel_cross): Y (m x b) = kappa(Z, X) diag(s) W for W n x b, or with
        trans Y (n x b) = diag(s) kappa(X, Z) W for W m x b.  kappa(Z, X) is never formed; the
        nugget does not enter and no pair is treated as "the same point".  Two calls give the same
        bits."""
        Z, n = self._cross_points("kernel_cross", Z)
        m = Z.shape[0]
        rin, rout = (m, n) if trans else (n, m)
        W = np.asarray(W, dtype=np.float64)
        if W.ndim == 1:
            W = W.reshape(-1, 1)
        if W.ndim != 2 or W.shape[0] != rin or W.shape[1] < 1:
            raise ValueError(f"kernel_cross: W must have {rin} rows and at least one column")
        if not np.all(np.isfinite(W)):
            raise ValueError("kernel_cross: W has a non-finite entry")
        W = np.asfortranarray(W)
        Y = np.zeros((rout, W.shape[1]), order="F")
        self._check(lib.rbl_kernel_cross(self._h, m, dptr(Z), m, int(bool(trans)), W.shape[1], dptr(W), rin,
                                         dptr(Y), rout), "rbl_kernel_cross")
        return Y

    def bench_kernel_cross(self, Z, b: int, trans: bool = False, splits: int = 0, reps: int = 5) -> float:
        """Milliseconds per cross-kernel product of the matrix held with the points Z and a
        device-resident block of b columns (rbl_bench_kernel_cross); splits = 0: the library's rule."""
        Z, _ = self._cross_points("bench_kernel_cross", Z)
        ms = np.zeros(1)
        self._check(lib.rbl_bench_kernel_cross(self._h, Z.shape[0], dptr(Z), Z.shape[0], int(bool(trans)),
                                               int(b), int(splits), int(reps), dptr(ms)),
                    "rbl_bench_kernel_cross")
        return float(ms[0])

    def _knn_args(self, what, k, Z):
        """(Z as an F-ordered m x d block or None, m, ldz, rows) for the two neighbour entries."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"{what}: k must be an integer")
        if Z is None:
            return None, 0, 0, self.kernel_info()["n"]
        Z, _ = self._cross_points(what, Z)
        return Z, Z.shape[0], Z.shape[0], Z.shape[0]

    def kernel_knn(self, k: int, Z=None, splits: int = 0):
        """The k nearest neighbours among the points X of the kernel matrix held (rbl_kernel_knn):
        of the n points themselves (Z None; the pair (i, i) is skipped by index, k <= n - 1) or of the
        m new points Z (m x d; no pair skipped, k <= n).  Returns (idx, d2), int32 and float64 arrays
        rows x k: column c holds the (c + 1)-th nearest point's index in X and its squared Euclidean
        distance in the operator's Gram form; each row ascending in (d2, index), the smaller index
        first on equal distances.  The kernel kind, gamma, scale and nugget do not enter.  splits = 0:
        the library's rule; the result does not depend on it.  Two calls give the same bits."""
        Z, m, ldz, rows = self._knn_args("kernel_knn", k, Z)
        idx = np.zeros((rows, max(int(k), 0)), dtype=np.int32, order="F")
        d2 = np.zeros((rows, max(int(k), 0)), order="F")
        self._check(lib.rbl_kernel_knn(self._h, m, dptr(Z), ldz, int(k), int(splits),
                                       idx.ctypes.data_as(_lib._pi32), rows, dptr(d2), rows), "rbl_kernel_knn")
        return idx, d2

    def bench_kernel_knn(self, k: int, Z=None, splits: int = 0, reps: int = 5) -> float:
        """Milliseconds per neighbour search of ``kernel_knn`` on the device (rbl_bench_kernel_knn)."""
        Z, m, ldz, _ = self._knn_args("bench_kernel_knn", k, Z)
        ms = np.zeros(1)
        self._check(lib.rbl_bench_kernel_knn(self._h, m, dptr(Z), ldz, int(k), int(splits), int(reps), dptr(ms)),
                    "rbl_bench_kernel_knn")
        return float(ms[0])

    @staticmethod
    def _pchol_rank(what, max_rank):
        if isinstance(max_rank, bool) or not isinstance(max_rank, (int, np.integer)):
            raise ValueError(f"{what}: max_rank must be an integer")
        return int(max_rank)

    def kernel_pchol(self, max_rank: int, tol: float = 0.0):
        """Partial pivoted Cholesky of the kernel matrix held, without its nugget (rbl_kernel_pchol):
        L L^T ~ diag(s) K diag(s) by at most max_rank (<= min(n, 256)) greedy steps, each one column of
        K; stops early when the largest residual diagonal entry is at rounding level or the residual
        trace is <= tol (in [0, 1)) times the first.  Returns (L, piv, trace): L n x rank (F-ordered),
        piv the rank pivots (int32), trace the rank + 1 residual traces.  Two calls give the same
        bits."""
        import ctypes as C
        R = self._pchol_rank("kernel_pchol", max_rank)
        n = self.matrix_info()[0]
        L = np.zeros((n, max(R, 0)), order="F")
        piv = np.full(max(R, 0), -1, dtype=np.int32)
        trace = np.zeros(max(R, 0) + 1)
        rank = C.c_int(0)
        self._check(lib.rbl_kernel_pchol(self._h, R, float(tol), dptr(L), n, piv.ctypes.data_as(_lib._pi32),
                                         dptr(trace), C.byref(rank)), "rbl_kernel_pchol")
        r = int(rank.value)
        return np.asfortranarray(L[:, :r]), piv[:r].copy(), trace[:r + 1].copy()

    def bench_kernel_pchol(self, max_rank: int, reps: int = 5) -> float:
        """Milliseconds per factorisation of ``kernel_pchol`` at tol = 0 on the device
        (rbl_bench_kernel_pchol)."""
        ms = np.zeros(1)
        self._check(lib.rbl_bench_kernel_pchol(self._h, self._pchol_rank("bench_kernel_pchol", max_rank), int(reps),
                                               dptr(ms)), "rbl_bench_kernel_pchol")
        return float(ms[0])

    def kernel_hadamard(self, A, B, Q, weight="value") -> np.ndarray:
        """U (n x b) = (Phi o A B^T) Q over the points of the kernel matrix held
        (rbl_kernel_hadamard): A and B n x r, Q n x b, Phi_ij = kappa (weight "value"), d kappa /
        d gamma ("dgamma") or the factor psi of d kappa / d log s_k ("dscale": times (x_ik - x_jk)^2
        for the radial kernels, x_ik x_jk for poly), or the RBL_KWEIGHT_* id.  The operator's scale
        and nugget do not enter.  4 ceil(d / 4) + 4 ceil(r / 4) <= 256.  Two calls give the same bits."""
        from .kernelop import WEIGHTS
        if isinstance(weight, str):
            if weight not in WEIGHTS:
                raise ValueError("kernel_hadamard: weight must be 'value', 'dgamma' or 'dscale'")
            weight = WEIGHTS[weight]
        n = self.kernel_info()["n"]
        blocks = []
        for name, M in (("A", A), ("B", B), ("Q", Q)):
            M = np.asarray(M, dtype=np.float64)
            if M.ndim == 1:
                M = M.reshape(-1, 1)
            if M.ndim != 2 or M.shape[0] != n or M.shape[1] < 1:
                raise ValueError(f"kernel_hadamard: {name} must have n = {n} rows and at least one column")
            if not np.all(np.isfinite(M)):
                raise ValueError(f"kernel_hadamard: {name} has a non-finite entry")
            blocks.append(np.asfortranarray(M))
        A, B, Q = blocks
        if A.shape[1] != B.shape[1]:
            raise ValueError("kernel_hadamard: A and B must have the same number of columns")
        U = np.zeros((n, Q.shape[1]), order="F")
        self._check(lib.rbl_kernel_hadamard(self._h, int(weight), A.shape[1], dptr(A), n, dptr(B), n, Q.shape[1],
                                            dptr(Q), n, dptr(U), n), "rbl_kernel_hadamard")
        return U

    def bench_kernel_hadamard(self, r: int, b: int, weight="value", reps: int = 5) -> float:
        """Milliseconds per derivative product of the matrix held with device-resident factors of r
        columns and a block of b columns (rbl_bench_kernel_hadamard)."""
        from .kernelop import WEIGHTS
        ms = np.zeros(1)
        mode = WEIGHTS[weight] if isinstance(weight, str) else int(weight)
        self._check(lib.rbl_bench_kernel_hadamard(self._h, mode, int(r), int(b), int(reps), dptr(ms)),
                    "rbl_bench_kernel_hadamard")
        return float(ms[0])

    # -- k-means on the device: the points are the context's own, beside whatever matrix it holds --
    def kmeans_set_points(self, X) -> None:
        """The n x d points of the k-means entries (rbl_kmeans_set_points): copied to the device once;
        the matrix, the basis and the options of the context are left as they were."""
        from .kmeans import _points
        X = np.asfortranarray(_points("kmeans_set_points", X))
        n, d = X.shape
        self._check(lib.rbl_kmeans_set_points(self._h, n, d, dptr(X), n), "rbl_kmeans_set_points")
        self._km_shape = (n, d)

    def kmeans_clear(self) -> None:
        """Release the k-means points (rbl_kmeans_clear)."""
        self._check(lib.rbl_kmeans_clear(self._h), "rbl_kmeans_clear")
        self._km_shape = None

    def _kmeans_shape(self, what):
        shape = getattr(self, "_km_shape", None)
        if shape is None:
            raise ValueError(f"{what}: no points set (kmeans_set_points)")
        return shape

    def kmeans_seed(self, n_clusters: int, uniforms) -> np.ndarray:
        """Plain k-means++ over the points set (rbl_kmeans_seed) from n_clusters uniforms in [0, 1):
        the int32 indices of the picked points.  Round 0 picks min(floor(u_0 n), n - 1); round r the
        smallest i whose inclusive prefix sum of w_i = min over the picked points of d2(i, .) exceeds
        u_r total.  Two calls give the same bits."""
        from .kmeans import _check_clusters
        n, _ = self._kmeans_shape("kmeans_seed")
        c = _check_clusters("kmeans_seed", n_clusters, n)
        u = np.ascontiguousarray(uniforms, dtype=np.float64).ravel()
        if u.size != c:
            raise ValueError(f"kmeans_seed: needs n_clusters = {c} uniforms, got {u.size}")
        if not np.all(np.isfinite(u)) or np.any(u < 0.0) or np.any(u >= 1.0):
            raise ValueError("kmeans_seed: every uniform must be finite and in [0, 1)")
        picked = np.zeros(c, dtype=np.int32)
        self._check(lib.rbl_kmeans_seed(self._h, c, dptr(u), i32ptr(picked)), "rbl_kmeans_seed")
        return picked

    def _kmeans_centres(self, what, C0):
        from .kmeans import _check_clusters
        n, d = self._kmeans_shape(what)
        C0 = np.asarray(C0, dtype=np.float64)
        if C0.ndim == 1 and d == 1:
            C0 = C0.reshape(-1, 1)
        if C0.ndim != 2 or C0.shape[1] != d:
            raise ValueError(f"{what}: the centres must be a c x d array with d = {d}")
        c = _check_clusters(what, C0.shape[0], n)
        if not np.all(np.isfinite(C0)):
            raise ValueError(f"{what}: a centre has a non-finite entry")
        return np.asfortranarray(C0), c, n, d

    def kmeans_run(self, C0, max_iter: int = 300, tol: float = 0.0):
        """Lloyd's iteration over the points set from the centres C0 (c x d) (rbl_kmeans_run): a
        ``rbl.kmeans.KMeansResult`` with the consistent triple (labels_t, C_t, inertia_t), counts_t,
        n_iter = t and converged (1: no label changed, 2: |C_t - C_{t-1}|_F^2 <= tol, 0: max_iter
        reached).  max_iter = 0 assigns only.  A point goes to the centre with the smallest
        (d2, index); a centre without points keeps its value.  Two calls give the same bits."""
        import ctypes as C
        from .kmeans import KMeansResult
        C0, c, n, d = self._kmeans_centres("kmeans_run", C0)
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
            raise ValueError("kmeans_run: max_iter must be an integer >= 0")
        if not np.isfinite(tol) or tol < 0.0:
            raise ValueError("kmeans_run: tol must be finite and >= 0")
        labels = np.zeros(n, dtype=np.int32)
        centers = np.zeros((c, d), order="F")
        counts = np.zeros(c, dtype=np.int64)
        inertia = np.zeros(1)
        n_iter, conv = C.c_int(0), C.c_int(0)
        self._check(lib.rbl_kmeans_run(self._h, c, dptr(C0), c, int(max_iter), float(tol), i32ptr(labels),
                                       dptr(centers), c, i64ptr(counts), dptr(inertia), C.byref(n_iter),
                                       C.byref(conv)), "rbl_kmeans_run")
        return KMeansResult(labels, np.ascontiguousarray(centers), float(inertia[0]), counts, n_iter.value,
                            conv.value)

    def bench_kmeans_iter(self, C0, reps: int = 5) -> float:
        """Milliseconds per Lloyd iteration over the points set against the centres C0
        (rbl_bench_kmeans_iter)."""
        C0, c, _, _ = self._kmeans_centres("bench_kmeans_iter", C0)
        ms = np.zeros(1)
        self._check(lib.rbl_bench_kmeans_iter(self._h, c, dptr(C0), c, int(reps), dptr(ms)), "rbl_bench_kmeans_iter")
        return float(ms[0])

    # -- implicit symmetric low-rank update: the operator A + P S P^T ------------------------
    def set_lowrank(self, P, S) -> None:
        """The operator becomes A + P S P^T (rbl_set_lowrank): P n x r, S r x r symmetric,
        1 <= r <= 32, both copied to the device; a 1-D P with a scalar S is r = 1; ``None, None``
        clears the update.  While set, apply / start / step / the Chebyshev filters / cheb_moments / cheb_diag /
        ritz_project run on the updated operator.  Square A, one rank, fp64 basis."""
        if P is None and S is None:
            self._check(lib.rbl_set_lowrank(self._h, 0, None, None), "rbl_set_lowrank")
            return
        if P is None or S is None:
            raise ValueError("set_lowrank: P and S must both be given or both be None")
        n, r0, r1, _ = self.matrix_info()
        P = np.asarray(P, dtype=np.float64)
        S = np.asarray(S, dtype=np.float64)
        if P.ndim == 1:
            P = P.reshape(-1, 1)
        if S.ndim == 0:
            S = S.reshape(1, 1)
        if P.ndim != 2 or P.shape[0] != r1 - r0:
            raise ValueError(f"set_lowrank: P must have {r1 - r0} rows")
        r = P.shape[1]
        if S.shape != (r, r):
            raise ValueError(f"set_lowrank: S must be {r} x {r}")
        if r < 1:
            raise ValueError("set_lowrank: P has no columns (None, None clears the update)")
        P = np.asfortranarray(P)
        S = np.asfortranarray(S)
        self._check(lib.rbl_set_lowrank(self._h, r, dptr(P), dptr(S)), "rbl_set_lowrank")

    def get_lowrank(self):
        """(P, S) of the update set (rbl_get_lowrank), exactly as passed: P n x r, S r x r;
        RBLError (RBL_ERR_STATE) when none is."""
        import ctypes as C
        r = C.c_int(0)
        self._check(lib.rbl_get_lowrank(self._h, C.byref(r), None, None), "rbl_get_lowrank")
        n, r0, r1, _ = self.matrix_info()
        P = np.zeros((r1 - r0, r.value), order="F")
        S = np.zeros((r.value, r.value), order="F")
        self._check(lib.rbl_get_lowrank(self._h, C.byref(r), dptr(P), dptr(S)), "rbl_get_lowrank")
        return P, S

    def bench_lowrank_pass(self, rows: int, b: int, r: int, reps: int = 10):
        """(project_ms, update_ms) per pass of the two n-sized passes of the low-rank update on
        scratch blocks (rbl_bench_lowrank_pass)."""
        pm, um = np.zeros(1), np.zeros(1)
        self._check(lib.rbl_bench_lowrank_pass(self._h, int(rows), int(b), int(r), int(reps), dptr(pm),
                                               dptr(um)), "rbl_bench_lowrank_pass")
        return float(pm[0]), float(um[0])

    def set_preconditioner(self, V, dv=None) -> None:
        """The preconditioner of ``solve``, M^-1 = I + V diag(dv) V^T (rbl_set_precond_lowrank): V
        n x r with orthonormal columns, 1 <= r <= 32, dv its r entries (all > -1), both copied to the
        device in buffers of their own (a ``set_lowrank`` update may be set too).  ``None`` clears it
        (rbl_clear_precond); setting a matrix clears it as well."""
        if V is None:
            self._check(lib.rbl_clear_precond(self._h), "rbl_clear_precond")
            return
        n, r0, r1, _ = self.matrix_info()
        V = np.asarray(V, dtype=np.float64)
        dv = np.asarray(dv, dtype=np.float64) if dv is not None else None
        if V.ndim == 1:
            V = V.reshape(-1, 1)
        if V.ndim != 2 or V.shape[0] != r1 - r0:
            raise ValueError(f"set_preconditioner: V must have {r1 - r0} rows")
        r = V.shape[1]
        if dv is None or dv.reshape(-1).shape != (r,):
            raise ValueError(f"set_preconditioner: dv must have {r} entries")
        if r < 1:
            raise ValueError("set_preconditioner: V has no columns (None clears the preconditioner)")
        V = np.asfortranarray(V)
        dv = np.ascontiguousarray(dv.reshape(-1))
        self._check(lib.rbl_set_precond_lowrank(self._h, r, dptr(V), dptr(dv)), "rbl_set_precond_lowrank")

    def solve(self, B, shift: float = 0.0, tol: float = 1e-10, max_iter: int = 1000, x0=None,
              check_every: int = 10, coef: bool = False):
        """(X, iters, status, resid[, alpha, beta]) of (Op + shift I) X = B by batched preconditioned
        CG on the device (rbl_solve): B n x b with b <= RBL_MAX_BLOCK, every column its own recurrence
        and one shared product per iteration.  Per column: iters, status (0 converged to |r| <= tol
        |b|, 1 max_iter reached, 2 not positive definite) and resid, the true |b - (Op + shift) x| /
        |b| of the returned x.  x0: a starting guess of B's shape.  coef=True (max_iter <= 4096) also
        returns the CG coefficients alpha, beta as max_iter x b arrays, zero past a column's iters
        (``rbl.cg_tridiag``).  The preconditioner is the one of ``set_preconditioner``."""
        n, r0, r1, _ = self.matrix_info()
        B = np.asfortranarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != r1 - r0 or B.shape[1] < 1:
            raise ValueError(f"solve: B must be {r1 - r0} x b")
        b, max_iter = B.shape[1], int(max_iter)
        if x0 is None:
            X = np.zeros(B.shape, order="F")
        else:
            X = np.array(x0, dtype=np.float64, order="F")
            if X.shape != B.shape:
                raise ValueError("solve: x0 must have the shape of B")
        iters = np.zeros(b, dtype=np.int32)
        status = np.zeros(b, dtype=np.int32)
        resid = np.zeros(b)
        hist = np.zeros((2 * max(max_iter, 1), b), order="F") if coef else None
        self._check(lib.rbl_solve(self._h, b, dptr(B), dptr(X), float(shift), float(tol), max_iter,
                                  int(check_every), int(x0 is not None), i32ptr(iters), i32ptr(status),
                                  dptr(resid), dptr(hist)), "rbl_solve")
        if coef:
            return X, iters, status, resid, hist[0::2].copy(), hist[1::2].copy()
        return X, iters, status, resid

    def bench_cg_pass(self, rows: int, b: int, r: int = 0, reps: int = 20):
        """(dot_ms, update_ms, dir_ms) per pass of the three row passes of one CG iteration on scratch
        blocks of rows x b (rbl_bench_cg_pass); r > 0: with a rank-r preconditioner."""
        ms = np.zeros(3)
        self._check(lib.rbl_bench_cg_pass(self._h, int(rows), int(b), int(r), int(reps), dptr(ms)),
                    "rbl_bench_cg_pass")
        return tuple(float(v) for v in ms)

    def left_vectors(self, V: np.ndarray, sigma) -> np.ndarray:
        """U = B V diag(1 / sigma) (images.jl:24), m x k, from V (n x k) and the singular values
        (with a shift set: C V diag(1 / sigma))."""
        m, n, _ = self.rect_info()
        V = np.asfortranarray(V, dtype=np.float64)
        sigma = np.ascontiguousarray(sigma, dtype=np.float64).ravel()
        if V.ndim != 2 or V.shape[0] != n or sigma.size != V.shape[1]:
            raise ValueError("left_vectors: V must be n x k and sigma of length k")
        U = np.zeros((m, V.shape[1]), order="F")
        self._check(lib.rbl_left_vectors(self._h, V.shape[1], dptr(V), dptr(sigma), dptr(U)),
                    "rbl_left_vectors")
        return U

    def gen_hashwindow(self, n: int, halfwidth: int, density: float, seed: int,
                       plant=None) -> None:
        plant = np.ascontiguousarray(plant if plant is not None else np.zeros(0), np.float64)
        self._check(lib.rbl_gen_matrix_hashwindow(self._h, n, halfwidth, density, seed,
                                                  plant.size, dptr(plant) if plant.size else None),
                    "rbl_gen_matrix_hashwindow")

    def gen_rmat(self, n: int, scale: int, edges: int, seed: int, plant=None,
                 a: float = 0.57, b: float = 0.19, c: float = 0.19) -> None:
        """Seeded symmetric R-MAT matrix generated on the device."""
        plant = np.ascontiguousarray(plant if plant is not None else np.zeros(0), np.float64)
        self._check(lib.rbl_gen_matrix_rmat(self._h, n, scale, edges, a, b, c, seed, plant.size,
                                            dptr(plant) if plant.size else None),
                    "rbl_gen_matrix_rmat")

    def gen_circuit(self, n: int = 1_585_478, seed: int = 20261015, plant=None,
                    width: int = 1259, p_edge: float = 0.95873) -> None:
        """Seeded circuit-like SPD matrix of G3_circuit's shape (BASELINE config 3), generated
        on the device (rbl_gen_matrix_circuit); the defaults give n and nnz of G3_circuit."""
        plant = np.ascontiguousarray(plant if plant is not None else np.zeros(0), np.float64)
        self._check(lib.rbl_gen_matrix_circuit(self._h, n, width, p_edge, seed, plant.size,
                                               dptr(plant) if plant.size else None),
                    "rbl_gen_matrix_circuit")

    def matrix_info(self):
        v = [np.zeros(1, np.int64) for _ in range(4)]
        self._check(lib.rbl_matrix_info(self._h, *[i64ptr(x) for x in v]), "rbl_matrix_info")
        n, r0, r1, nnz = (int(x[0]) for x in v)
        return n, r0, r1, nnz

    def row_ids(self) -> np.ndarray:
        """Original (generator) id of each local row (rbl_row_ids): r0..r1-1, or the inverse
        relabel of a matrix generated with RBL_OPT_RELABEL — the order of omega's and V's rows."""
        n, r0, r1, _ = self.matrix_info()
        ids = np.zeros(max(r1 - r0, 1), np.int64)
        self._check(lib.rbl_row_ids(self._h, i64ptr(ids)), "rbl_row_ids")
        return ids[: r1 - r0]

    def get_matrix_csr(self):
        n, r0, r1, nnz = self.matrix_info()
        rowptr = np.zeros(r1 - r0 + 1, np.int64)
        col = np.zeros(max(nnz, 1), np.int32)
        val = np.zeros(max(nnz, 1), np.float64)
        self._check(lib.rbl_get_matrix_csr(self._h, i64ptr(rowptr), i32ptr(col), dptr(val)),
                    "rbl_get_matrix_csr")
        return rowptr, col[:nnz], val[:nnz]

    def apply(self, X: np.ndarray) -> np.ndarray:
        """Y = A X on the device (local rows), through the same SpMM kernels as a step."""
        n, r0, r1, _ = self.matrix_info()
        X = np.asfortranarray(X, dtype=np.float64)
        b = X.shape[1]
        Y = np.zeros((r1 - r0, b), order="F")
        self._check(lib.rbl_apply(self._h, b, dptr(X), dptr(Y)), "rbl_apply")
        return Y

    def matrix_format(self) -> int:
        """0 CSR only, 1 band tiles, 2 packed band tiles, 3 half band tiles, 4 dense,
        5 rectangular B (both orientations as CSR)."""
        return self._check(lib.rbl_matrix_format(self._h), "rbl_matrix_format")

    def spmm_kernel_for(self, b: int) -> int:
        """The SpMM kernel rbl_step runs at block size b: 1 global-gather CSR, 2 LDS-window CSR,
        3 LDS-densified band, 4 dense panels, 5 band tiles, 6 segmented gather, 7 column panels
        (the same ids RBL_OPT_SPMM_KERNEL takes), 8 the rectangular gather pair."""
        return self._check(lib.rbl_spmm_kernel_for(self._h, b), "rbl_spmm_kernel_for")

    # -- Krylov run -------------------------------------------------------------------------
    def start(self, b: int, max_blocks: int, omega=None, seed: int = 0, basis_bits: int = 64) -> None:
        """basis_bits 32: the mixed mode of RBL_gpu.jl with FLOAT = Float32 (fp32 Krylov blocks
        and reorth, fp64 A*Q / 3-term / QR / Ritz)."""
        om = None
        if omega is not None:
            om = np.asfortranarray(omega, dtype=np.float64)
        self._check(lib.rbl_start(self._h, b, max_blocks, basis_bits, dptr(om), seed), "rbl_start")
        self.b = b

    def step(self, i: int, part_reorth):
        """part_reorth: bool, or the flag word of rbl_step (bit 0 partial reorth, bit 1 the
        locked-vector reorth of the restarted variants)."""
        b = self.b
        A = np.zeros((b, b), order="F")
        B = np.zeros((b, b), order="F")
        st = self._check(lib.rbl_step(self._h, i, int(part_reorth), dptr(A), dptr(B)), "rbl_step")
        return A, B, st

    def step_async(self, i: int, part_reorth) -> None:
        """rbl_step_async: enqueue step i; A_i, B_{i+1} and its status come from fetch()."""
        self._check(lib.rbl_step_async(self._h, i, int(part_reorth)), "rbl_step_async")

    def fetch(self, i0: int, i1: int):
        """rbl_fetch: wait, then [(A_j, B_j, status_j) for j in i0..i1-1]."""
        b, m = self.b, i1 - i0
        A = np.zeros((m, b, b))
        B = np.zeros((m, b, b))
        st = np.zeros(m, np.int32)
        self._check(lib.rbl_fetch(self._h, i0, i1, dptr(A), dptr(B), i32ptr(st)), "rbl_fetch")
        # each b x b block arrives column-major
        return [(A[j].T.copy(order="F"), B[j].T.copy(order="F"), int(st[j])) for j in range(m)]

    # ---- restarted variants (restarted.jl) ----
    def restart(self, nblocks: int, S: np.ndarray) -> None:
        S = np.asfortranarray(S, dtype=np.float64)
        self._check(lib.rbl_restart(self._h, nblocks, dptr(S)), "rbl_restart")

    def lock(self, nblocks: int, S: np.ndarray) -> None:
        S = np.asfortranarray(S, dtype=np.float64)
        self._check(lib.rbl_lock(self._h, nblocks, S.shape[1], dptr(S)), "rbl_lock")

    def locked(self) -> np.ndarray:
        n, r0, r1, _ = self.matrix_info()
        L = lib.rbl_num_locked(self._h)
        V = np.zeros((r1 - r0, L), order="F")
        if L:
            self._check(lib.rbl_get_locked(self._h, dptr(V)), "rbl_get_locked")
        return V

    def reorth_last(self, nblocks: int, flags: int) -> None:
        self._check(lib.rbl_reorth_last(self._h, nblocks, flags), "rbl_reorth_last")

    # ---- thick restart (rbl.thick) ----
    def thick_restart(self, nblocks: int, S: np.ndarray, W: np.ndarray) -> None:
        """rbl_thick_restart after m = nblocks steps: the basis [Q_1 .. Q_m, Q_{m+1}] becomes
        [Q S, Q_{m+1}] in place.  S: (m b) x (kb b) chosen eigenvector columns of the projected
        matrix, W: b x (kb b) = B_{m+1} S[last b rows]; kb < m blocks are kept.  The next step is
        kb + 1, the arrow step U = Op Q_{m+1} - (Q S) W^T."""
        b = self.b
        S = np.asfortranarray(S, dtype=np.float64)
        W = np.asfortranarray(W, dtype=np.float64)
        if S.ndim != 2 or S.shape[0] != nblocks * b or S.shape[1] < b or S.shape[1] % b:
            raise ValueError(f"thick_restart: S must be {nblocks * b} x (keep_blocks * {b})")
        if W.shape != (b, S.shape[1]):
            raise ValueError(f"thick_restart: W must be {b} x {S.shape[1]}")
        self._check(lib.rbl_thick_restart(self._h, int(nblocks), S.shape[1] // b, dptr(S), dptr(W)),
                    "rbl_thick_restart")

    def bench_compress_pass(self, rows: int, b: int, m: int, keep_blocks: int, reps: int = 5):
        """(inplace_ms, sliced_ms) per pass of the in-place compression of m synthetic rows x b
        blocks to keep_blocks, and of the ceil(keep_blocks b / 64) out-of-place tall-skinny GEMMs
        it replaces (rbl_bench_compress_pass)."""
        im, sm = np.zeros(1), np.zeros(1)
        self._check(lib.rbl_bench_compress_pass(self._h, int(rows), int(b), int(m), int(keep_blocks),
                                                int(reps), dptr(im), dptr(sm)),
                    "rbl_bench_compress_pass")
        return float(im[0]), float(sm[0])

    def ritz(self, nblocks: int, k: int, S: np.ndarray) -> np.ndarray:
        n, r0, r1, _ = self.matrix_info()
        S = np.asfortranarray(S[: nblocks * self.b, :k], dtype=np.float64)
        V = np.zeros((r1 - r0, k), order="F")
        self._check(lib.rbl_ritz(self._h, nblocks, k, dptr(S), dptr(V)), "rbl_ritz")
        return V

    def get_block(self, j: int) -> np.ndarray:
        n, r0, r1, _ = self.matrix_info()
        Q = np.zeros((r1 - r0, self.b), order="F")
        self._check(lib.rbl_get_block(self._h, j, dptr(Q)), "rbl_get_block")
        return Q

    def num_blocks(self) -> int:
        return lib.rbl_num_blocks(self._h)

    # ---- Chebyshev filter and Rayleigh-Ritz on A (rbl.filtered) ----
    def set_filter(self, degree: int, lo: float = 0.0, hi: float = 0.0, ref: float = 0.0) -> None:
        """rbl_set_filter: later start / step calls run on p(A) = T_d((A - c)/e) / T_d((ref - c)/e)
        with [lo, hi] the damped interval; degree 0 clears the filter."""
        self._check(lib.rbl_set_filter(self._h, int(degree), float(lo), float(hi), float(ref)),
                    "rbl_set_filter")

    def set_filter_series(self, lo: float, hi: float, mu) -> None:
        """rbl_set_filter_series: later start / step calls run on the Chebyshev series p(A) =
        sum_j mu[j] T_j((A - c)/e) with [lo, hi] enclosing the whole spectrum (degree =
        len(mu) - 1 >= 1).  Replaces a set_filter; set_filter(0) clears it."""
        mu = np.ascontiguousarray(mu, dtype=np.float64).ravel()
        self._check(lib.rbl_set_filter_series(self._h, int(mu.size) - 1, float(lo), float(hi), dptr(mu)),
                    "rbl_set_filter_series")

    def apply_filter(self, X: np.ndarray) -> np.ndarray:
        """Y = p(A) X on the device (rbl_apply_filter); apply() stays the plain A X."""
        n, r0, r1, _ = self.matrix_info()
        X = np.asfortranarray(X, dtype=np.float64)
        Y = np.zeros((r1 - r0, X.shape[1]), order="F")
        self._check(lib.rbl_apply_filter(self._h, X.shape[1], dptr(X), dptr(Y)), "rbl_apply_filter")
        return Y

    def cheb_moments(self, b: int, degree: int, lo: float, hi: float, X=None, seed: int = 0) -> np.ndarray:
        """rbl_cheb_moments: mom[j, c] = x_c^T T_j((A - cI)/e) x_c, j = 0..2 degree, shape
        (2 degree + 1, b), from `degree` SpMMs.  [lo, hi] must enclose the whole spectrum.  X: n x b
        host block, or None for the device's N(0,1) draw from `seed` (rbl.density turns the moments
        into a spectral density and eigenvalue counts)."""
        b, degree = int(b), int(degree)
        xp = None
        if X is not None:
            n, r0, r1, _ = self.matrix_info()
            X = np.asfortranarray(X, dtype=np.float64)
            if X.ndim != 2 or X.shape != (r1 - r0, b):
                raise ValueError(f"cheb_moments: X must be {r1 - r0} x {b}")
            xp = dptr(X)
        mom = np.zeros((max(2 * degree + 1, 1), max(b, 1)), order="F")
        self._check(lib.rbl_cheb_moments(self._h, b, degree, float(lo), float(hi), xp, int(seed) & (2**64 - 1),
                                         dptr(mom)), "rbl_cheb_moments")
        return mom

    def cheb_diag(self, b: int, lo: float, hi: float, coef, X=None, seed: int = 0, probe="sign"):
        """rbl_cheb_diag: (num, den) with num[row, e] = sum_c x_c[row] (p_e(A) x_c)[row] and
        den[row] = sum_c x_c[row]^2 over a block of b vectors, p_e = sum_j coef[j, e] T_j((A - cI)/e),
        from ONE recurrence of degree = coef.shape[0] - 1 >= 1 SpMMs for all nf = coef.shape[1] <= 32
        series (a 1-D coef is one series); num / den[:, None] estimates the diagonals.  [lo, hi]
        must enclose the whole spectrum.  X: n x b host block (b <= 256), or None for the device's
        draw from `seed`: probe "sign" (+-1) or "gauss" (N(0,1)).  rbl.funm builds on it."""
        b = int(b)
        coef = np.asarray(coef, dtype=np.float64)
        if coef.ndim == 1:
            coef = coef[:, None]
        if coef.ndim != 2:
            raise ValueError("cheb_diag: coef must be (degree + 1) x nf")
        coef = np.asfortranarray(coef)
        degree, nf = coef.shape[0] - 1, coef.shape[1]
        if isinstance(probe, str):
            try:
                probe = {"gauss": _lib.RBL_PROBE_GAUSS, "sign": _lib.RBL_PROBE_SIGN}[probe]
            except KeyError:
                raise ValueError('cheb_diag: probe must be "sign" or "gauss"') from None
        n, r0, r1, _ = self.matrix_info()
        xp = None
        if X is not None:
            X = np.asfortranarray(X, dtype=np.float64)
            if X.ndim != 2 or X.shape != (r1 - r0, b):
                raise ValueError(f"cheb_diag: X must be {r1 - r0} x {b}")
            xp = dptr(X)
        num = np.zeros((max(r1 - r0, 1), max(nf, 1)), order="F")
        den = np.zeros(max(r1 - r0, 1))
        self._check(lib.rbl_cheb_diag(self._h, b, degree, float(lo), float(hi), nf, dptr(coef), xp,
                                      int(seed) & (2**64 - 1), int(probe), dptr(num), dptr(den)),
                    "rbl_cheb_diag")
        return num[: r1 - r0], den[: r1 - r0]

    def ritz_project(self, nblocks: int, k: int, S: np.ndarray) -> np.ndarray:
        """rbl_ritz_project: V = [Q_1..Q_nblocks] S and W = A V stay on the device; returns
        H = V^T W (k x k)."""
        S = np.asfortranarray(S[: nblocks * self.b, :k], dtype=np.float64)
        H = np.zeros((k, k), order="F")
        self._check(lib.rbl_ritz_project(self._h, nblocks, k, dptr(S), dptr(H)), "rbl_ritz_project")
        return H

    def ritz_finish(self, Y: np.ndarray, theta: np.ndarray):
        """rbl_ritz_finish with H = Y diag(theta) Y^T: returns (V Y, the true residual norms
        ||A v_j - theta_j v_j||_2).  Y may hold only k chosen columns of the projected width kk
        (kk x k, theta of length k: rbl_ritz_finish_cols)."""
        n, r0, r1, _ = self.matrix_info()
        Y = np.asfortranarray(Y, dtype=np.float64)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        k = theta.size
        if Y.ndim != 2 or Y.shape[1] != k or Y.shape[0] < k:
            raise ValueError("ritz_finish: Y must be kk x k (kk >= k) and theta of length k")
        V = np.zeros((r1 - r0, k), order="F")
        res = np.zeros(k)
        if Y.shape[0] == k:
            self._check(lib.rbl_ritz_finish(self._h, k, dptr(Y), dptr(theta), dptr(V), dptr(res)),
                        "rbl_ritz_finish")
        else:
            self._check(lib.rbl_ritz_finish_cols(self._h, Y.shape[0], k, dptr(Y), dptr(theta), dptr(V),
                                                 dptr(res)), "rbl_ritz_finish_cols")
        return V, res

    def timers(self) -> dict:
        names = _lib.stage_names()
        ms = np.zeros(len(names))
        self._check(lib.rbl_timers(self._h, dptr(ms), len(names)), "rbl_timers")
        return dict(zip(names, ms.tolist()))

    def reset_timers(self) -> None:
        self._check(lib.rbl_reset_timers(self._h), "rbl_reset_timers")

    def device_memory(self) -> tuple:
        """(free, total) bytes of the context's GPU (rbl_device_memory)."""
        f, t = np.zeros(1, np.int64), np.zeros(1, np.int64)
        self._check(lib.rbl_device_memory(self._h, i64ptr(f), i64ptr(t)), "rbl_device_memory")
        return int(f[0]), int(t[0])

    def comm_info(self) -> dict:
        """Ranks as the transport counts them (RCCL: ncclCommCount), this rank, transport name."""
        import ctypes as C
        n, r = C.c_int(0), C.c_int(0)
        buf = C.create_string_buffer(32)
        self._check(lib.rbl_comm_info(self._h, C.byref(n), C.byref(r), buf, 32), "rbl_comm_info")
        out = {"nranks": n.value, "rank": r.value, "transport": buf.value.decode()}
        if out["transport"] == "rccl":
            out.update(rccl_version())
        return out

    def comm_stats(self, reset: bool = False, times: bool = False) -> dict:
        """Collectives this rank issued since the last reset (rbl_comm_stats): all-reduce
        calls / bytes, halo exchanges, bytes sent / received; and the halo plan of the matrix
        held (not reset): halo_push (the push/pull split runs, RBL_OPT_HALO_PUSH) and the Q rows
        per SpMM summed over ranks its setup predicted with the split / with the pull-all halo;
        with times=True also the time in the collectives (ns): host wall time inside the
        transport calls, and their hipEvent spans on the streams (recorded only while
        RBL_OPT_TIMERS is 1)."""
        out = np.zeros(12, np.int64)
        self._check(lib.rbl_comm_stats(self._h, i64ptr(out), 12, int(reset)), "rbl_comm_stats")
        keys = ("allreduce_calls", "allreduce_bytes", "exchange_calls", "send_bytes",
                "recv_bytes", "halo_push", "push_rows_pred", "pull_rows_pred")
        if times:  # (timings differ run to run: counts-only dicts compare across runs)
            keys += ("allreduce_host_ns", "exchange_host_ns", "allreduce_dev_ns", "exchange_dev_ns")
        return dict(zip(keys, (int(x) for x in out)))

    def path_stats(self, reset: bool = False) -> dict:
        """Which code path the steps took since the last reset (rbl_path_stats), counted as the
        work is issued: SpMM launches, those that applied the local-reorth update, separate
        local-reorth passes and Grams, the fused path's edge fix-ups, two-wave SpMM launches
        (variants build only), rbl_ritz calls that took the row-piece form, and local-reorth
        coefficients taken from the 3-term pass or derived through the partial reorth
        (RBL_OPT_CLOC_DERIVE).  upd32_taken / upd32_refused: partial-reorth updates the device
        gate sent to the fp32-MFMA kernel or kept on the fp64 one (RBL_OPT_UPD32), counted on the
        device and read back after a stream synchronise; upd32_shadow_read / upd32_shadow_conv:
        basis panels that kernel read from the fp32 shadow / rounded and stored to it
        (RBL_OPT_UPD32_SHADOW, device counts too); upd32_shadow_bytes: the bytes of the shadow the
        current run plan holds (0: none; not a counter, a reset leaves it)."""
        from . import _lib as L
        out = np.zeros(L.RBL_PATH_NSTATS, np.int64)
        self._check(lib.rbl_path_stats(self._h, i64ptr(out), L.RBL_PATH_NSTATS, int(reset)),
                    "rbl_path_stats")
        return dict(zip(("spmm", "spmm_loc_fused", "loc_separate", "loc_gram", "locfix_edges",
                         "locfix_rest", "spmm_two_wave", "ritz_pieces", "cloc_3term",
                         "cloc_reorth", "upd32_taken", "upd32_refused", "upd32_shadow_read",
                         "upd32_shadow_conv", "upd32_shadow_bytes"), (int(x) for x in out)))

    def upd32_gate_values(self) -> np.ndarray:
        """Diagnostics (rbl_upd32_gate_values): the RBL_OPT_UPD32 gate's g of block step i at
        [i % 64], 0 where the gate has not run."""
        out = np.zeros(64, np.float64)
        self._check(lib.rbl_upd32_gate_values(self._h, dptr(out), 64), "rbl_upd32_gate_values")
        return out

    def shadow_valid(self) -> int:
        """Diagnostics (rbl_shadow_valid): the leading blocks whose fp32 shadow is current
        (RBL_OPT_UPD32_SHADOW; 0 without a shadow)."""
        return int(lib.rbl_shadow_valid(self._h))

    def get_shadow_block(self, j: int) -> np.ndarray:
        """Diagnostics (rbl_get_shadow_block): the fp32 shadow of block j (1-based as get_block,
        j <= shadow_valid()), n_local x 32."""
        import ctypes as C
        n, r0, r1, _ = self.matrix_info()
        out = np.zeros((r1 - r0, 32), np.float32)
        self._check(lib.rbl_get_shadow_block(self._h, j, out.ctypes.data_as(C.POINTER(C.c_float))),
                    "rbl_get_shadow_block")
        return out

    def allgather(self, values) -> np.ndarray:
        """rbl_allgather_host: every rank's int64 values, shape (nranks, len(values)); ordered
        after the work enqueued on this context (a collective: every rank calls it)."""
        mine = np.ascontiguousarray(np.asarray(values, dtype=np.int64).ravel())
        out = np.zeros(self.nranks * mine.size, np.int64)
        self._check(lib.rbl_allgather_host(self._h, i64ptr(mine), i64ptr(out), mine.size),
                    "rbl_allgather_host")
        return out.reshape(self.nranks, mine.size)

    def synchronize(self) -> None:
        self._check(lib.rbl_synchronize(self._h), "rbl_synchronize")


@dataclass
class RBLInfo:
    iters: int = 0
    nblocks: int = 0
    converged: bool = False
    status: int = 0
    qr_shifted_steps: int = 0
    eig_ms: float = 0.0          # host T-band eigensolves (dsbev / dsbevd)
    fetch_ms: float = 0.0        # host waits in rbl_fetch (the GPU finishing enqueued steps)
    ritz_ms: float = 0.0         # host wall time of rbl_ritz (device work + D2H of V)
    start_ms: float = 0.0        # host wall time of rbl_start (A Omega + QR)
    enqueue_ms: float = 0.0      # host time inside rbl_step_async (enqueueing the steps)
    spec_steps: int = 0          # steps enqueued ahead of a convergence check (speculate)
    spec_wasted: int = 0         # of those, steps past the converging check (discarded)
    resid: list = field(default_factory=list)   # max residual bound at each check
    trace_A: list = field(default_factory=list)
    trace_B: list = field(default_factory=list)
    restarts: int = 0            # thick restarts taken (rbl.thick; 0 for an unrestarted run)
    op_applies: int = 0          # block applications of the operator, the start block included
    peak_blocks: int = 0         # the most basis blocks held at once


def rccl_version() -> dict:
    """The RCCL the library's RCCL transport calls (rbl_rccl_version: ROCm's own, opened by path
    whatever copy the process loaded first): {"rccl_version": "2.27.7", "rccl_version_code":
    22707, "rccl_path": file}.  No GPU call."""
    import ctypes as C
    v = C.c_int(0)
    buf = C.create_string_buffer(512)
    st = lib.rbl_rccl_version(C.byref(v), buf, 512)
    if st != 0:
        raise RBLError(st, f"rbl_rccl_version: {buf.value.decode()}")
    code = v.value
    # NCCL_VERSION(X,Y,Z): X*10000 + Y*100 + Z from 2.9 on
    return {"rccl_version": f"{code // 10000}.{code // 100 % 100}.{code % 100}",
            "rccl_version_code": code, "rccl_path": buf.value.decode()}


def set_update(ctx: Context, update) -> None:
    """The ``update=(P, S)`` keyword of the drivers: the operator A + P S P^T, set straight after
    the matrix (so bound estimation sees the updated operator); None: the plain A.  A callable is
    called with the loaded context and returns the pair (``rbl.kernelop.kernel_centering_update``)."""
    if update is None:
        return
    if callable(update):
        update = update(ctx)
    try:
        P, S = update
    except (TypeError, ValueError):
        raise ValueError("update must be a pair (P, S)") from None
    ctx.set_lowrank(P, S)


def max_steps_for(kryl_sz: int, b: int) -> int:
    """Number of block steps the loop `while i*b < kryl_sz` can run (RBL_gpu.jl:162)."""
    return max(1, math.ceil(kryl_sz / b))


def lanczos(ctx: Context, k: int, b: int, *, kryl_sz: int = KRYL_SZ_GPU, omega=None, seed=0,
            check: bool = True, max_steps: int | None = None, tol: float = RESIDUAL_TOL,
            trace: bool = False, ritz: bool = True, basis_bits: int = 64,
            speculate: "bool | int | str" = "auto"):
    """RBL_gpu.jl:134-203 + :219 on an already-loaded context.  Returns (D, V_local, info)."""
    steps_cap = max_steps_for(kryl_sz, b)
    if max_steps is not None:
        steps_cap = min(steps_cap, max_steps)
    info = RBLInfo()
    t0 = time.perf_counter()
    ctx.start(b, steps_cap, omega=omega, seed=seed, basis_bits=basis_bits)
    info.start_ms = (time.perf_counter() - t0) * 1e3
    T = TBand(b, steps_cap)
    D = np.zeros(0)
    S = np.zeros((0, 0))

    def _record(A, B, st):
        if st == _lib.RBL_WARN_QR_SHIFTED:
            info.qr_shifted_steps += 1
        if trace:
            info.trace_A.append(A.copy())
            info.trace_B.append(B.copy())

    # Steps are enqueued without a host round trip (rbl_step_async) and fetched where the host
    # needs the T band: at a convergence check (:186) and after the last step.  T receives the
    # same A_i / B_i in the same order as the reference's per-step pushes (:185, :193).
    # Speculation: before the host blocks at a check and solves the T band (dsbev, up to ~35 ms at
    # N = 896), it may enqueue further steps, so the GPU keeps working during the eigensolve.  The
    # check reads only steps <= i, and steps after an even i touch no block <= i (partial reorth
    # at even steps), so D, S and the Ritz vectors are unchanged; a converged run discards the
    # extra steps, which is the cost.  speculate="auto" (default) enqueues up to the next check
    # when the residual bounds of the previous two checks, extrapolated geometrically, put this
    # check at least 100x above the tolerance, and one step when they put it above the tolerance
    # (host.speculation_depth) — on several ranks agreed once per check together with the
    # convergence test (rank 0's decisions, below), so ranks issue the same steps.
    # True: as many steps as the eigensolve is expected to last (the previous one scaled by
    # (N/N_prev)^2.7, over the measured time per step; one rank only); an int: a fixed count (tests).
    last_i = min(steps_cap, math.ceil(kryl_sz / b))
    enq = 0
    # Several ranks: each rank solves the same T band on its own host, and every rank must
    # enqueue the same steps (their collectives pair up).  So the two decisions a check takes —
    # converged, and (auto) how far to speculate before the next check — are all-gathered once
    # per check (rbl_allgather_host) and rank 0's are taken by every rank: eigensolves that
    # differ in the last bit across ranks (BLAS threading) cannot split the ranks' step counts.
    multi = ctx.nranks > 1
    next_depth = 0                                 # agreed auto depth for the next check

    def enqueue(upto):
        nonlocal enq
        t0 = time.perf_counter()
        while enq < upto:
            enq += 1
            ctx.step_async(enq, enq >= 2 and enq % 2 == 0)   # :164-184
        info.enqueue_ms += (time.perf_counter() - t0) * 1e3

    first = 1                                      # first unfetched step
    i = 0
    last_eig = last_n = None
    step_ms = None
    t_prev, i_prev, eig_prev = time.perf_counter(), 0, 0.0
    while True:
        i += 1                                     # step 1: first loop, :149-161; then :162-194
        is_check = check and i >= 2 and i * b > k and i % 4 == 0
        is_last = not (i * b < kryl_sz and i < steps_cap)
        if not (is_check or is_last):
            continue
        enqueue(i)
        # (one rank only: the count comes from host timings, and every rank must issue the
        # same steps — their collectives pair up)
        # (speculate may also be a fixed count of extra steps per check: tests)
        spec_to = i
        if speculate is not False and is_check and not is_last and i % 2 == 0:
            if speculate == "auto":
                spec_to = i + (next_depth if multi else speculation_depth(info.resid, tol))
            elif speculate is True:
                if ctx.nranks == 1 and last_eig and step_ms:
                    spec_to = i + int(last_eig * (i * b / last_n) ** 2.7 // step_ms)
            else:
                spec_to = i + int(speculate)
            spec_to = min(last_i, i + 4, spec_to)
            if spec_to > i:
                info.spec_steps += spec_to - i
                enqueue(spec_to)
        t0 = time.perf_counter()
        fetched = ctx.fetch(first, i + 1)
        t1 = time.perf_counter()
        info.fetch_ms += (t1 - t0) * 1e3
        if i > i_prev and t1 - t_prev > eig_prev:  # GPU time per step since the last fetch
            step_ms = ((t1 - t_prev) - eig_prev) * 1e3 / (i - i_prev)
        t_prev, i_prev, eig_prev = t1, i, 0.0
        for j, (Aj, Bj, st) in zip(range(first, i + 1), fetched):
            _record(Aj, Bj, st)
            T.insert_A(Aj)                         # :185
            if j == i and is_check:
                t0 = time.perf_counter()
                D, S = eig_topk(T.view(), k)       # :187-188
                dt = time.perf_counter() - t0
                info.eig_ms += dt * 1e3
                eig_prev = dt
                last_eig, last_n = dt * 1e3, i * b
                res = residual_norms(Bj, S, b, k)
                info.resid.append(float(res.max()) if res.size else 0.0)
                conv = bool(np.all(res <= tol))            # :189 (check_convergence)
                if multi:
                    depth = speculation_depth(info.resid, tol) if speculate == "auto" else 0
                    agreed = ctx.allgather([int(conv), depth])[0]   # rank 0's decisions
                    conv, next_depth = bool(agreed[0]), int(agreed[1])
                if conv:
                    info.converged = True
                    info.spec_wasted += spec_to - i
                    break
            T.insert_B(Bj, j)                      # :193
        first = i + 1
        if info.converged or is_last:
            break
    info.iters = i
    info.nblocks = i                               # Q_1..Q_i (length(Q))
    info.op_applies = enq + 1                      # A Omega and every enqueued step
    info.peak_blocks = enq + 1
    D = D[::-1].copy()
    # each Ritz vector's sign: its coefficient column's largest entry positive (host.fix_signs;
    # the eigensolvers disagree on signs, the reference returns dsbev's)
    S = fix_signs(S[:, ::-1])
    info.status = _lib.RBL_OK if info.converged else _lib.RBL_WARN_NOT_CONVERGED
    V = None
    if ritz and S.size:
        t0 = time.perf_counter()
        V = ctx.ritz(S.shape[0] // b, min(k, S.shape[1]), S)   # RBL_gpu.jl:219
        info.ritz_ms = (time.perf_counter() - t0) * 1e3
    return D, V, info


def RBL_gpu(A, k: int, b: int, *, device: int = 0, kryl_sz: int = KRYL_SZ_GPU, omega=None,
            seed: int = 0, reorth_order: int = 0, return_info: bool = False, basis_bits: int = 64,
            device_blocks: int = 0, update=None):
    """Drop-in for ``RBL_gpu(A::SparseMatrixCSC{Float64}, k, b)`` (RBL_gpu.jl:205):
    returns (D, V) — D the k largest-|lambda| eigenvalues (descending |lambda|), V n x k.
    device_blocks: Krylov blocks kept in HBM (RBL_OPT_DEVICE_BLOCKS: 0 all, -1 what fits —
    the reference's gpu_buffer_size — or G >= 3; older blocks spill to pinned host memory).
    update=(P, S): the eigenpairs of A + P S P^T, never formed (Context.set_lowrank; rbl.lowrank
    builds the usual ones; fp64 basis)."""
    with Context(device) as ctx:
        ctx.set_matrix(A)
        set_update(ctx, update)
        ctx.set_option(_lib.RBL_OPT_REORTH_ORDER, reorth_order)
        ctx.set_option(_lib.RBL_OPT_DEVICE_BLOCKS, device_blocks)
        D, V, info = lanczos(ctx, k, b, kryl_sz=kryl_sz, omega=omega, seed=seed,
                             basis_bits=basis_bits)
    return (D, V, info) if return_info else (D, V)
