"""Implicit kernel matrices: eigenpairs and f(K) from the points alone.

``KernelMatrix(X, kind, gamma, ...)`` describes the operator

    Op = diag(s) K diag(s) + nugget I,    K_ij = kappa(x_i, x_j),

over the n rows of X (n x d) without ever forming it: ``Context.set_matrix`` uploads the n x d points
(rbl_set_matrix_kernel) and every product Op Q evaluates K tile by tile on the device.  Every driver
that takes a matrix takes a KernelMatrix: ``RBL_gpu`` / ``RBL_thick`` (the leading eigenpairs),
``RBL_filtered``, ``trace_function`` / ``logdet`` (log det(K + tau I) of a Gaussian process),
``apply_function`` ((K + tau I)^-1 y through f = 1 / x), ``spectral_density``.

  kappa:  "rbf"      exp(-gamma |x - y|^2)
          "laplace"  exp(-gamma |x - y|_2)
          "poly"     (gamma x^T y + coef0)^degree,  1 <= degree <= 8

``kernel_centering_update(ctx)`` is ``rbl.lowrank.centering_update`` for the kernel matrix a context
holds, from one product with the ones vector; ``RBL_kernel_pca`` and ``RBL_spectral_embedding`` are
kernel PCA and the normalised spectral embedding on top of these.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .rbl_gpu import Context, lanczos

KINDS = {"rbf": _lib.RBL_KERNEL_RBF, "laplace": _lib.RBL_KERNEL_LAPLACE, "poly": _lib.RBL_KERNEL_POLY}


class KernelMatrix:
    """The n x n operator diag(scale) K diag(scale) + nugget I over the rows of X (n x d), K_ij =
    kappa(x_i, x_j); nothing of size n^2 is formed except by ``toarray()`` (tests, small n)."""

    ndim = 2

    def __init__(self, X, kind: str = "rbf", gamma: float = 1.0, coef0: float = 0.0, degree: int = 3,
                 scale=None, nugget: float = 0.0):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(-1, 1)
        if X.ndim != 2 or X.shape[0] < 1:
            raise ValueError("KernelMatrix: X must be an n x d array with n >= 1")
        if not 1 <= X.shape[1] <= _lib.RBL_KERNOP_MAX_DIM:
            raise ValueError(f"KernelMatrix: d = {X.shape[1]} must be in [1, {_lib.RBL_KERNOP_MAX_DIM}]")
        if not np.all(np.isfinite(X)):
            raise ValueError("KernelMatrix: X has a non-finite entry")
        if kind not in KINDS:
            raise ValueError("KernelMatrix: kind must be 'rbf', 'laplace' or 'poly'")
        if isinstance(gamma, bool) or not np.isscalar(gamma) or not np.isfinite(gamma) or not gamma > 0:
            raise ValueError("KernelMatrix: gamma must be a finite number > 0")
        if not np.isscalar(coef0) or not np.isfinite(coef0):
            raise ValueError("KernelMatrix: coef0 must be finite")
        if isinstance(degree, bool) or not isinstance(degree, (int, np.integer)) or not 1 <= degree <= 8:
            raise ValueError("KernelMatrix: degree must be an integer in [1, 8]")
        if not np.isscalar(nugget) or not np.isfinite(nugget):
            raise ValueError("KernelMatrix: nugget must be finite")
        if scale is not None:
            scale = np.ascontiguousarray(scale, dtype=np.float64)
            if scale.shape != (X.shape[0],):
                raise ValueError(f"KernelMatrix: scale must have n = {X.shape[0]} entries")
            if not np.all(np.isfinite(scale)):
                raise ValueError("KernelMatrix: scale has a non-finite entry")
        self.X = np.asfortranarray(X)
        self.kind = kind
        self.gamma = float(gamma)
        self.coef0 = float(coef0)
        self.degree = int(degree)
        self.scale = scale
        self.nugget = float(nugget)

    @property
    def n(self) -> int:
        return self.X.shape[0]

    @property
    def d(self) -> int:
        return self.X.shape[1]

    @property
    def shape(self):
        return (self.n, self.n)

    def kernel_array(self) -> np.ndarray:
        """K alone (no scale, no nugget) as a host fp64 array, distances by direct differences."""
        X = self.X
        if self.kind == "poly":
            return (self.gamma * (X @ X.T) + self.coef0) ** self.degree
        d2 = np.zeros((self.n, self.n))
        for c in range(self.d):
            d2 += np.subtract.outer(X[:, c], X[:, c]) ** 2
        return np.exp(-self.gamma * (d2 if self.kind == "rbf" else np.sqrt(d2)))

    def toarray(self) -> np.ndarray:
        """The operator as a host fp64 n x n array — tests and small n only."""
        K = self.kernel_array()
        if self.scale is not None:
            K = self.scale[:, None] * K * self.scale[None, :]
        if self.nugget != 0.0:
            K[np.diag_indices(self.n)] += self.nugget
        return K


def kernel_centering_update(ctx: Context):
    """(P, S) of ``centering_update`` for the kernel matrix ``ctx`` holds: P = [1, Op 1 / n], S =
    [[1^T Op 1 / n^2, -1], [-1, 0]], so Op + P S P^T = H Op H — from one ``ctx.apply`` on the ones
    vector, no n^2 pass.  It is a callable ``update=`` of the drivers:
    ``RBL_gpu(K, k, b, update=kernel_centering_update)``."""
    n = ctx.kernel_info()["n"]
    m = ctx.apply(np.ones((n, 1), order="F"))[:, 0] / n
    c = float(m.sum()) / n
    P = np.empty((n, 2), order="F")
    P[:, 0] = 1.0
    P[:, 1] = m
    return P, np.array([[c, -1.0], [-1.0, 0.0]])


def _check_kb(what, n, k, b):
    for name, v in (("k", k), ("b", b)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{what}: {name} must be an integer >= 1")
    if k > n:
        raise ValueError(f"{what}: k = {k} exceeds n = {n}")


def _run(ctx, k, b, max_blocks, omega, seed):
    if max_blocks is None:
        return lanczos(ctx, k, b, omega=omega, seed=seed)
    from .thick import lanczos_thick
    return lanczos_thick(ctx, k, b, max_blocks=max_blocks, omega=omega, seed=seed)


def RBL_kernel_pca(X, k: int, b: int, *, kind: str = "rbf", gamma: float = 1.0, coef0: float = 0.0,
                   degree: int = 3, max_blocks=None, omega=None, seed: int = 0, device: int = 0,
                   return_info: bool = False):
    """Kernel PCA of the n points X (n x d): the k leading eigenpairs of H K H, H = I - 1 1^T / n.
    Returns (lam, V, scores): lam descending, V n x k orthonormal, scores = V sqrt(lam) (the
    coordinates of the points on the k principal axes in feature space).  K is never formed: the
    operator is loaded once and the centring enters as a rank-two update from one product with the
    ones vector.  For "rbf" and "laplace" the points are mean-centred on the host first (K is
    unchanged; the Gram-form cancellation on the device stays small).  max_blocks: the thick-restart
    loop in a basis of max_blocks + 1 blocks instead of the unrestarted one."""
    K = KernelMatrix(X, kind=kind, gamma=gamma, coef0=coef0, degree=degree)
    _check_kb("RBL_kernel_pca", K.n, k, b)
    if kind != "poly":
        K.X = np.asfortranarray(K.X - K.X.mean(axis=0))
    with Context(device) as ctx:
        ctx.set_matrix(K)
        ctx.set_lowrank(*kernel_centering_update(ctx))
        lam, V, info = _run(ctx, k, b, max_blocks, omega, seed)
    scores = V * np.sqrt(np.maximum(lam, 0.0))
    return (lam, V, scores, info) if return_info else (lam, V, scores)


def row_normalize(V) -> np.ndarray:
    """The rows of V scaled to unit length (a zero row stays zero)."""
    V = np.asarray(V, dtype=np.float64)
    nrm = np.linalg.norm(V, axis=1, keepdims=True)
    return V / np.where(nrm > 0.0, nrm, 1.0)


def RBL_spectral_embedding(X, k: int, b: int, *, kind: str = "rbf", gamma: float = 1.0,
                           coef0: float = 0.0, degree: int = 3, max_blocks=None, omega=None,
                           seed: int = 0, device: int = 0, return_info: bool = False):
    """The normalised spectral embedding of the n points X (Ng, Jordan & Weiss): the k leading
    eigenpairs of D^-1/2 K D^-1/2 with D = diag(K 1).  The degrees come from one product with the
    ones vector and enter as the operator's scale, so K is never formed.  Returns (lam, V, Y): lam
    descending, V n x k, Y the rows of V normalised to unit length — points of one cluster share a
    direction, so any clustering of Y's rows (k-means is not part of this library) labels them."""
    K = KernelMatrix(X, kind=kind, gamma=gamma, coef0=coef0, degree=degree)
    _check_kb("RBL_spectral_embedding", K.n, k, b)
    if kind != "poly":
        K.X = np.asfortranarray(K.X - K.X.mean(axis=0))
    with Context(device) as ctx:
        ctx.set_matrix(K)
        deg = ctx.apply(np.ones((K.n, 1), order="F"))[:, 0]
        if not np.all(deg > 0.0):
            raise ValueError("RBL_spectral_embedding: a point has degree K 1 <= 0")
        ctx.set_kernel_scale(deg ** -0.5)
        lam, V, info = _run(ctx, k, b, max_blocks, omega, seed)
    Y = row_normalize(V)
    return (lam, V, Y, info) if return_info else (lam, V, Y)
