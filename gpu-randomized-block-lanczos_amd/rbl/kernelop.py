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

A fit is used on points outside the training set through the cross-kernel matrix kappa(Z, X) (m new
points against the n stored ones), which ``Context.kernel_cross`` multiplies into a block without
forming it: ``kernel_pca_fit(...).transform(Z)``, ``spectral_embedding_fit(...).transform(Z)`` (the
Nystrom extension) and ``gp_fit(...).predict(Z, return_var=True)`` / ``.log_marginal_likelihood()``.

``RBL_spectral_embedding`` and ``spectral_embedding_fit`` take ``neighbors=m`` to run on the
m-nearest-neighbour graph of the points (``rbl.knn``) through the sparse eigensolver instead.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .rbl_gpu import Context, lanczos

KINDS = {"rbf": _lib.RBL_KERNEL_RBF, "laplace": _lib.RBL_KERNEL_LAPLACE, "poly": _lib.RBL_KERNEL_POLY}
# the weight Phi of Context.kernel_hadamard: kappa, d kappa / d gamma, the factor of d kappa / d log s_k
WEIGHTS = {"value": _lib.RBL_KWEIGHT_VALUE, "dgamma": _lib.RBL_KWEIGHT_DGAMMA, "dscale": _lib.RBL_KWEIGHT_DSCALE}


def _new_points(what, Z, d):
    """Z as an m x d fp64 array (a vector is m x 1 for d = 1, one point otherwise), finite, m >= 1."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim == 1:
        Z = Z.reshape(-1, 1) if d == 1 else Z.reshape(1, -1)
    if Z.ndim != 2 or Z.shape[0] < 1 or Z.shape[1] != d:
        raise ValueError(f"{what}: Z must be an m x d array with m >= 1 and d = {d}")
    if not np.all(np.isfinite(Z)):
        raise ValueError(f"{what}: Z has a non-finite entry")
    return Z


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

    def cross_array(self, Z) -> np.ndarray:
        """kappa(Z, X) alone (no scale) as a host fp64 m x n array, distances by direct differences —
        tests and small sizes only; the device product is ``Context.kernel_cross``."""
        Z = _new_points("KernelMatrix.cross_array", Z, self.d)
        X = self.X
        if self.kind == "poly":
            return (self.gamma * (Z @ X.T) + self.coef0) ** self.degree
        d2 = np.zeros((Z.shape[0], self.n))
        for c in range(self.d):
            d2 += np.subtract.outer(Z[:, c], X[:, c]) ** 2
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


def _run(ctx, k, b, max_blocks, omega, seed, tol=None):
    kw = {} if tol is None else {"tol": float(tol)}
    if max_blocks is None:
        return lanczos(ctx, k, b, omega=omega, seed=seed, **kw)
    from .thick import lanczos_thick
    return lanczos_thick(ctx, k, b, max_blocks=max_blocks, omega=omega, seed=seed, **kw)


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
                           seed: int = 0, device: int = 0, return_info: bool = False, neighbors=None,
                           mode: str = "union", weight: str = "binary"):
    """The normalised spectral embedding of the n points X (Ng, Jordan & Weiss): the k leading
    eigenpairs of D^-1/2 K D^-1/2 with D = diag(K 1).  The degrees come from one product with the
    ones vector and enter as the operator's scale, so K is never formed.  Returns (lam, V, Y): lam
    descending, V n x k, Y the rows of V normalised to unit length — points of one cluster share a
    direction, so any clustering of Y's rows labels them (``rbl.RBL_spectral_clustering`` runs the
    device k-means of ``rbl.kmeans`` on them and returns the labels).

    neighbors=m: the affinity is the m-nearest-neighbour graph of the points instead (``rbl.knn``:
    one device sweep builds the lists, ``graph_from_knn`` with ``mode`` and ``weight`` the graph A;
    weight="rbf" uses ``gamma``), and D^-1/2 A D^-1/2, D = diag(A 1), goes to the sparse eigensolver as
    an ordinary CSR matrix.  ValueError naming the count if a vertex has degree 0 (mode="mutual"
    leaves isolated vertices); ``kind`` must be a radial kernel.  The same return tuple."""
    if neighbors is not None:
        from .knn import knn_affinity
        K, _, N, _ = knn_affinity("RBL_spectral_embedding", X, neighbors, mode, weight, kind, gamma, device)
        _check_kb("RBL_spectral_embedding", K.n, k, b)
        with Context(device) as ctx:
            ctx.set_matrix(N)
            lam, V, info = _run(ctx, k, b, max_blocks, omega, seed)
        Y = row_normalize(V)
        return (lam, V, Y, info) if return_info else (lam, V, Y)
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


# ---- fits that can be used on points outside the training set: every such use is one product with
# ---- the cross-kernel matrix kappa(Z, X) (Context.kernel_cross), which is never formed

def cross_splits(rows: int, cols: int, d: int) -> int:
    """The number of splits of the column range ``Context.kernel_cross`` uses for a rows x cols
    product in d dimensions (rbl_kernel_cross_splits): a function of the three numbers alone."""
    s = _lib.lib.rbl_kernel_cross_splits(int(rows), int(cols), int(d))
    if s < 1:
        raise ValueError("cross_splits: needs rows >= 1, cols >= 1 and 1 <= d <= "
                         f"{_lib.RBL_KERNOP_MAX_DIM}")
    return int(s)


# The residual the fits iterate to: a model's eigenpairs are multiplied into every later transform
# (an eigenvector's error enters lam^-1/2 or lam^-1 times), so they are taken well below the drivers'
# RESIDUAL_TOL
FIT_TOL = 1e-10


class _KernelFit:
    """What the three models share: the kernel matrix over the (shifted) training points and the
    shift new points get before they meet it."""

    def __init__(self, K: KernelMatrix, shift, device: int):
        self.K = K
        self.shift = shift
        self.device = device

    def _points(self, what, Z):
        return np.asfortranarray(_new_points(what, Z, self.K.d) - self.shift)


def _centred_kernel(what, X, kind, gamma, coef0, degree, **kw):
    """KernelMatrix over X, mean-centred for the two radial kernels (K is unchanged by a shift and
    the Gram-form cancellation on the device stays small); (K, the shift)."""
    K = KernelMatrix(X, kind=kind, gamma=gamma, coef0=coef0, degree=degree, **kw)
    shift = np.zeros(K.d)
    if kind != "poly":
        shift = K.X.mean(axis=0)
        K.X = np.asfortranarray(K.X - shift)
    return K, shift


class KernelPCAModel(_KernelFit):
    """A fitted kernel PCA (``kernel_pca_fit``).  lam (k, descending, all > 0), V (n x k
    orthonormal) the eigenpairs of H K H; scores = V sqrt(lam), the training points' coordinates;
    col_mean = K 1 / n and grand_mean = 1^T K 1 / n^2, the training means the centring of a new
    point needs; X the training points as the kernel sees them (minus ``shift`` for the radial
    kernels)."""

    def __init__(self, K, shift, device, lam, V, col_mean, grand_mean, info):
        super().__init__(K, shift, device)
        self.lam, self.V, self.scores = lam, V, V * np.sqrt(lam)
        self.col_mean, self.grand_mean, self.info = col_mean, grand_mean, info

    @property
    def X(self):
        return self.K.X

    def transform(self, Z) -> np.ndarray:
        """The coordinates of the m points Z on the k principal axes:
        (kappa(Z, X) - r 1^T - 1 (K 1 / n)^T + c) V lam^-1/2 with r = kappa(Z, X) 1 / n the row means
        and c the grand mean — ONE cross product with the block [V lam^-1/2, 1 / n], whose last
        column is r.  ``transform`` of the training points reproduces ``scores``."""
        Zs = self._points("KernelPCAModel.transform", Z)
        n, k = self.V.shape
        A = self.V / np.sqrt(self.lam)
        with Context(self.device) as ctx:
            ctx.set_matrix(self.K)
            Y = ctx.kernel_cross(Zs, np.column_stack([A, np.full(n, 1.0 / n)]))
        return pca_transform_algebra(Y[:, :k], Y[:, k], A, self.col_mean, self.grand_mean)


def pca_transform_algebra(KA, r, A, col_mean, grand_mean) -> np.ndarray:
    """(Kz - r 1^T - 1 m^T + c) A from KA = Kz A and the row means r = Kz 1 / n, with m the training
    column means and c the grand mean: KA - r (1^T A) - 1 (m^T A) + c (1^T A)."""
    a = A.sum(axis=0)
    return KA - np.outer(r, a) - (col_mean @ A)[None, :] + grand_mean * a[None, :]


def kernel_pca_fit(X, k: int, b: int, *, kind: str = "rbf", gamma: float = 1.0, coef0: float = 0.0,
                   degree: int = 3, max_blocks=None, omega=None, seed: int = 0, tol: float = FIT_TOL,
                   device: int = 0) -> KernelPCAModel:
    """Kernel PCA of the n points X as ``RBL_kernel_pca`` computes it, kept as a model whose
    ``transform(Z)`` places new points on the same axes.  ValueError if one of the k leading
    eigenvalues of H K H is not > 0 (an axis of zero variance has no coordinates).  tol: the
    residual the eigenpairs are iterated to (FIT_TOL, tighter than the drivers')."""
    K, shift = _centred_kernel("kernel_pca_fit", X, kind, gamma, coef0, degree)
    _check_kb("kernel_pca_fit", K.n, k, b)
    with Context(device) as ctx:
        ctx.set_matrix(K)
        P, S = kernel_centering_update(ctx)
        ctx.set_lowrank(P, S)
        lam, V, info = _run(ctx, k, b, max_blocks, omega, seed, tol)
    if not np.all(lam > 0.0):
        raise ValueError(f"kernel_pca_fit: eigenvalue {int(np.argmin(lam > 0.0))} of H K H is not > 0 (lower k)")
    return KernelPCAModel(K, shift, device, lam, V, P[:, 1].copy(), float(S[0, 0]), info)


def nystrom_algebra(KB, dz) -> np.ndarray:
    """D_z^-1/2 (kappa(Z, X) D^-1/2 V lam^-1) from KB, the product in brackets, and the new points'
    degrees dz = kappa(Z, X) 1."""
    if not np.all(dz > 0.0):
        raise ValueError("a new point has degree kappa(z, X) 1 <= 0")
    return KB / np.sqrt(dz)[:, None]


class SpectralEmbeddingModel(_KernelFit):
    """A fitted normalised spectral embedding (``spectral_embedding_fit``): deg = K 1, (lam, V) the k
    leading eigenpairs of D^-1/2 K D^-1/2, Y the rows of V at unit length."""

    def __init__(self, K, shift, device, deg, lam, V, info):
        super().__init__(K, shift, device)
        self.deg, self.lam, self.V, self.Y, self.info = deg, lam, V, row_normalize(V), info

    def transform(self, Z, normalize: bool = True) -> np.ndarray:
        """The Nystrom extension of the embedding to the m points Z:
        D_z^-1/2 kappa(Z, X) D^-1/2 V lam^-1 with d_z = kappa(Z, X) 1 — one cross product with the
        block [V lam^-1, deg^1/2] against the operator's scale deg^-1/2, whose last column is d_z.
        Rows at unit length unless normalize=False; a training point lands on its own row of V (Y)."""
        Zs = self._points("SpectralEmbeddingModel.transform", Z)
        k = self.V.shape[1]
        with Context(self.device) as ctx:
            ctx.set_matrix(self.K)
            Yc = ctx.kernel_cross(Zs, np.column_stack([self.V / self.lam, np.sqrt(self.deg)]))
        E = nystrom_algebra(Yc[:, :k], Yc[:, k])
        return row_normalize(E) if normalize else E


def spectral_embedding_fit(X, k: int, b: int, *, kind: str = "rbf", gamma: float = 1.0, coef0: float = 0.0,
                           degree: int = 3, max_blocks=None, omega=None, seed: int = 0, tol: float = FIT_TOL,
                           device: int = 0, neighbors=None, mode: str = "union", weight: str = "binary"):
    """The embedding of ``RBL_spectral_embedding`` kept as a model whose ``transform(Z)`` embeds new
    points by the Nystrom extension.  ValueError for a degree <= 0 or one of the k eigenvalues == 0.

    neighbors=m: the embedding on the m-nearest-neighbour graph (as ``RBL_spectral_embedding`` with
    neighbors=), kept as a ``rbl.knn.KnnSpectralEmbeddingModel`` whose ``transform(Z)`` takes the m
    neighbours of each new point among the training points and applies the Nystrom extension
    restricted to them."""
    if neighbors is not None:
        from .knn import KnnSpectralEmbeddingModel, knn_affinity
        K, shift, N, deg = knn_affinity("spectral_embedding_fit", X, neighbors, mode, weight, kind, gamma, device)
        _check_kb("spectral_embedding_fit", K.n, k, b)
        with Context(device) as ctx:
            ctx.set_matrix(N)
            lam, V, info = _run(ctx, k, b, max_blocks, omega, seed, tol)
        if np.any(lam == 0.0):
            raise ValueError("spectral_embedding_fit: a zero eigenvalue has no Nystrom extension (lower k)")
        return KnnSpectralEmbeddingModel(K, shift, device, int(neighbors), mode, weight, float(gamma), deg, lam, V,
                                         info)
    K, shift = _centred_kernel("spectral_embedding_fit", X, kind, gamma, coef0, degree)
    _check_kb("spectral_embedding_fit", K.n, k, b)
    with Context(device) as ctx:
        ctx.set_matrix(K)
        deg = ctx.apply(np.ones((K.n, 1), order="F"))[:, 0]
        if not np.all(deg > 0.0):
            raise ValueError("spectral_embedding_fit: a point has degree K 1 <= 0")
        K.scale = deg ** -0.5
        ctx.set_kernel_scale(K.scale)
        lam, V, info = _run(ctx, k, b, max_blocks, omega, seed, tol)
    if np.any(lam == 0.0):
        raise ValueError("spectral_embedding_fit: a zero eigenvalue has no Nystrom extension (lower k)")
    return SpectralEmbeddingModel(K, shift, device, deg, lam, V, info)


def _inverse(x):
    return 1.0 / x


class GPModel(_KernelFit):
    """A fitted Gaussian-process regression (``gp_fit``): alpha = (K + noise I)^-1 y (n x t), the
    spectrum bounds (lo, hi) and the Chebyshev coefficients of 1 / x on them that every solve uses —
    or, fitted with solver="cg", neither (both None): every solve is then batched CG with the fit's
    tol, max_iter and spectral preconditioner ``precond`` = (V, dv) or None."""

    def __init__(self, K, shift, device, y, alpha, bounds, coef, tol, vec, solver="chebyshev", precond=None,
                 max_iter=1000):
        super().__init__(K, shift, device)
        self.y, self.alpha, self.bounds, self.coef, self.tol, self._vec = y, alpha, bounds, coef, tol, vec
        # solver="cg": every solve is ``Context.solve`` (bounds and coef are None); precond: its (V, dv)
        self.solver, self.precond, self.max_iter = solver, precond, max_iter

    def _cg_solve(self, ctx, C):
        """(K + noise I)^-1 C by the fit's CG (the preconditioner already set on ctx)."""
        from .solve import solve_on
        S, info = solve_on(ctx, C, tol=self.tol, max_iter=self.max_iter)
        _cg_check("GPModel.predict", info, self.max_iter)
        return S

    @property
    def noise(self) -> float:
        return self.K.nugget

    def _prior_var(self, Zs):
        if self.K.kind != "poly":
            return np.ones(Zs.shape[0])
        return (self.K.gamma * (Zs * Zs).sum(axis=1) + self.K.coef0) ** self.K.degree

    def predict(self, Z, return_var: bool = False):
        """The predictive mean kappa(Z, X) alpha at the m points Z (m, or m x t for an n x t y), and
        with return_var the variance of the latent function there,
        kappa(z, z) - k_z^T (K + noise I)^-1 k_z  (add ``noise`` for that of an observation):
        C = kappa(X, Z) from the transposed cross product on identity columns (chunks of at most
        RBL_MAX_BLOCK points), S = (K + noise I)^-1 C by the series of the fit, var = kappa(z, z) -
        colsum(C o S).  The series is accurate to ``tol`` relative to 1 / lo, so a variance is
        accurate to about tol kappa(z, z) hi / lo; values below that can come out slightly negative
        and are returned clipped at 0.  A model fitted with solver="cg" solves S = (K + noise I)^-1 C
        by batched CG instead (the fit's tol, max_iter and preconditioner; chunks of 64 columns): each
        column then meets |c - (K + noise I) s| <= tol |c|, so a variance is accurate to about
        tol |c|^2 / noise."""
        Zs = self._points("GPModel.predict", Z)
        m = Zs.shape[0]
        with Context(self.device) as ctx:
            ctx.set_matrix(self.K)
            mean = ctx.kernel_cross(Zs, self.alpha)
            mean = mean[:, 0] if self._vec else mean
            if not return_var:
                return mean
            if self.solver == "cg":
                if self.precond is not None:
                    ctx.set_preconditioner(*self.precond)
            else:
                ctx.set_filter_series(self.bounds[0], self.bounds[1], self.coef)
            var = self._prior_var(Zs)
            for c0 in range(0, m, _lib.RBL_MAX_BLOCK):
                Zc = Zs[c0:c0 + _lib.RBL_MAX_BLOCK]
                C = ctx.kernel_cross(Zc, np.eye(Zc.shape[0]), trans=True)
                if self.solver == "cg":
                    var[c0:c0 + C.shape[1]] -= (C * self._cg_solve(ctx, C)).sum(axis=0)
                    continue
                for j0 in range(0, C.shape[1], _SOLVE_CHUNK):
                    Cj = C[:, j0:j0 + _SOLVE_CHUNK]
                    var[c0 + j0:c0 + j0 + Cj.shape[1]] -= (Cj * ctx.apply_filter(Cj)).sum(axis=0)
        return mean, np.maximum(var, 0.0)

    def log_marginal_likelihood(self, nvec: int = 64, seed: int = 0, use_precond: bool = False):
        """(estimate, stderr) of log p(y | X) = -1/2 y^T alpha - 1/2 log det(K + noise I) - n / 2
        log 2 pi, summed over the t columns of y.  The log det term is a Hutchinson estimate over
        nvec Gaussian probes (``rbl.logdet`` on the bounds of the fit); stderr is its standard error
        carried to the result (t / 2 times the estimator's) — the data-fit term is exact to the
        solver's tolerance.  A model fitted with solver="cg" has no bounds: its log det term is
        stochastic Lanczos quadrature on the CG coefficients of nvec Rademacher probes drawn on the
        host from ``seed`` (``rbl.logdet_lanczos``: runs to the fit's tol or min(n, max_iter, 4096)
        iterations, unpreconditioned), with the standard error over those probes.  use_precond=True on
        a model that holds a preconditioner (``gp_fit`` with precond_rank >= 1, either kind): the
        quadrature runs preconditioned (``logdet_lanczos(..., precond=)``) — fewer iterations per probe
        and a smaller standard error; on any other model it changes nothing."""
        from .funm import _trace_on
        n, t = self.y.shape
        with Context(self.device) as ctx:
            ctx.set_matrix(self.K)
            if self.solver == "cg":
                from .solve import MAX_COEF_ITER, logdet_lanczos_on
                ld, err = logdet_lanczos_on(ctx, nvec, 0.0, seed, max(self.tol, 1e-12),
                                            min(n, self.max_iter, MAX_COEF_ITER),
                                            self.precond if use_precond else None)
                fit = float(np.sum(self.y * self.alpha))
                return -0.5 * fit - 0.5 * t * ld - 0.5 * n * t * np.log(2.0 * np.pi), 0.5 * t * err
            ld, err = _trace_on(ctx, np.log, self.bounds[0], self.bounds[1], nvec, None, max(self.tol, 1e-12),
                                seed, None)
        fit = float(np.sum(self.y * self.alpha))
        return -0.5 * fit - 0.5 * t * ld - 0.5 * n * t * np.log(2.0 * np.pi), 0.5 * t * err


    def mll_gradient(self, nvec: int = 32, seed: int = 0, ard: bool = False, probes=None) -> "MLLGradient":
        """The gradient of log p(y | X) (summed over the t columns of y) with respect to log gamma, log
        noise and, with ard, the logarithms of per-coordinate length scales s_k at s = 1 (the kernel on
        the points x o s).  For any kernel parameter theta

            dL / d theta = sum_ij M_ij dK_ij / d theta,    M = 1/2 alpha alpha^T - t/2 (K + noise I)^-1,

        and with nvec probes z_c (E z z^T = I) and w_c = (K + noise I)^-1 z_c the inverse is replaced by
        the symmetric low-rank estimate (1 / 2 nv) sum_c (w_c z_c^T + z_c w_c^T), so M ~ A B^T with
        A = [alpha / 2, -t W / (4 nv), -t Z / (4 nv)], B = [alpha, Z, W]; ``kernel_gradients`` then needs
        one derivative product of width 1 (gamma) and one of width d + 1 (the scales), K never formed.
        Z: Rademacher probes drawn on the host from ``seed`` (``rbl.solve.rademacher``, as
        ``logdet_lanczos``), or ``probes`` (n x nv) in their place — probes = sqrt(n) I makes the trace
        term exact.  W comes from the fit's CG (tol, max_iter, preconditioner): only a model fitted with
        solver="cg" has one, any other raises ValueError.  dlog_noise = noise (1/2 |alpha|^2 - t / (2 nv)
        sum_c z_c . w_c).

        ``stderr`` holds the standard error over the probes of the trace part of each component, from
        per-probe contributions tau_c = w_c^T (dK / d theta) z_c: they come from further products
        Phi [Z, x_k o Z, x_k^2 o Z] with A = B = 1 (nv columns, and 2 d nv more with ard), not from the
        low-rank launch, which only yields their sum.  The data-fit part is exact to the solver's tol.

        The laplace kernel is not differentiable at coincident points: pairs whose Gram-form squared
        distance is rounding noise contribute up to about gamma sqrt(N_ij u) each to ``dlog_scales``
        (N_ij = |x_i|^2 + |x_j|^2, u = 2^-53).  The other components are well conditioned."""
        if self.solver != "cg":
            raise ValueError('GPModel.mll_gradient: only for a model fitted with solver="cg" (the probes are '
                             "solved by the fit's CG)")
        from .solve import rademacher
        n, t = self.y.shape
        if probes is None:
            if isinstance(nvec, bool) or not isinstance(nvec, (int, np.integer)) or nvec < 2:
                raise ValueError("GPModel.mll_gradient: nvec must be an integer >= 2")
            Z = rademacher(n, int(nvec), seed)
        else:
            Z = np.asarray(probes, dtype=np.float64)
            if Z.ndim != 2 or Z.shape[0] != n or Z.shape[1] < 2 or not np.all(np.isfinite(Z)):
                raise ValueError(f"GPModel.mll_gradient: probes must be a finite n x nv array, n = {n}, nv >= 2")
        nv = Z.shape[1]
        K = self.K
        with Context(self.device) as ctx:
            ctx.set_matrix(K)
            if self.precond is not None:
                ctx.set_preconditioner(*self.precond)
            W = self._cg_solve(ctx, Z)
            A = np.column_stack([0.5 * self.alpha, (-0.25 * t / nv) * W, (-0.25 * t / nv) * Z])
            B = np.column_stack([self.alpha, Z, W])
            g = kernel_gradients(ctx, A, B, ard=ard, X=K.X)
            tau_g, tau_s = _probe_contributions(ctx, K, Z, W, ard)
        zw = (Z * W).sum(axis=0)
        half = 0.5 * t / np.sqrt(nv)
        err = {"dlog_gamma": half * K.gamma * float(np.std(tau_g, ddof=1)),
               "dlog_noise": half * K.nugget * float(np.std(zw, ddof=1)),
               "dlog_scales": half * np.std(tau_s, axis=0, ddof=1) if ard else None}
        return MLLGradient(g.dlog_gamma, K.nugget * g.trace, g.dlog_scales, err)


class KernelGradient:
    """``kernel_gradients``: dlog_gamma = sum_ij (A B^T)_ij dK_ij / d log gamma, dlog_scales the same
    for the d per-coordinate log length scales (None without ard), trace = sum_i a_i . b_i, the
    coefficient of d / d noise."""

    def __init__(self, dlog_gamma, dlog_scales, trace):
        self.dlog_gamma, self.dlog_scales, self.trace = dlog_gamma, dlog_scales, trace


class MLLGradient:
    """``GPModel.mll_gradient``: dlog_gamma, dlog_noise, dlog_scales (length d, or None) and ``stderr``,
    a dict of the standard error of each by those names."""

    def __init__(self, dlog_gamma, dlog_noise, dlog_scales, stderr):
        self.dlog_gamma, self.dlog_noise, self.dlog_scales, self.stderr = dlog_gamma, dlog_noise, dlog_scales, stderr


def hadamard_max_rank(d: int) -> int:
    """The most columns of A and B one ``Context.kernel_hadamard`` launch takes for points in d
    dimensions: 4 ceil(d / 4) + 4 ceil(r / 4) <= 256."""
    return _lib.RBL_KERNOP_MAX_DIM - 4 * ((int(d) + 3) // 4)


def scale_gradient_sums(kind: str, X, U) -> np.ndarray:
    """The host half of the per-coordinate gradients: g_k from U = (Psi o A B^T) [X, 1] (n x (d + 1)),
    Psi the "dscale" weight and A B^T symmetric.  Radial kernels: d kappa / d log s_k = psi (x_ik -
    x_jk)^2, so g_k = 2 sum_i x_ik^2 U_id - 2 sum_i x_ik U_ik; poly: psi x_ik x_jk, g_k = sum_i x_ik U_ik."""
    X, U = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64)
    d = X.shape[1]
    if kind == "poly":
        return (X * U[:, :d]).sum(axis=0)
    return 2.0 * ((X * X) * U[:, d:d + 1]).sum(axis=0) - 2.0 * (X * U[:, :d]).sum(axis=0)


def kernel_gradients(ctx_or_K, A, B, *, ard: bool = False, X=None, device: int = 0) -> KernelGradient:
    """sum_ij (A B^T)_ij dK_ij / d theta for theta = log gamma and, with ard, theta = log s_k, the
    per-coordinate length scales of the kernel on the points x o s at s = 1 — the gradient of any
    objective whose derivative with respect to K is the low-rank matrix A B^T (n x r factors): the GP
    log marginal likelihood (``GPModel.mll_gradient``), kernel alignment, kernel-PCA objectives.
    A B^T MUST BE SYMMETRIC; this is not checked (the per-coordinate sums use it).

    ``ctx_or_K``: a KernelMatrix (a context is made on ``device``), or a Context holding one — then
    ``X``, the n x d points it was loaded with, is needed for ard.  K is never formed:
    dlog_gamma = gamma sum_i ((Phi_dgamma o A B^T) 1)_i from one derivative product of width 1, and
    with ard one of width d + 1, U = (Psi o A B^T) [X, 1], followed by ``scale_gradient_sums``.  An r
    beyond ``hadamard_max_rank(d)`` is split into column groups of A and B whose U's are added in
    group order.  trace = sum_i a_i . b_i."""
    if isinstance(ctx_or_K, KernelMatrix):
        with Context(device) as ctx:
            ctx.set_matrix(ctx_or_K)
            return kernel_gradients(ctx, A, B, ard=ard, X=ctx_or_K.X)
    ctx = ctx_or_K
    info = ctx.kernel_info()
    n, d = info["n"], info["d"]
    kind = {v: k for k, v in KINDS.items()}[info["kind"]]
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.ndim == 1:
        A = A.reshape(-1, 1)
    if B.ndim == 1:
        B = B.reshape(-1, 1)
    if A.ndim != 2 or A.shape != B.shape or A.shape[0] != n or A.shape[1] < 1:
        raise ValueError(f"kernel_gradients: A and B must be n x r arrays of one shape, n = {n}")
    rmax = hadamard_max_rank(d)
    if rmax < 1:
        raise ValueError(f"kernel_gradients: d = {d} leaves no room for a factor column (d <= 252)")
    if ard:
        if X is None:
            raise ValueError("kernel_gradients: ard on a Context needs X, the points it was loaded with")
        X = np.asarray(X, dtype=np.float64)
        if X.shape != (n, d):
            raise ValueError(f"kernel_gradients: X must be {n} x {d}")

    def product(Q, weight):
        U = None
        for c0 in range(0, A.shape[1], rmax):
            Ug = ctx.kernel_hadamard(A[:, c0:c0 + rmax], B[:, c0:c0 + rmax], Q, weight)
            U = Ug if U is None else U + Ug
        return U

    dlog_gamma = info["gamma"] * float(product(np.ones((n, 1)), "dgamma").sum())
    dlog_scales = None
    if ard:
        dlog_scales = scale_gradient_sums(kind, X, product(np.column_stack([X, np.ones(n)]), "dscale"))
    return KernelGradient(dlog_gamma, dlog_scales, float(np.sum(A * B)))


def _probe_contributions(ctx, K: KernelMatrix, Z, W, ard: bool):
    """Per probe c: tau_c = w_c^T (dK / d gamma) z_c (nv), and with ard tau_ck = w_c^T (dK / d log s_k)
    z_c (nv x d), from products Phi Q with A = B = 1 in column chunks of at most RBL_MAX_BLOCK."""
    n, nv = Z.shape
    one = np.ones((n, 1))

    def phi_times(Q, weight):
        return np.column_stack([ctx.kernel_hadamard(one, one, Q[:, c0:c0 + _lib.RBL_MAX_BLOCK], weight)
                                for c0 in range(0, Q.shape[1], _lib.RBL_MAX_BLOCK)])

    tau_g = (W * phi_times(Z, "dgamma")).sum(axis=0)
    if not ard:
        return tau_g, None
    X = K.X
    tau_s = np.empty((nv, K.d))
    P = phi_times(Z, "dscale")
    for k in range(K.d):
        xk = X[:, k:k + 1]
        if K.kind == "poly":
            tau_s[:, k] = (W * xk * phi_times(xk * Z, "dscale")).sum(axis=0)
            continue
        RS = phi_times(np.column_stack([xk * Z, xk * xk * Z]), "dscale")
        tau_s[:, k] = (W * (xk * xk * P - 2.0 * xk * RS[:, :nv] + RS[:, nv:])).sum(axis=0)
    return tau_g, tau_s


_SOLVE_CHUNK = 64   # columns per rbl_apply_filter call, as rbl.funm.APPLY_CHUNK


def _cg_check(what, info, max_iter):
    """A CG solve of K + noise I must converge: RBLError for a column that is not positive definite,
    a warning for one that reached max_iter."""
    if np.any(info.status == _lib.RBL_SOLVE_NOT_POSDEF):
        raise _lib.RBLError(_lib.RBL_ERR_NUMERIC, f"{what}: K + noise I is not positive definite in floating point")
    slow = np.flatnonzero(info.status == _lib.RBL_SOLVE_MAX_ITER)
    if slow.size:
        import warnings
        warnings.warn(f"{what}: {slow.size} column(s) reached max_iter = {max_iter} (largest residual "
                      f"{float(info.residual[slow].max()):.2e})", RuntimeWarning, stacklevel=3)


def gp_fit(X, y, *, kind: str = "rbf", gamma: float = 1.0, noise: float, coef0: float = 0.0, degree: int = 3,
           tol: float = 1e-10, bounds=None, device: int = 0, solver: str = "chebyshev", precond_rank: int = 0,
           max_iter: int = 1000, precond: str = "eig", pchol_rank=None) -> GPModel:
    """Gaussian-process regression on the n points X with targets y (n, or n x t for t outputs) and
    observation noise variance ``noise`` > 0: alpha = (K + noise I)^-1 y by ``apply_function`` with
    f = 1 / x, K never formed; ``predict`` and ``log_marginal_likelihood`` on the model.

    The solver is ``apply_function``'s Chebyshev series of 1 / x on [lo, hi] and has its limits: the
    degree grows like sqrt(hi / lo) log(1 / tol), so it suits K + noise I of moderate condition number
    (noise not many orders below the largest eigenvalue, at most n for the radial kernels); solver="cg"
    below is the Krylov alternative.  bounds=(lo, hi) must enclose the spectrum of K + noise I with lo > 0.
    None: for the positive semi-definite kernels (rbf, laplace, poly with coef0 >= 0) lo = 0.99
    noise; hi = 1.01 max((K + noise I) 1) for the two radial kernels (entries >= 0: a row sum bounds
    the spectrum), else the estimate of ``estimate_spectrum``.

    solver="cg": alpha comes from ``Context.solve`` (batched conjugate gradients to |r| <= tol |y|, at
    most max_iter iterations) and no spectrum bounds are computed or needed; ``predict(return_var=True)``
    solves its columns the same way and ``log_marginal_likelihood`` uses Lanczos quadrature on the CG
    coefficients (``rbl.logdet_lanczos``).  precond_rank=r (1..32, solver="cg" only): the r leading
    eigenpairs of K + noise I are computed first (``lanczos``, block size r) and deflated by
    ``spectral_preconditioner`` — the iteration count then follows the spectrum below them.
    precond="pchol" (needs solver="cg" and precond_rank >= 1) builds the pair without an eigensolve: a
    partial pivoted Cholesky factor of K of rank pchol_rank (default min(4 precond_rank, 256, n);
    ``Context.kernel_pchol``) compressed to its best precond_rank directions by
    ``pchol_preconditioner(L, noise, precond_rank)``; the model stores the pair as with "eig".  A status
    other than converged raises RBLError (not positive definite) or warns (max_iter reached)."""
    if solver not in ("chebyshev", "cg"):
        raise ValueError('gp_fit: solver must be "chebyshev" or "cg"')
    if isinstance(precond_rank, bool) or not isinstance(precond_rank, (int, np.integer)) or not 0 <= precond_rank <= 32:
        raise ValueError("gp_fit: precond_rank must be an integer in [0, 32]")
    if precond_rank and solver != "cg":
        raise ValueError('gp_fit: precond_rank needs solver="cg"')
    if precond not in ("eig", "pchol"):
        raise ValueError('gp_fit: precond must be "eig" or "pchol"')
    if precond == "pchol" and (solver != "cg" or precond_rank < 1):
        raise ValueError('gp_fit: precond="pchol" needs solver="cg" and precond_rank >= 1')
    if pchol_rank is not None:
        if precond != "pchol":
            raise ValueError('gp_fit: pchol_rank belongs to precond="pchol"')
        if isinstance(pchol_rank, bool) or not isinstance(pchol_rank, (int, np.integer)) or \
                not 1 <= pchol_rank <= _lib.RBL_PCHOL_MAX_RANK:
            raise ValueError(f"gp_fit: pchol_rank must be an integer in [1, {_lib.RBL_PCHOL_MAX_RANK}]")
    if isinstance(noise, bool) or not np.isscalar(noise) or not np.isfinite(noise) or not noise > 0:
        raise ValueError("gp_fit: noise must be a finite number > 0")
    if not np.isscalar(tol) or not 0 < tol < 1:
        raise ValueError("gp_fit: tol must be in (0, 1)")
    K, shift = _centred_kernel("gp_fit", X, kind, gamma, coef0, degree, nugget=noise)
    y = np.asarray(y, dtype=np.float64)
    vec = y.ndim == 1
    if vec:
        y = y[:, None]
    if y.ndim != 2 or y.shape[0] != K.n or y.shape[1] < 1:
        raise ValueError(f"gp_fit: y must have n = {K.n} rows")
    if not np.all(np.isfinite(y)):
        raise ValueError("gp_fit: y has a non-finite entry")
    if solver == "cg":
        if bounds is not None:
            raise ValueError('gp_fit: bounds belong to solver="chebyshev" (CG needs none)')
        if precond_rank > K.n:
            raise ValueError(f"gp_fit: precond_rank = {precond_rank} exceeds n = {K.n}")
        if pchol_rank is not None and pchol_rank > K.n:
            raise ValueError(f"gp_fit: pchol_rank = {pchol_rank} exceeds n = {K.n}")
        from .solve import solve_on, spectral_preconditioner
        pair = None
        with Context(device) as ctx:
            ctx.set_matrix(K)
            if precond_rank and precond == "pchol":
                from .pchol import pchol_preconditioner
                R = min(4 * int(precond_rank), _lib.RBL_PCHOL_MAX_RANK, K.n) if pchol_rank is None else int(pchol_rank)
                L = ctx.kernel_pchol(R)[0]
                if L.shape[1] < 1:
                    raise _lib.RBLError(_lib.RBL_ERR_NUMERIC, "gp_fit: the pivoted Cholesky factor of K has rank 0")
                V, dv = pchol_preconditioner(L, float(noise), int(precond_rank))
                pair = (np.asfortranarray(V), dv)
                ctx.set_preconditioner(*pair)
            elif precond_rank:
                lam, V, _ = _run(ctx, int(precond_rank), int(precond_rank), None, None, 0)
                V, dv = spectral_preconditioner(lam, V)
                pair = (np.asfortranarray(V), dv)
                ctx.set_preconditioner(*pair)
            alpha, info = solve_on(ctx, y, tol=tol, max_iter=max_iter)
        _cg_check("gp_fit", info, max_iter)
        return GPModel(K, shift, device, y, alpha, None, None, float(tol), vec, "cg", pair, int(max_iter))
    from .density import _bounds
    from .funm import apply_function, cheb_fit
    with Context(device) as ctx:
        ctx.set_matrix(K)
        if bounds is not None:
            (lo, hi), _ = _bounds(ctx, bounds, 0)
        else:
            if kind != "poly":
                lo, hi = 0.0, 1.01 * float(ctx.apply(np.ones((K.n, 1), order="F")).max())
            else:
                (lo, hi), _ = _bounds(ctx, None, 0)
            if kind != "poly" or coef0 >= 0:
                lo = 0.99 * float(noise)
        if not lo > 0:
            raise ValueError(f"gp_fit: the lower spectrum bound {lo} is not > 0 (pass bounds=(lo, hi))")
    coef = cheb_fit(_inverse, lo, hi, tol)       # the series apply_function fits; predict reuses it
    alpha = apply_function(K, _inverse, y, tol=tol, bounds=(lo, hi), device=device)
    return GPModel(K, shift, device, y, alpha, (lo, hi), coef, float(tol), vec)
