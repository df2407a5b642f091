"""k-means on the device and spectral clustering that returns labels.

``kmeans(X, n_clusters)`` is Lloyd's iteration with k-means++ seeding, both in librbl_hip.so
(csrc/kmeans.hip; ``Context.kmeans_set_points`` / ``kmeans_seed`` / ``kmeans_run``): the host draws the
uniforms of the seeding and keeps the best of ``n_init`` starts, everything of size n stays on the GPU.
``RBL_spectral_clustering`` is ``RBL_spectral_embedding`` followed by ``kmeans`` on the row-normalised
embedding; ``spectral_clustering_fit`` keeps the fit as a model whose ``predict(Z)`` labels new points.

The device takes squared distances in Gram form, max((|x|^2 + |c|^2) - 2 x.c, 0): points far from the
origin lose digits to the cancellation, so centre such data first (the rows of a normalised spectral
embedding have unit length: nothing to do).  A point goes to the centre with the smallest
(distance, index), and a centre that loses all its points keeps its value — visible in ``counts``.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np

from . import _lib
from .kernelop import RBL_spectral_embedding, spectral_embedding_fit
from .rbl_gpu import Context


@dataclass
class KMeansResult:
    """labels (n, int32), centers (c x d), inertia = sum_i d2(i, labels_i) and counts (c, int64) of one
    consistent state of the iteration; n_iter its index t; converged 1 (no label changed), 2 (the
    centres moved by at most tol in squared Frobenius norm) or 0 (max_iter reached)."""
    labels: np.ndarray
    centers: np.ndarray
    inertia: float
    counts: np.ndarray
    n_iter: int
    converged: int

    @property
    def n_empty(self) -> int:
        return int((self.counts == 0).sum())


def _points(what, X):
    """X as an n x d fp64 array (a vector is n x 1), finite, n >= 1, 1 <= d <= RBL_KERNOP_MAX_DIM."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(-1, 1)
    if X.ndim != 2 or X.shape[0] < 1 or not 1 <= X.shape[1] <= _lib.RBL_KERNOP_MAX_DIM:
        raise ValueError(f"{what}: X must be an n x d array with n >= 1 and 1 <= d <= {_lib.RBL_KERNOP_MAX_DIM}")
    if not np.all(np.isfinite(X)):
        raise ValueError(f"{what}: X has a non-finite entry")
    return X


def _check_clusters(what, c, n):
    if isinstance(c, bool) or not isinstance(c, (int, np.integer)):
        raise ValueError(f"{what}: n_clusters must be an integer")
    if not 1 <= c <= _lib.RBL_KMEANS_MAX_CLUSTERS:
        raise ValueError(f"{what}: n_clusters must be in [1, {_lib.RBL_KMEANS_MAX_CLUSTERS}]")
    if c > n:
        raise ValueError(f"{what}: n_clusters = {c} exceeds n = {n}")
    return int(c)


def seeding_uniforms(seed, n_clusters: int, n_init: int) -> np.ndarray:
    """The uniforms of ``kmeans``'s starts, n_init x n_clusters: row s seeds start s.  One generator,
    ``np.random.default_rng(seed)``, drawn start after start."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(n_clusters) for _ in range(n_init)])


def select_best(results):
    """The index of the result with the lowest inertia; the first wins a tie."""
    best = 0
    for s, r in enumerate(results):
        if r.inertia < results[best].inertia:
            best = s
    return best


def _warn_empty(what, res):
    if res.n_empty:
        warnings.warn(f"{what}: {res.n_empty} of {res.counts.size} clusters are empty (their centres kept "
                      "their last value)", RuntimeWarning, stacklevel=3)


def kmeans(X, n_clusters: int, *, init="k-means++", n_init: int = 1, max_iter: int = 300, tol: float = 0.0,
           seed=0, device: int = 0) -> KMeansResult:
    """k-means of the n points X (n x d) into n_clusters clusters on the device.

    init="k-means++": every start is seeded by plain k-means++ on the device from n_clusters uniforms of
    ``np.random.default_rng(seed)`` (``seeding_uniforms``); the best of the n_init starts (the lowest
    inertia, the first on a tie) is returned.  init=ndarray (n_clusters x d): one start from these
    centres.  max_iter and tol: see ``Context.kmeans_run`` (tol = 0: run until no label changes).  The
    points are uploaded once for all starts.  RuntimeWarning naming the number of empty clusters if the
    result has any."""
    X = _points("kmeans", X)
    n = X.shape[0]
    c = _check_clusters("kmeans", n_clusters, n)
    if isinstance(n_init, bool) or not isinstance(n_init, (int, np.integer)) or n_init < 1:
        raise ValueError("kmeans: n_init must be an integer >= 1")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 0:
        raise ValueError("kmeans: max_iter must be an integer >= 0")
    if not np.isfinite(tol) or tol < 0.0:
        raise ValueError("kmeans: tol must be finite and >= 0")
    given = None
    if isinstance(init, str):
        if init != "k-means++":
            raise ValueError("kmeans: init must be 'k-means++' or an n_clusters x d array")
        U = seeding_uniforms(seed, c, int(n_init))
    else:
        given = np.asarray(init, dtype=np.float64)
        if given.ndim == 1 and X.shape[1] == 1:
            given = given.reshape(-1, 1)
        if given.shape != (c, X.shape[1]):
            raise ValueError(f"kmeans: init must be 'k-means++' or an n_clusters x d = {c} x {X.shape[1]} array")
        if not np.all(np.isfinite(given)):
            raise ValueError("kmeans: init has a non-finite entry")
    with Context(device) as ctx:
        ctx.kmeans_set_points(X)
        if given is not None:
            results = [ctx.kmeans_run(given, max_iter, tol)]
        else:
            results = [ctx.kmeans_run(X[ctx.kmeans_seed(c, u)], max_iter, tol) for u in U]
    res = results[select_best(results)]
    _warn_empty("kmeans", res)
    return res


def kmeans_predict(Y, centers, device: int = 0) -> np.ndarray:
    """The label of every row of Y against fixed centres: one assign-only run (max_iter = 0) on the device."""
    with Context(device) as ctx:
        ctx.kmeans_set_points(Y)
        return ctx.kmeans_run(centers, 0).labels


def RBL_spectral_clustering(X, n_clusters: int, b: int, *, n_init: int = 10, seed=0, return_info: bool = False,
                            **embedding_kw):
    """Spectral clustering of the n points X: ``RBL_spectral_embedding(X, k=n_clusters, b, ...)`` and
    ``kmeans`` (k-means++, n_init starts) on the row-normalised embedding.  embedding_kw goes to the
    embedding as it stands (gamma=, kind=, neighbors=, mode=, weight=, max_blocks=, device=, ...); seed
    seeds both the embedding's start block and the k-means uniforms.  Returns the labels (n, int32); with
    return_info (labels, Y, lam, KMeansResult)."""
    if "return_info" in embedding_kw or "k" in embedding_kw:
        raise ValueError("RBL_spectral_clustering: k is n_clusters, and return_info is this function's own")
    lam, _, Y = RBL_spectral_embedding(X, n_clusters, b, seed=seed, **embedding_kw)
    res = kmeans(Y, n_clusters, n_init=n_init, seed=seed, device=embedding_kw.get("device", 0))
    return (res.labels, Y, lam, res) if return_info else res.labels


class SpectralClusteringModel:
    """A fitted spectral clustering (``spectral_clustering_fit``): ``embedding_model`` the fitted
    embedding, ``embedding`` its row-normalised training rows, ``labels`` / ``centers`` the k-means
    result on them (``kmeans_result`` in full)."""

    def __init__(self, embedding_model, kmeans_result: KMeansResult, device: int = 0):
        self.embedding_model, self.kmeans_result, self.device = embedding_model, kmeans_result, device
        self.embedding = embedding_model.Y
        self.labels, self.centers = kmeans_result.labels, kmeans_result.centers

    def predict(self, Z) -> np.ndarray:
        """Labels of the m new points Z: their normalised out-of-sample embedding
        (``embedding_model.transform(Z)``) assigned to the stored centres."""
        return kmeans_predict(self.embedding_model.transform(Z), self.centers, self.device)


def spectral_clustering_fit(X, n_clusters: int, b: int, *, n_init: int = 10, seed=0,
                            **embedding_kw) -> SpectralClusteringModel:
    """``RBL_spectral_clustering`` kept as a model: ``spectral_embedding_fit(X, n_clusters, b, ...)`` and
    ``kmeans`` on its row-normalised embedding; ``predict(Z)`` labels new points."""
    if "k" in embedding_kw:
        raise ValueError("spectral_clustering_fit: k is n_clusters")
    device = embedding_kw.get("device", 0)
    model = spectral_embedding_fit(X, n_clusters, b, seed=seed, **embedding_kw)
    res = kmeans(model.Y, n_clusters, n_init=n_init, seed=seed, device=device)
    return SpectralClusteringModel(model, res, device)
