"""CPU: the host side of the rank-one shifted SVD and PCA (rbl/pca.py, rbl/svd.py) — argument
validation before any device call, the O(nnz) column statistics against dense NumPy, and the new
entry points in every layer that names them (ctypes table, library, header, Context, Julia).
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rbl_set_rect_shift", "rbl_get_rect_shift", "rbl_apply_rect_shifted")


@pytest.fixture(scope="module")
def rbl():
    import rbl as _r
    return _r


@pytest.fixture()
def no_context(rbl, monkeypatch):
    """Any attempt to open a context fails the test: validation must come first."""
    def boom(*a, **k):
        raise AssertionError("a context was created before the arguments were validated")
    monkeypatch.setattr(rbl.Context, "__init__", boom)
    import rbl.svd
    monkeypatch.setattr(rbl.svd, "Context", rbl.Context)


def small(m=40, n=30):
    rng = np.random.default_rng(2)
    B = sp.random(m, n, 0.2, format="csr", random_state=rng)
    B = B.tolil()
    B[:, 4] = 0.0                                    # an empty column
    B[:, 9] = rng.uniform(1.0, 2.0, (m, 1))          # a full column
    B = B.tocsr()
    B.eliminate_zeros()
    return B


def test_svd_shift_validation(rbl, no_context):
    B = small()
    m, n = B.shape
    u, v = np.ones(m), np.ones(n)
    for bad in ((u,), (u, v, v), (v, u), (u[:-1], v), (u, v[:-1]), (u.reshape(m, 1), v), 3.0,
                (np.where(np.arange(m) == 2, np.nan, u), v), (u, np.where(np.arange(n) == 0, np.inf, v))):
        with pytest.raises(ValueError):
            rbl.RBL_svd(B, 3, 4, shift=bad)
    with pytest.raises(ValueError):
        rbl.RBL_svd(B, 0, 4, shift=(u, v))
    with pytest.raises(ValueError):
        rbl.RBL_svd(B, 3, 4, side="up", shift=(u, v))


def test_pca_validation(rbl, no_context):
    B = small()
    for kw in (dict(k=0), dict(k=31), dict(k=2.0), dict(b=0), dict(b=True), dict(side="top"),
               dict(ddof=2), dict(ddof=-1), dict(ddof=0.5)):
        args = dict(k=3, b=4)
        args.update(kw)
        k, b = args.pop("k"), args.pop("b")
        with pytest.raises(ValueError):
            rbl.RBL_pca(B, k, b, **args)
    with pytest.raises(ValueError):
        rbl.RBL_pca(B.toarray(), 3, 4)
    with pytest.raises(ValueError):
        rbl.RBL_pca(B[:1], 1, 1, ddof=1)             # m > ddof


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("fmt", ["csr", "csc", "coo"])
def test_column_stats_match_dense(rbl, ddof, fmt):
    B = small().asformat(fmt)
    Bd = B.toarray() + 1000.0 * (np.arange(B.shape[1]) == 9)     # a mean that dominates its spread
    B = sp.csr_matrix(Bd).asformat(fmt)
    mean, var, sumsq = rbl.column_stats(B, ddof)
    assert not Bd[:, 4].any() and Bd[:, 9].all()
    assert mean[4] == 0.0 and var[4] == 0.0
    ref_mean, ref_var = Bd.mean(axis=0), Bd.var(axis=0, ddof=ddof)
    assert np.abs(mean - ref_mean).max() <= 1e-14 * np.abs(ref_mean).max()
    assert np.all(np.abs(var - ref_var) <= 1e-14 * np.maximum(ref_var, ref_var.max() * 1e-3))
    assert np.abs(sumsq - (Bd ** 2).sum(axis=0)).max() <= 1e-14 * (Bd ** 2).sum(axis=0).max()


def test_names_in_every_layer(rbl):
    from rbl import _lib
    hdr = open(os.path.join(ROOT, "include", "rbl_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.lib, name)
        assert re.search(rf"^int {name}\(", hdr, re.M), name
    for meth in ("set_rect_shift", "get_rect_shift", "apply_rect_shifted"):
        assert callable(getattr(rbl.Context, meth))
    assert callable(rbl.RBL_pca)
    assert re.search(r"^#define RBL_ABI_VERSION 2$", hdr, re.M)
    assert _lib.lib.rbl_abi_version() == 2


def test_julia_source_has_pca():
    src = open(os.path.join(ROOT, "julia", "RBL_hip.jl")).read()
    assert re.search(r"^function RBL_gpu_pca\(B::SparseMatrixCSC\{DOUBLE\},\s*k::Int64,\s*b::Int64\)",
                     src, re.M)
    assert ":rbl_set_rect_shift" in src
    assert re.search(r"^function set_rect_shift!\(", src, re.M)
    assert re.search(r"shift\s*=\s*nothing", src)
