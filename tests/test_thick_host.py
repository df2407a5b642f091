"""CPU: thick-restart block Lanczos without a GPU — the NumPy restatement (tests/thick_ref.py)
against dense eigh on the inputs of the GPU tests, with the restart counts those tests rely on;
the projected-matrix assembly against V^T A V; the property the arrow-step test pins; argument
validation of the drivers; the binding's new names."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import thick_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rbl_hip.h")
JL = os.path.join(ROOT, "julia", "RBL_hip.jl")


@pytest.mark.parametrize("name", list(tr.CASES))
def test_restatement_matches_dense_eigh(name):
    """Every input converges to the dense eigenvalues within the project's parity bound
    1e-10 max|lambda| (measured: <= 6e-14), in exactly the restarts written in thick_ref.CASES —
    each of these bases is far too small for an unrestarted run."""
    c = tr.CASES[name]
    A = c["make"]()
    D, V, info = tr.thick_ref(A, c["k"], c["b"], c["m"], c["kb"])
    ev = np.linalg.eigvalsh(A.toarray())
    top = tr.top_abs(ev, c["k"])
    assert info["converged"]
    assert info["restarts"] == c["restarts"]
    scale = np.abs(ev).max()
    assert np.max(np.abs(np.sort(D) - np.sort(top))) <= 1e-10 * scale
    R = A @ V - V * D
    assert np.linalg.norm(R, axis=0).max() <= 1e-6 * scale
    assert np.abs(V.T @ V - np.eye(c["k"])).max() <= 1e-12


@pytest.mark.parametrize("b,m,kb", [(4, 12, 5), (1, 16, 7), (16, 6, 3)])
def test_projected_matrix_assembly(b, m, kb):
    """diag(Theta_p) + the W border + the block tridiagonal tail is V^T A V of the restatement's own
    basis, within 1e-12 ||A||, after several restarts; rbl.thick.projected_matrix assembles the same
    matrix from the same pieces."""
    A = tr.make(600, 7)
    k = (kb - 1) * b
    D, V, info = tr.thick_ref(A, k, b, m, kb, max_restarts=3, keep_state=True)
    assert info["restarts"] == 3
    Vb, T = info["basis"], info["T"]
    norm_a = abs(A).sum(axis=0).max()
    assert np.abs(Vb.T @ Vb - np.eye(m * b)).max() <= 1e-12
    assert np.abs(Vb.T @ (A @ Vb) - T).max() <= 1e-12 * norm_a
    # the Krylov relation with the residual block: A V = V T + Q_{m+1} B_{m+1} E_m^T
    E = np.zeros((m * b, b))
    E[-b:] = np.eye(b)
    rel = A @ Vb - Vb @ T - info["resid_block"] @ info["B_last"] @ E.T
    assert np.abs(rel).max() <= 1e-12 * norm_a

    from rbl.thick import projected_matrix
    p = kb * b
    theta = np.diag(T)[:p]
    W = T[p:p + b, :p]
    As = [T[p + t * b:p + (t + 1) * b, p + t * b:p + (t + 1) * b] for t in range(m - kb)]
    Bs = [T[p + (t + 1) * b:p + (t + 2) * b, p + t * b:p + (t + 1) * b] for t in range(m - kb - 1)]
    assert np.array_equal(projected_matrix(theta, W, As, Bs + [info["B_last"]], b), T)


@pytest.mark.parametrize("b", [4, 32])
def test_arrow_step_needs_the_border_term(b):
    """The property tests/test_gpu_thick.py pins on the device: after a restart the next block is
    orthogonal to the kept Ritz block Y to ~1e-14 when U = A Q_{m+1} - Y W^T, and off by >= 1e-3
    when the Y W^T term is left out (n = 1237, the GPU test's shapes)."""
    n, m, kb = 1237, (12, 6)[b == 32], (5, 2)[b == 32]
    A = tr.make(n, 11)
    _, _, info = tr.thick_ref(A, b, b, m, kb, max_restarts=0, keep_state=True)
    lam, Z = np.linalg.eigh(info["T"])
    theta, Sp = tr.sort_abs(lam, Z, kb * b)
    W = info["B_last"] @ Sp[-b:, :]
    Y, Qr = info["basis"] @ Sp, info["resid_block"]
    _, Qn, _ = tr.arrow_step(A, Y, Qr, W)
    assert np.abs(Y.T @ Qn).max() <= 1e-13
    _, Qbad, _ = tr.arrow_step(A, Y, Qr, W, drop_border=True)
    assert np.abs(Y.T @ Qbad).max() >= 1e-3


def test_compress_ref_and_gamma():
    rng = np.random.default_rng(0)
    Q = [rng.standard_normal((9, 2)) for _ in range(3)]
    S = rng.standard_normal((6, 4))
    Y, absb = tr.compress_ref(Q, S)
    assert Y.dtype == np.longdouble and Y.shape == (9, 4)
    assert np.abs(np.asarray(Y, dtype=np.float64) - np.hstack(Q) @ S).max() <= 2 * tr.gamma(6) * absb.max()
    assert tr.gamma(1) == pytest.approx(2.0 ** -53, rel=1e-12)


def test_thick_argument_validation():
    """Bad arguments raise ValueError before a context is created (no GPU here)."""
    import rbl
    from rbl.thick import check_keep_blocks, default_keep_blocks
    A = sp.identity(200, format="csr")
    for bad in (np.zeros(5), sp.random(30, 20, 0.2, format="csr"), None, [[1.0]]):
        with pytest.raises(ValueError):
            rbl.RBL_thick(bad, 2, 1, max_blocks=10)
    for k in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            rbl.RBL_thick(A, k, 2, max_blocks=10)
    for b in (0, -3, 1.5):
        with pytest.raises(ValueError):
            rbl.RBL_thick(A, 4, b, max_blocks=10)
    for mb in (0, 2.0, None):
        with pytest.raises((ValueError, TypeError)):
            rbl.RBL_thick(A, 4, 2, max_blocks=mb)
    # max_blocks too small for k: the message says how large it must be (kb >= 3, m >= 5)
    with pytest.raises(ValueError, match=r"max_blocks must be at least 5"):
        rbl.RBL_thick(A, 4, 2, max_blocks=4)
    with pytest.raises(ValueError, match=r"keep_blocks \* b must be at least k \+ b = 6"):
        rbl.RBL_thick(A, 4, 2, max_blocks=10, keep_blocks=2)
    with pytest.raises(ValueError, match=r"needs max_blocks >= 11"):
        rbl.RBL_thick(A, 4, 2, max_blocks=10, keep_blocks=9)
    with pytest.raises(ValueError, match="RBL_COMPRESS_MAX_COLS"):
        rbl.RBL_thick(sp.identity(40000, format="csr"), 4, 32, max_blocks=40, keep_blocks=17)
    with pytest.raises(ValueError, match="RBL_COMPRESS_MAX_COLS"):
        rbl.RBL_thick(sp.identity(40000, format="csr"), 600, 32, max_blocks=40)
    with pytest.raises(ValueError, match="must be below n"):
        rbl.RBL_thick(A, 4, 2, max_blocks=100)
    # the default: half the basis, at least ceil((k + b) / b), at most max_blocks - 2 and 512 columns
    assert default_keep_blocks(20, 4, 24) == 12
    assert default_keep_blocks(100, 4, 60) == 30
    assert default_keep_blocks(100, 4, 28) == 26
    assert default_keep_blocks(40, 32, 40) == 16
    for k, b, m in ((20, 4, 24), (100, 4, 28), (12, 1, 40), (40, 32, 10)):
        kb = default_keep_blocks(k, b, m)
        assert kb * b >= k + b and kb <= m - 2
    assert check_keep_blocks(20, 4, 24, 10) == 10


def test_lanczos_thick_validates_before_the_device(monkeypatch):
    """lanczos_thick checks its arguments before it touches the context."""
    from rbl.thick import lanczos_thick

    class Boom:
        nranks = 1

        def __getattr__(self, name):
            raise AssertionError(f"context touched: {name}")

    for kw in (dict(max_blocks=4), dict(max_blocks=10, keep_blocks=2), dict(max_blocks=10, max_restarts=-1),
               dict(max_blocks=10, tol=0.0), dict(max_blocks=10, keep_blocks=3.5)):
        with pytest.raises(ValueError):
            lanczos_thick(Boom(), 4, 2, **kw)


def test_svd_max_blocks_validation():
    import rbl
    B = sp.random(300, 200, 0.05, format="csr", random_state=1)
    with pytest.raises(ValueError, match="max_blocks must be at least"):
        rbl.RBL_svd(B, 8, 2, max_blocks=5)
    with pytest.raises(ValueError, match="need max_blocks"):
        rbl.RBL_svd(B, 8, 2, keep_blocks=5)
    with pytest.raises(ValueError, match="need max_blocks"):
        rbl.RBL_svd(B, 8, 2, max_restarts=5)
    with pytest.raises(ValueError, match="keep_blocks"):
        rbl.RBL_svd(B, 8, 2, max_blocks=12, keep_blocks=4)
    with pytest.raises(ValueError, match="iterated dimension"):
        rbl.RBL_svd(B, 8, 2, max_blocks=100)


def test_new_names_in_binding_header_and_julia():
    from rbl import _lib
    import rbl
    hdr = open(HEADER).read()
    for name in ("rbl_thick_restart", "rbl_bench_compress_pass"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name), name
        assert re.search(rf"^int {name}\(", hdr, re.M), name
    m = re.search(r"^#define\s+RBL_COMPRESS_MAX_COLS\s+(\d+)\b", hdr, re.M)
    assert m and int(m.group(1)) == _lib.RBL_COMPRESS_MAX_COLS >= 512
    assert re.search(r"^#define\s+RBL_ABI_VERSION\s+2\b", hdr, re.M)
    for name in ("thick_restart", "bench_compress_pass"):
        assert callable(getattr(rbl.Context, name))
    assert callable(rbl.RBL_thick) and callable(rbl.lanczos_thick)
    info = rbl.RBLInfo()
    assert (info.restarts, info.op_applies, info.peak_blocks) == (0, 0, 0)
    src = open(JL).read()
    assert re.search(r"^function RBL_gpu_thick\(", src, re.M)
    assert ":rbl_thick_restart" in src
