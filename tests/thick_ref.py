"""NumPy restatement of thick-restart block Lanczos (rbl.thick) — float64, dense linear algebra,
full reorthogonalisation — and the inputs of its tests.  It is the authority for the restart
counts written into tests/test_gpu_thick.py; nothing here imports the package.

After m block steps  A Q = Q T + Q_{m+1} B_{m+1} E_m^T.  With T = S Theta S^T, the p = kb b Ritz
pairs of largest |theta| and W = B_{m+1} S_p[last b rows, :]:

    Y = Q S_p,   A Y = Y Theta_p + Q_{m+1} W,

and the run continues from [Y, Q_{m+1}] with the projected matrix diag(Theta_p), bordered by W,
followed by the block tridiagonal tail.  The first step after a restart is
    U = A Q_{m+1} - Y W^T,  A_new = Q_{m+1}^T U,  U -= Q_{m+1} A_new,  Q_next B_next = qr(U).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


# ---- inputs ---------------------------------------------------------------------------------
def make(n: int, seed: int, kind: str = "lin"):
    """diag(linspace(0, 1, n)) + R + R^T, R with 6 entries of size +-0.02 per row (CSR)."""
    if kind != "lin":
        raise ValueError(kind)
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), 6)
    cols = rng.integers(0, n, size=6 * n)
    vals = 0.02 * rng.choice([-1.0, 1.0], size=6 * n)
    R = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A = sp.diags(np.linspace(0.0, 1.0, n)) + R + R.T
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def laplacian5(nx: int):
    """The five-point Laplacian on an nx x nx grid (CSR, n = nx^2)."""
    T = sp.diags([-np.ones(nx - 1), 2.0 * np.ones(nx), -np.ones(nx - 1)], [-1, 0, 1])
    I = sp.identity(nx)
    A = sp.csr_matrix(sp.kron(I, T) + sp.kron(T, I))
    A.sort_indices()
    return A


def start_block(n: int, b: int, seed: int) -> np.ndarray:
    """The start block the tests hand to both the restatement and the device driver."""
    return np.random.default_rng(seed).standard_normal((n, b))


# The end-to-end inputs: generator, k, b, max_blocks, keep_blocks, and the restarts thick_ref needs
# with the start block start_block(n, b, 0) (tests/test_thick_host.py asserts the counts; the GPU
# tests cap a run at twice the count).
CASES = {
    "lin3000_b4": dict(make=lambda: make(3000, 1), k=20, b=4, m=24, kb=10, restarts=13),
    "lin4000_b4": dict(make=lambda: make(4000, 2), k=100, b=4, m=60, kb=35, restarts=13),
    "lap45_b1": dict(make=lambda: laplacian5(45), k=12, b=1, m=40, kb=20, restarts=20),
    "lin3000_b16": dict(make=lambda: make(3000, 3), k=40, b=16, m=16, kb=7, restarts=9),
    "lin3000_b32": dict(make=lambda: make(3000, 3), k=40, b=32, m=10, kb=4, restarts=11),
}


def top_abs(ev, k):
    """The k eigenvalues of largest |lambda| from a full spectrum, descending |lambda|."""
    return ev[np.argsort(-np.abs(ev), kind="stable")[:k]]


# ---- pieces ---------------------------------------------------------------------------------
def gamma(N: int) -> float:
    """gamma_N = N u / (1 - N u), u = 2^-53: the dot-product bound for any summation order."""
    u = 2.0 ** -53
    return N * u / (1.0 - N * u)


def compress_ref(Q_blocks, S):
    """[Q_1 .. Q_m] S in numpy.longdouble, and |Q| |S| (float64) for the entry-wise bound."""
    Q = np.hstack([np.asarray(q) for q in Q_blocks])
    Y = Q.astype(np.longdouble) @ np.asarray(S).astype(np.longdouble)
    return Y, np.abs(Q) @ np.abs(np.asarray(S))


def sort_abs(lam, Z, count):
    """The `count` eigenpairs of largest |lambda|, ascending |lambda| (stable)."""
    perm = np.argsort(np.abs(lam), kind="stable")[len(lam) - count:]
    return lam[perm], Z[:, perm]


def assemble(theta, W, As, Bs, b):
    """diag(theta), the border W, then the block tridiagonal tail (A_t diagonal, B_t below)."""
    p, nt = len(theta), len(As)
    T = np.zeros((p + nt * b, p + nt * b))
    T[:p, :p] = np.diag(theta)
    for t in range(nt):
        o = p + t * b
        T[o:o + b, o:o + b] = As[t]
        if t == 0 and p:
            T[o:o + b, :p] = W
            T[:p, o:o + b] = W.T
        if t:
            T[o:o + b, o - b:o] = Bs[t - 1]
            T[o - b:o, o:o + b] = Bs[t - 1].T
    return T


def arrow_step(A, Y, Qr, W, drop_border: bool = False):
    """The first step after a restart on the basis [Y, Qr]: returns (A_new, Q_next, B_next).
    drop_border leaves out the Y W^T term (what a plain 3-term step would do)."""
    U = A @ Qr
    if not drop_border:
        U = U - Y @ W.T
    A_new = Qr.T @ U
    U = U - Qr @ A_new
    Q_next, B_next = np.linalg.qr(U)
    return A_new, Q_next, B_next


# ---- the driver -----------------------------------------------------------------------------
def thick_ref(A, k, b, max_blocks, keep_blocks, *, tol=1e-7, max_restarts=500, omega=None, seed=0,
              keep_state=False):
    """Returns (D, V, info): D the k Ritz values of largest |lambda| (descending |lambda|), V their
    Ritz vectors, info a dict with restarts, op_applies, converged and — with keep_state — the
    basis `basis` (n x (m b)), the assembled projected matrix `T` and the residual block of the
    last cycle."""
    n = A.shape[0]
    m, kb = max_blocks, keep_blocks
    if omega is None:
        omega = start_block(n, b, seed)
    Q1, _ = np.linalg.qr(A @ omega)
    V = np.zeros((n, (m + 1) * b))
    V[:, :b] = Q1
    theta, W = np.zeros(0), np.zeros((b, 0))
    head = 0
    info = {"restarts": 0, "op_applies": 1, "converged": False}
    while True:
        As, Bs = [], []
        for i in range(head, m):                       # block i -> block i + 1
            q = V[:, i * b:(i + 1) * b]
            U = A @ q
            info["op_applies"] += 1
            if i == head and head:
                U -= V[:, :head * b] @ W.T
            elif i > head:
                U -= V[:, (i - 1) * b:i * b] @ Bs[-1].T
            Ai = q.T @ U
            Ai = 0.5 * (Ai + Ai.T)
            U -= q @ Ai
            for _ in range(2):                         # full reorthogonalisation
                U -= V[:, :(i + 1) * b] @ (V[:, :(i + 1) * b].T @ U)
            Qn, Bn = np.linalg.qr(U)
            V[:, (i + 1) * b:(i + 2) * b] = Qn
            As.append(Ai)
            Bs.append(Bn)
        T = assemble(theta, W, As, Bs, b)
        lam, Z = np.linalg.eigh(T)
        D, S = sort_abs(lam, Z, k)
        res = np.linalg.norm(Bs[-1] @ S[-b:, :], axis=0)
        if np.all(res <= tol):
            info["converged"] = True
            break
        if info["restarts"] >= max_restarts:
            break
        theta, Sp = sort_abs(lam, Z, kb * b)
        W = Bs[-1] @ Sp[-b:, :]
        V[:, :kb * b] = V[:, :m * b] @ Sp
        V[:, kb * b:(kb + 1) * b] = V[:, m * b:(m + 1) * b]
        head = kb
        info["restarts"] += 1
    if keep_state:
        info["basis"] = V[:, :m * b].copy()
        info["T"] = T
        info["resid_block"] = V[:, m * b:(m + 1) * b].copy()
        info["B_last"] = Bs[-1]
    Vr = V[:, :m * b] @ S
    return D[::-1].copy(), Vr[:, ::-1].copy(), info
