"""Long-double references for the partial reorthogonalisation, the locked-vector projection and
the Ritz projection (helper of test_reorth_ref_host.py, test_gpu_reorth_direct.py and
test_gpu_small_blocks.py; no GPU, no library call).

  * cgs_ref / mgs_ref — [Q_m, Q_{m-1}] against Q_1..Q_{m-2}: one block-CGS projection with every
    coefficient from the unmodified pair (the library's default), and the reference's ascending-j
    block MGS (RBL.jl:30-48, oracle.part_reorth(..., "mgs"), RBL_OPT_REORTH_ORDER = 1);
  * lock_ref — one projection per locked vector, in lock order (restarted.jl:1-21);
  * ritz_ref — V = sum_j Q_j S_j (RBL.jl:61-71);
  * cgs_bound / ritz_bound — the entry-by-entry forward bounds the GPU tests assert, and
    seq_tol, the measured tolerance of the orderings that have no simple forward bound;
  * lost_orth_blocks — the oracle's block loop WITHOUT partial reorth.  On a matrix whose top
    eigenvalues converge within a few steps the basis loses orthogonality to O(1), so a partial
    reorth of its last two blocks has O(1e-3 .. 1) coefficients to remove: a kernel that drops a
    basis panel or a row then misses the reference by many orders of magnitude, where on a healthy
    basis (W^T X ~ 1e-15) it would be invisible;
  * CASES / LOCK_CASES / RANK_CASES — the case table shared by the host and the GPU tests.

Every reference is evaluated in numpy.longdouble (x87 extended, 64-bit significand), with every
dtype accepted so that the same code gives the float64 restatement the measured tolerances need.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import matgen
from oracle import rbl_oracle as o

LD = np.longdouble
if not np.finfo(LD).eps <= 2.0 ** -63:
    raise AssertionError(f"numpy.longdouble has eps = {np.finfo(LD).eps}: the references of "
                         "tests/reorth_ref.py need the x87 extended type (eps <= 2^-63)")

U = 2.0 ** -53
MIN_COEFF = 1e-3      # max|W^T X| every case must reach (a condition on the inputs)
MIN_MARGIN = 100.0    # a dropped panel / row must move some entry by this many bounds

_POOL = ThreadPoolExecutor(max_workers=8)


def _mm(A, B):
    """A @ B.  NumPy has no BLAS for long double; its loop releases the GIL, so the columns of B
    are spread over a few threads (each entry is still one plain left-to-right dot product)."""
    if A.dtype != LD or B.ndim != 2 or B.shape[1] < 2 or A.size * B.shape[1] < 1 << 20:
        return A @ B
    A = np.ascontiguousarray(A)
    parts = np.array_split(np.arange(B.shape[1]), min(8, B.shape[1]))
    cols = list(_POOL.map(lambda c: A @ np.ascontiguousarray(B[:, c]), parts))
    return np.hstack(cols)


def _stack(blocks, dtype):
    return np.hstack([np.asarray(q, dtype=dtype) for q in blocks])


def cgs_ref(W_blocks, X, dtype=LD):
    """X - W (W^T X), every coefficient from the unmodified X.  X = [Q_m, Q_{m-1}],
    W = [Q_1..Q_{m-2}] (a list of n x b blocks)."""
    W = _stack(W_blocks, dtype)
    X = np.asarray(X, dtype=dtype)
    return X - _mm(W, _mm(np.ascontiguousarray(W.T), X))


def _seq_project(panels, X, dtype, dot_rows=None):
    """X -= P (P^T X) panel after panel, each from the current X; dot_rows limits the rows the
    coefficients' dot products run over (the drop-last-row mutation), the update is full height."""
    X = np.array(X, dtype=dtype)
    r = slice(None) if dot_rows is None else slice(0, dot_rows)
    for P in panels:
        P = np.asarray(P, dtype=dtype)
        X = X - _mm(P, _mm(np.ascontiguousarray(P[r].T), X[r]))
    return X


def mgs_ref(W_blocks, X, dtype=LD):
    """The ascending-j block MGS: X -= Q_j (Q_j^T X) for j = 1..m-2, each from the current X."""
    return _seq_project(W_blocks, X, dtype)


def lock_ref(L, Xp, dtype=LD):
    """Xp -= l (l^T Xp) for every column l of L, in lock order (lock_reorth of the library)."""
    return _seq_project([L[:, j:j + 1] for j in range(L.shape[1])], Xp, dtype)


def ritz_ref(blocks, S, dtype=LD):
    """sum_j Q_j S_j with S_j the j-th b rows of S."""
    b = blocks[0].shape[1]
    S = np.asarray(S, dtype=dtype)
    V = np.zeros((blocks[0].shape[0], S.shape[1]), dtype=dtype)
    for j, Q in enumerate(blocks):
        V = V + _mm(np.asarray(Q, dtype=dtype), S[j * b:(j + 1) * b])
    return V


def cgs_bound(W_blocks, X, n=None):
    """|got - ref| <= 2 (n + K + 4) u (|W| (|W|^T |X|)) + 4 u |X|, entry by entry: each
    coefficient a length-n dot product in any summation order (n + 2: split partials, MFMA
    chains, the all-reduce), each output entry a length-K dot product and one subtraction
    (K + 2); the factor 2 covers the second-order terms.  n is the global row count."""
    W = np.abs(_stack(W_blocks, np.float64))
    X = np.abs(np.asarray(X, dtype=np.float64))
    n = W.shape[0] if n is None else n
    return 2.0 * (n + W.shape[1] + 4) * U * (W @ (W.T @ X)) + 4.0 * U * X


def ritz_bound(blocks, S):
    """|V - ref| <= 2 (K + 2) u |Q| |S|, entry by entry (K = number of basis columns)."""
    Q = np.abs(_stack(blocks, np.float64))
    return 2.0 * (Q.shape[1] + 2) * U * (Q @ np.abs(np.asarray(S, dtype=np.float64)))


def seq_tol(ref, ref64, X):
    """Tolerance of an ordering whose steps depend on each other (MGS, the locked vectors):
    16 max(err_np, u max|X|) with err_np the max-norm error of the float64 NumPy restatement
    `ref64` of the same ordering against the long-double `ref` on the same inputs.  Returns
    (tolerance, err_np)."""
    err_np = float(np.abs(np.asarray(ref64, dtype=LD) - ref).max())
    return 16.0 * max(err_np, U * float(np.abs(X).max())), err_np


def coeff_max(W_blocks, X):
    """max|W^T X| — how much the projection has to remove."""
    return float(np.abs(_stack(W_blocks, np.float64).T @ np.asarray(X, dtype=np.float64)).max())


def cgs_drop_margins(W_blocks, X, bound):
    """By how many bounds the CGS reference moves when one basis panel, or the last row of the
    coefficients' dot products, is left out: a list with max_e |move_e| / bound_e per dropped
    panel, and the same figure for the last row.  Without panel j the reference gains
    Q_j (Q_j^T X); without the last row r the coefficients lose W[r]^T X[r].  (float64: the
    moves are many orders above its rounding.)"""
    X = np.asarray(X, dtype=np.float64)
    panels = [float((np.abs(Wj @ (Wj.T @ X)) / bound).max()) for Wj in W_blocks]
    W = _stack(W_blocks, np.float64)
    row = float((np.abs(W @ np.outer(W[-1], X[-1])) / bound).max())
    return panels, row


def seq_drop_margins(panels, X, tol):
    """The same for an ordering with a scalar tolerance (the MGS blocks, or the locked vectors as
    1-column panels): max|without panel j - all| / tol per panel, and with the last row left out
    of every coefficient's dot product."""
    full = _seq_project(panels, X, np.float64)
    out = [float(np.abs(_seq_project(panels[:j] + panels[j + 1:], X, np.float64) - full).max()) / tol
           for j in range(len(panels))]
    cut = _seq_project(panels, X, np.float64, dot_rows=np.shape(X)[0] - 1)
    return out, float(np.abs(cut - full).max()) / tol


def assert_sensitive(records):
    """The conditions that keep a direct test from passing vacuously, on the records
    (nblocks, max|W^T X|, per-panel drop margins, last-row drop margin) of one case's calls:

      * every call has max|W^T X| >= MIN_COEFF and a last-row margin above MIN_MARGIN;
      * every basis panel Q_j that any call projects against has a margin above MIN_MARGIN in at
        least one call of the case;
      * from the second call on, so does the last panel Q_{nblocks-2} of that very call (the
        remainder of the kernels' panel groups).

    Not every panel of every call can: a block Lanczos basis stays semi-orthogonal between
    neighbouring blocks whatever else it has lost, so on the first call the two to four panels
    next to the pair carry coefficients at rounding level, at any run length (measured: margins
    0.04, 3, 380, 3e4, ... going back from the pair).  The later calls see those same panels from
    further away, and the pair of the call before, now changed by O(1e-2), as their last panels."""
    best = {}
    for k, (nb, c, panels, row) in enumerate(records):
        assert c >= MIN_COEFF, (nb, c)
        assert row > MIN_MARGIN, (nb, row)
        assert len(panels) == nb - 2
        for j, p in enumerate(panels):
            best[j] = max(best.get(j, 0.0), p)
        if k > 0:
            assert panels[-1] > MIN_MARGIN, (nb, panels[-1])
    low = {j + 1: f"{p:.1e}" for j, p in best.items() if not p > MIN_MARGIN}
    assert not low, f"panels never above {MIN_MARGIN} bounds in any call: {low}"


def describe(records):
    return " ".join(f"[nb={nb} max|W^T X|={c:.1e} panels {min(p):.1e}..{max(p):.1e} row {r:.1e}]"
                    for nb, c, p, r in records)


def case_matrix(n, W):
    """The direct tests' matrix: four planted eigenvalues (400, 300, 200, 100) far above a
    hash-window bulk, so their Ritz values converge within a few block steps."""
    return matgen.hashwindow_csr(n, W, 0.5, 20261015, matgen.planted_spectrum(2, 100.0))


def case_omega(n, b):
    return np.random.default_rng(b).standard_normal((n, b))


def lost_orth_blocks(A, b, m, omega, qr_mode="posdiag"):
    """Q_1..Q_m of the oracle's block loop (lanczos_iteration, RBL.jl:74-117) with the partial
    reorth left out: block steps 1..m-1 of local reorth, three-term update and QR only — what
    rbl_step(i, 0) runs.  As after rbl_step(m - 1, 0), Q_m is the last QR's output as it stands
    (its local reorth belongs to step m)."""
    Q = [o._qr(A @ np.asarray(omega, dtype=np.float64), qr_mode)[0]]
    Bi = None
    for i in range(1, m):
        if i >= 2:
            o.loc_reorth(Q[i - 1], Q[i - 2])
        V = A @ Q[i - 1]
        if i >= 2:
            V -= Q[i - 2] @ Bi.T
        Ai = Q[i - 1].T @ V
        V -= Q[i - 1] @ Ai
        Qn, Bi = o._qr(V, qr_mode)
        Q.append(Qn)
    return Q


def _case(what, n, W, b, m, at, order):
    return dict(what=what, n=n, W=W, b=b, m=m, at=tuple(at), order=order,
                id=f"{what}-n{n}-b{b}-m{m}-{'mgs' if order else 'cgs'}")


# (what, n, halfwidth W, b, m, the nblocks values rbl_reorth_last runs at, RBL_OPT_REORTH_ORDER)
CASES = (
    # k_gram44 / k_tsmm44f: every remainder of the 4-panel groups (nW = 7 .. 14)
    [_case("fast", n, 48, b, 16, range(9, 17), 0) for n in (1021, 3001) for b in (16, 32)]
    # fewer rows than a 128-row tile / few tiles
    + [_case("fastshort", 259, 16, 16, 12, range(9, 13), 0),
       _case("fastshort", 515, 16, 32, 12, range(9, 13), 0)]
    # the generic k_gram<AT,CT> / k_tsmm<RT,CT>, both orders
    # (b = 1 runs two steps longer: at m = 14 its max|W^T X| is 2e-5 at nblocks = 11)
    + [_case("generic", 1021, 48, b, 16 if b == 1 else 14, range(13, 17) if b == 1 else range(11, 15), order)
       for b in (1, 2, 4, 5, 8) for order in (0, 1)]
    # a deep run of narrow panels
    + [_case("deep", 1021, 48, 1, 60, (59, 60), 0), _case("deep", 1021, 48, 2, 60, (59, 60), 0),
       _case("deep", 1021, 48, 4, 40, (39, 40), 0)]
    # fewer rows than one wave's row group
    # ((131, 8) runs one step shorter: after the calls at 12 and 13 its max|W^T X| at 14 is 8e-4)
    + [_case("fewrows", n, 8, b, m, range(m - 2, m + 1), 0)
       for n, b, m in ((67, 1, 14), (67, 4, 14), (131, 2, 14), (131, 8, 13))]
    # wide panels (more than one accumulator group)
    + [_case("wide", 1021, 48, b, 12, range(10, 13), 0) for b in (64, 80)]
    # the reference's order on the fast path
    + [_case("fastmgs", 1021, 48, b, 12, (10, 12), 1) for b in (16, 32)]
)
# locked vectors (flags 2 and 3): (n, W, b, m), 3 locked vectors
LOCK_CASES = ((1021, 48, 8, 14), (1021, 48, 32, 12))
# several in-process ranks: (P, n, W, b, m, nblocks values)
RANK_CASES = ((3, 131, 8, 8, 13, (11, 12, 13)), (2, 1021, 48, 32, 12, (10, 11, 12)))


def lock_coeffs(m, b, nvec=3):
    """The S of rbl_lock: nvec random columns scaled by 1 / sqrt(m b)."""
    return np.asfortranarray(np.random.default_rng(100 + b).standard_normal((m * b, nvec))
                             / np.sqrt(m * b))


def pair(blocks, nb):
    """X = [Q_nb, Q_{nb-1}] and W = [Q_1..Q_{nb-2}] of a block list."""
    return list(blocks[:nb - 2]), np.hstack([blocks[nb - 1], blocks[nb - 2]])
