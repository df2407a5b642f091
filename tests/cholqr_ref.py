"""Long-double references for the tall-skinny QR of a block step (tsqr in csrc/rbl_api.cpp:
CholQR2 on the Gram matrix, shifted CholQR3 when the block is nearly rank deficient) on blocks of
a chosen condition number (helper of test_cholqr_ref_host.py and test_gpu_tsqr_direct.py; NumPy
and SciPy only, no GPU, no library call).

  * bipartite — A = [[0, D], [D, 0]], D = diag(c) with c = 1 on the first max(1, b // 2) rows and
    eps on the rest, and Omega = [Omega1; 0].  Every product of the first block step then has a
    single term: A Omega = [0; c o Omega1], so Q_1 = [0; Y]; A Q_1 = [c o Y; 0]; A_1 = Q_1^T A Q_1
    is exactly zero (disjoint supports); and the step's QR input is U = [c o Y; 0], known from the
    fetched Q_1 up to one rounding per entry.  cond(U) = 1 / eps to three digits: eps is the dial.
  * step_omega — the Omega of the step-QR cases.  With the standard normal Omega1 the start
    block is genuinely graded, but the step's U has its condition number through a column
    scaling only, which Cholesky QR does not see; step_omega's docstring says why and what it
    does instead.
  * qr_ref — Householder QR in numpy.longdouble, R's diagonal non-negative.
  * cholqr_emulate — a plain float64 transcription of k_chol (csrc/smallmat.hip) and of tsqr's
    pass structure: the same shift formula, the same pivot rule, Rtot = R3 R2 R1.  It only shows
    that the bounds below are attainable and that a broken algorithm exceeds them (drop_pass3: the
    third pass skipped although the first one shifted; drop_shift: no pivot rule and no shift,
    i.e. plain CholQR2 whatever the block).
  * orth / resid / lower / cond — the checks, evaluated in long double, each returning the
    measured number.
  * the case tables and the bounds, as named constants with their origin.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
if not np.finfo(LD).eps <= 2.0 ** -63:
    raise AssertionError(f"numpy.longdouble has eps = {np.finfo(LD).eps}: the references of "
                         "tests/cholqr_ref.py need the x87 extended type (eps <= 2^-63)")

U = 2.0 ** -53            # float64 unit roundoff

# status words of rbl_step (include/rbl_hip.h), restated so that this file imports no library
RBL_OK = 0
RBL_WARN_QR_SHIFTED = 2

# -- bounds ------------------------------------------------------------------------------------
# max|Q^T Q - I| of the QR's output: twenty times the float64 emulation's worst over the case
# tables below (5e-15), six orders below its weakest negative control (2.4e-7 without pass 3)
ORTH_TOL = 1e-13
# max|Q B - U| / max|U|: ten times the emulation's worst over the case tables (1e-14)
RESID_TOL = 1e-13
# first-order QR perturbation bound |dQ|, |dR| / |R| <= cond(U) u, with a factor of 100
PERT_FACTOR = 100.0
# the sign / column-order comparison against qr_ref is made up to this condition number (above
# it PERT_FACTOR cond u passes 1e-8 and fixes nothing the other checks do not)
PERT_MAX_COND = 1e6
# from this condition number on the first pass must have shifted: the pivot rule d < 1e-15 g_jj
# fires once cond exceeds ~3e7; between 1e6 and 3e10 it depends on the block, not only on cond
SHIFT_MIN_COND = 3e10
# a negative control must miss ORTH_TOL by this factor (without pass 3 the emulation ends at
# 2e-4 at cond 1e11, n = 1040, b = 32: u cond(Q1)^2 with cond(Q1) ~ sqrt(shift) / sigma_min)
CONTROL_FACTOR = 100.0
# fp32 basis: Q + E, |E| <= 2^-24 |Q|, unit columns: |(Q + E)^T (Q + E) - I| <= 2 2^-24 + 2^-48
# + ORTH_TOL < 2^-22 by Cauchy-Schwarz
ORTH32_TOL = 2.0 ** -22
# exactly rank-deficient start block: |Rhat[j, j]| of the dependent column against max|U0| (the
# column's component outside the span of the others is rounding, ~1e-15; 1e-6 leaves the shifted
# passes' sqrt(shift) ~ 1e-3 far outside)
DEFICIENT_DIAG_TOL = 1e-6

# -- cases -------------------------------------------------------------------------------------
M = 520                   # n = 1040: neither a multiple of 128, halves meet inside a 16-row tile
SEED = 20261020
# b -> the path it selects in chol_step / tsqr
BS = {1: "k_chol<true>, unfused tsmm", 2: "k_chol<true>, unfused tsmm",
      5: "k_chol<true>, unfused tsmm", 8: "k_chol<true>, unfused tsmm",
      16: "k_chol_elim2, rowop fused form", 32: "k_chol_elim2, rowop fused form",
      64: "k_chol<true> at the LDS limit kMaxB",
      80: "k_chol<false>, L2 scratch, out-of-place apply through d_T"}
# eps -> the band cond(U_ref) must lie in
BANDS = {1.0: (1.0, 30.0), 1e-4: (3e3, 3e4), 1e-8: (3e7, 3e8), 1e-11: (3e10, 3e11),
         1e-13: (3e12, 3e13)}
# The start QR (the block c o Omega1 with a standard normal Omega1) runs at all 40 pairs.
START_CASES = tuple((b, e) for b in BS for e in BANDS)
# The step QR (Omega from step_omega): (b, eps of the band, eps used, m).
#  * The top band runs at eps = 3e-13 (cond 3.3e12, inside [3e12, 3e13]), not 1e-13.  After the
#    shifted first pass cond(Q1) ~ sqrt(shift) / sigma_min with shift = 11 (n b + b (b + 1)) u
#    tr(G); the second pass is a plain Cholesky QR of Q1 and needs u cond(Q1)^2 < 1.  At 1e-13
#    with n = 1040 the emulation's Q after two passes is off by O(1) already at b = 16, and from
#    b = 32 on its second pass meets a non-positive pivot, shifts again and ends at 8e-10
#    (b = 32) to 3e-8 (b = 80).  This is the range of shifted CholQR3, not a property of an
#    implementation.
#  * (32, top band) runs at m = 132 (n = 264, still no multiple of 128 or 16): at m = 520 the
#    emulation passes, but with Q off by 1.4 after two passes it sits on that edge, and which
#    side a run falls on depends on its rounding (0.03 at m = 132).
#  * Dropped, the reference itself misses ORTH_TOL (test_cholqr_ref_host.py shows it):
#    - b = 1 with eps < 1: a block of one column has cond 1 whatever its grading, so no eps
#      puts cond(U_ref) into the band;
#    - b = 64 and 80 in the top band: beyond that edge even at the band's lower end (the
#      emulation's second pass shifts again and ends at 2e-9 and 4e-9; fewer rows move the edge
#      too little: b = 80 still ends at 4e-10 at n = 324, and b = 64 at n = 264 passes with Q
#      off by 0.7 after two passes, on the edge again).
#    That is 6 pairs of 40, none at b = 16 or 32.  (A construction that reaches the shift at
#    all cannot do with fewer: see step_omega for why the standard normal Omega1 never does.)
TOP_EPS_USED = 3e-13
STEP_DROPPED = tuple((1, e) for e in BANDS if e < 1.0) + ((64, 1e-13), (80, 1e-13))
STEP_M = {(32, 1e-13): 132}
STEP_CASES = tuple((b, e, TOP_EPS_USED if e == 1e-13 else e, STEP_M.get((b, e), M))
                   for b in BS for e in BANDS if (b, e) not in STEP_DROPPED)
assert not any(b in (16, 32) for b, _ in STEP_DROPPED)
# The pass-3 / shift controls run at every step case of the two highest bands but b = 2: a block
# of two columns has one singular value below sqrt(shift), which the shifted pass turns into a
# column scaling — two passes already give 1e-15 there (shown in the host test).
CONTROL_CASES = tuple(c for c in STEP_CASES if BANDS[c[1]][0] >= SHIFT_MIN_COND and c[0] > 2)
CONTROL_EXEMPT = tuple(c for c in STEP_CASES if BANDS[c[1]][0] >= SHIFT_MIN_COND and c[0] == 2)

FUSED_CASES = tuple((b, e) for b in (16, 32) for e in (1e-4, 1e-11))      # (d) and (e)
FUSE_VALUES = (0, 1, 3, 7)
RANK_CASES = ((2, 32, 1e-11), (3, 32, 1e-11), (2, 8, 1e-4))               # (P, b, eps)
DEFICIENT_CASES = tuple((b, kind) for b in (8, 16, 32) for kind in ("duplicate", "zero"))


def case_id(b, eps):
    return f"b{b}-eps{eps:g}"


def bipartite(m, b, eps, seed=SEED):
    """A = [[0, D], [D, 0]] (scipy CSR, n = 2m), c = diag(D) and Omega = [Omega1; 0] (n x b)."""
    c = np.full(m, float(eps))
    c[:max(1, b // 2)] = 1.0
    D = sp.diags(c)
    A = sp.bmat([[None, D], [D, None]], format="csr")
    A.sort_indices()
    omega = np.zeros((2 * m, b))
    omega[:m] = np.random.default_rng(seed + b).standard_normal((m, b))
    return A, c, omega


def step_omega(m, b, eps, seed=SEED):
    """The Omega of the step-QR cases: Omega1 = (s / c) o G with G the standard normal block of
    `bipartite`, s_i = 16 eps^(i / h) on c's h = max(1, b // 2) unit rows and m^-1/2 on the rest.

    Why not the standard normal Omega1 itself: Q_1 = qr(c o Omega1).Q then has its first h
    columns on the unit rows and the others off them (up to O(eps)), so U = c o Y is an
    orthogonal block with its last columns scaled by eps.  cond(U) = 1 / eps, but only through a
    column scaling, which a Cholesky factorisation does not see: the pivot ratio d / g_jj stays
    O(1), and the emulation takes the unshifted two-pass path at every eps and meets every bound
    without a third pass (test_cholqr_ref_host.py::test_column_scaling_does_not_reach_the_shift).

    With this Omega1 the start block s o G is mildly graded (cond < 200: its m - h bulk rows add
    ~I to its Gram), Y is a generic orthonormal block, and U^T U = (1 - eps^2) Yt^T Yt + eps^2 I
    with Yt the h unit rows of Y, whose singular values follow s: U has singular values spread
    geometrically from ~1 down to eps^((h-1)/h), and b - h equal to eps, in directions that no
    column scaling removes.  cond(U) = 1 / eps within the bands, the pivot rule fires from ~3e7
    on, and — because several singular values lie spread out below sqrt(shift) — the block after
    the shifted first pass is itself ill-conditioned, so the third pass is needed."""
    _, c, omega = bipartite(m, b, eps, seed)
    h = max(1, b // 2)
    s = np.full(m, 1.0 / np.sqrt(m))
    s[:h] = 16.0 * float(eps) ** (np.arange(h) / h)
    omega[:m] *= (s / c)[:, None]
    return omega


def start_block(c, omega):
    """U0 = A Omega = [0; c o Omega1]: one term per entry, so exact up to its single rounding."""
    m = c.shape[0]
    U0 = np.zeros(omega.shape, dtype=LD)
    U0[m:] = c.astype(LD)[:, None] * omega[:m].astype(LD)
    return U0


def step_block(c, Q1):
    """U_ref = c o Y in long double (m x b), Y the lower half of the fetched Q_1: the non-zero
    rows of the step's QR input U = A Q_1 - Q_1 A_1 = [c o Y; 0]."""
    m = c.shape[0]
    return c.astype(LD)[:, None] * np.asarray(Q1[m:], dtype=LD)


def deficient_omega(omega, kind):
    """Omega with column b // 2 a duplicate of column 1, or zero."""
    b = omega.shape[1]
    om = omega.copy()
    om[:, b // 2] = om[:, 1] if kind == "duplicate" else 0.0
    return om


def qr_ref(X):
    """Householder QR in long double: X = Q R, Q (rows x b) with orthonormal columns, R upper
    triangular with a non-negative diagonal."""
    R = np.array(X, dtype=LD)
    n, b = R.shape
    V = []
    for j in range(b):
        x = R[j:, j].copy()
        nx = np.sqrt(x @ x)
        if nx == 0:
            V.append(None)
            continue
        x[0] += nx if x[0] >= 0 else -nx
        v = x / np.sqrt(x @ x)
        R[j:, j:] -= 2 * np.outer(v, v @ R[j:, j:])
        V.append(v)
    Q = np.zeros((n, b), dtype=LD)
    Q[:b, :b] = np.eye(b, dtype=LD)
    for j in range(b - 1, -1, -1):
        if V[j] is not None:
            Q[j:, :] -= 2 * np.outer(V[j], V[j] @ Q[j:, :])
    R = np.triu(R[:b])
    s = np.where(np.diag(R) < 0, LD(-1), LD(1))
    return Q * s[None, :], R * s[:, None]


def _chol(G, nglob, mode, drop_shift=False):
    """k_chol: R with G (+ shift I) = R^T R, R^-1 by back substitution, and the flags
    (zero, bad, shifted).  mode 0: the first pass (pivot rule active).  An exactly zero column of
    the block (g_jj = 0) takes the pivot 1 and R(j, j) = 0, as in the kernels: it neither fails
    nor makes the pass shift the other columns."""
    b = G.shape[0]
    tr = 0.0
    for j in range(b):
        tr += G[j, j]
    zero = not tr > 0.0
    shift = 0.0 if zero else 11.0 * (float(nglob) * b + float(b) * (b + 1)) * U * tr
    fail, shifted = 0, 0
    M = np.zeros((b, b))
    if not zero:
        for attempt in range(1 if drop_shift else 2):
            sh = shift if attempt else 0.0
            M = np.triu(G).astype(np.float64)
            M[np.arange(b), np.arange(b)] += sh
            fail = 0
            for j in range(b):
                d = 1.0 if G[j, j] == 0.0 else M[j, j]     # an exactly zero column: pivot 1
                if not d > 0.0 or not np.isfinite(d):
                    fail = 1
                    break
                if attempt == 0 and mode == 0 and not drop_shift and d < 1e-15 * (G[j, j] + sh):
                    fail = 2
                    break
                M[j, j] = np.sqrt(d)
                M[j, j + 1:] /= M[j, j]
                M[j + 1:, j + 1:] -= np.triu(np.outer(M[j, j + 1:], M[j, j + 1:]))
            if not fail:
                break
            shifted = 1
        if drop_shift:
            shifted = 0
    bad = (not zero) and fail != 0
    R = np.zeros((b, b))
    X = np.zeros((b, b))
    if not zero and not bad:
        R = np.triu(M)
        for c in range(b):
            X[c, c] = 1.0 / R[c, c]
            for i in range(c - 1, -1, -1):
                X[i, c] = -(R[i, i + 1:c + 1] @ X[i + 1:c + 1, c]) / R[i, i]
        R[np.diag(G) == 0.0, np.diag(G) == 0.0] = 0.0      # ... and R(j, j) = 0
    return R, X, zero, bad, shifted


def cholqr_emulate(X, n_global, drop_shift=False, drop_pass3=False):
    """tsqr in float64: Gram, k_chol, apply; a second pass; a third after a shifted first pass.
    Returns Q, Rtot = R3 R2 R1 and a dict with `shifted` (passes that shifted), `breakdown`,
    `passes` and `status` (the word rbl_step would return; breakdown is an error there)."""
    Q = np.asarray(X, dtype=np.float64)
    info = dict(shifted=0, breakdown=False, passes=0)
    Rtot = None
    need3 = False
    for p in range(3):
        if p == 2 and (not need3 or drop_pass3):
            break
        G = Q.T @ Q
        R, Rinv, zero, bad, shifted = _chol(G, n_global, 0 if p == 0 else 1, drop_shift)
        if p == 0:
            need3 = bool(shifted)
        info["shifted"] += shifted
        info["breakdown"] |= bool(bad)
        info["passes"] += 1
        Q = Q @ Rinv
        Rtot = R if Rtot is None else R @ Rtot
    info["status"] = RBL_WARN_QR_SHIFTED if info["shifted"] else RBL_OK
    return Q, Rtot, info


def _mm(A, B):
    return np.ascontiguousarray(A, dtype=LD) @ np.ascontiguousarray(B, dtype=LD)


def orth(Q, cols=None):
    """max|Q^T Q - I| (over the columns `cols` only, if given)."""
    Q = np.asarray(Q, dtype=LD)
    if cols is not None:
        Q = Q[:, cols]
    return float(np.abs(_mm(Q.T, Q) - np.eye(Q.shape[1], dtype=LD)).max())


def resid(Q, B, X):
    """max|Q B - X| / max|X|."""
    X = np.asarray(X, dtype=LD)
    return float(np.abs(_mm(Q, B) - X).max() / np.abs(X).max())


def lower(B):
    """The strictly lower triangle of B."""
    return np.tril(np.asarray(B), -1)


def singular_values(X):
    """Singular values of X in long double, descending: one-sided Jacobi on the R of qr_ref."""
    W = qr_ref(X)[1].copy()
    b = W.shape[0]
    eps = np.finfo(LD).eps
    for _ in range(60):
        rotated = False
        for p in range(b - 1):
            for q in range(p + 1, b):
                a, d, g = W[:, p] @ W[:, p], W[:, q] @ W[:, q], W[:, p] @ W[:, q]
                if g == 0 or abs(g) <= 4 * eps * np.sqrt(a * d):
                    continue
                rotated = True
                zeta = (d - a) / (2 * g)
                t = (1 if zeta >= 0 else -1) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                cs = 1 / np.sqrt(1 + t * t)
                sn = cs * t
                wp = W[:, p].copy()
                W[:, p] = cs * wp - sn * W[:, q]
                W[:, q] = sn * wp + cs * W[:, q]
        if not rotated:
            break
    else:
        raise AssertionError("singular_values: Jacobi did not converge")
    return np.sort(np.sqrt(np.einsum("ij,ij->j", W, W)))[::-1]


def cond(X):
    """The 2-norm condition number of X."""
    s = singular_values(X)
    return float(s[0] / s[-1])


def rhat(Q1, U0):
    """Rhat = Q_1^T U0 in long double."""
    return _mm(np.asarray(Q1, dtype=LD).T, U0)


def check_start(Q1, c, omega, tag="", skip_col=None):
    """The assertions on Q_1 = qr(A Omega).Q (a of the GPU test); returns (orth, resid).  With
    skip_col (the dependent column of a rank-deficient start block) the orthonormality is asked
    of the other columns only, the residual is not asserted, and Rhat's diagonal entry there must
    be below DEFICIENT_DIAG_TOL max|U0|."""
    m, b = c.shape[0], Q1.shape[1]
    U0 = start_block(c, omega)
    assert Q1.shape == U0.shape
    assert not Q1[:m].any(), f"{tag}: the first m rows of Q_1 are not exactly zero"
    assert np.isfinite(Q1).all(), tag
    Rh = rhat(Q1, U0)
    umax = float(np.abs(U0).max())
    r = float(np.abs(_mm(Q1, Rh) - U0).max()) / umax
    if skip_col is None:
        cols = np.arange(b)
    else:
        cols = np.array([j for j in range(b) if j != skip_col])
    o = orth(Q1, cols)
    assert o <= ORTH_TOL, (tag, o)
    if skip_col is None:
        assert r <= RESID_TOL, (tag, r)
        colnorm = np.sqrt(np.einsum("ij,ij->j", U0, U0))
        low = np.abs(lower(Rh)).max(axis=0)
        assert np.all(low <= ORTH_TOL * colnorm), (tag, float((low / colnorm).max()))
        assert np.all(np.diag(Rh) > 0), tag
    else:
        d = abs(float(Rh[skip_col, skip_col]))
        assert d <= DEFICIENT_DIAG_TOL * umax, (tag, d)
    return o, r


def check_step(Q1, A1, B2, Q2, status, c, eps, tag=""):
    """The assertions on the first block step's QR (b of the GPU test); returns the measured
    (cond(U_ref), orth(Q_2), resid)."""
    m, b = c.shape[0], Q1.shape[1]
    assert not np.asarray(A1).any(), f"{tag}: A_1 is not exactly zero"
    assert not lower(B2).any(), f"{tag}: B_2 is not exactly upper triangular"
    assert np.all(np.diag(B2) > 0), tag
    Uref = step_block(c, Q1)
    k = cond(Uref)
    lo, hi = BANDS[eps]
    assert lo <= k <= hi, (tag, k)
    assert not Q2[m:].any(), f"{tag}: the zero rows of U are not zero in Q_2"
    o = orth(Q2)
    r = resid(Q2[:m], B2, Uref)
    assert o <= ORTH_TOL, (tag, o)
    assert r <= RESID_TOL, (tag, r)
    if k <= PERT_MAX_COND:
        assert status == RBL_OK, (tag, status)
        Qr, Rr = qr_ref(Uref)
        tol = PERT_FACTOR * k * U
        dq = float(np.abs(np.asarray(Q2[:m], dtype=LD) - Qr).max())
        dr = float(np.sqrt(((np.asarray(B2, dtype=LD) - Rr) ** 2).sum()) / np.sqrt((Rr ** 2).sum()))
        assert dq <= tol, (tag, dq, tol)
        assert dr <= tol, (tag, dr, tol)
    if k >= SHIFT_MIN_COND:
        assert status == RBL_WARN_QR_SHIFTED, (tag, status)
    return k, o, r


def emulate_run(b, eps, omega, m=M, **broken):
    """The start QR and the first step's QR by the emulation (the mutation `broken` applies to
    the step's QR only): dict with c, omega, Q1, A1, B2, Q2, status, info (step), info0 (start)."""
    _, c, _ = bipartite(m, b, eps)
    om = omega
    n = 2 * m
    Q1, _, info0 = cholqr_emulate(np.asarray(start_block(c, om), dtype=np.float64), n)
    Ustep = np.zeros((n, b))
    Ustep[:m] = c[:, None] * Q1[m:]
    Q2, B2, info = cholqr_emulate(Ustep, n, **broken)
    return dict(c=c, omega=om, Q1=Q1, A1=np.zeros((b, b)), B2=B2, Q2=Q2, status=info["status"],
                info=info, info0=info0)
