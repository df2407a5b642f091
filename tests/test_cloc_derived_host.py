"""CPU: the numerics of RBL_OPT_CLOC_DERIVE in NumPy.

A block Lanczos with the reference's schedule (partial reorth of the pair (Q_i, Q_{i-1}) against
Q_1..Q_{i-2} at the even steps, block CGS; then the local reorth Q_i -= Q_{i-1} (Q_{i-1}^T Q_i);
3-term update; CholQR2) on the bench's kind of matrix: hash-window band, half-width 16, the
planted spectrum 100 (2k + 1 - l); n = 6,000, b = 8, 30 steps, fp64.

The local-reorth coefficient of every step is formed three ways:
  direct   Q_{i-1}^T Q_i in fp64 (what a Gram pass gives);
  derived  from the step before: M R1^-1 R2^-1 with M = Q_{i-1}^T U' of its 3-term pass and the
           two CholQR factors; at an even step with a partial reorth then G - Cm^T Ci with G that
           value and [Ci | Cm] = W^T [Q_i | Q_{i-1}] the reorth's own coefficients
           (Cm^T (W^T W - I) Ci dropped);
  reference  Q_{i-1}^T Q_i of the same fp64 blocks in np.longdouble.
Condition on every step: max |derived - reference| <= 8 max |direct - reference| + 8 eps.  The
floor is there because both errors are a few eps.  The run continues with the derived coefficient,
as the library does with the option on; the gate of k_cloc_gate (E <= 4: a step whose U' is
graded keeps the direct Gram) is applied as there.

Measured: worst ratio of the derived error to the bound 0.10 over the 29 coefficients, the two
routes within 1.9 eps of each other; E = 6.1, 6.7 and 93.1 at the QRs of steps 1 to 3 (gated:
without the gate step 4's derived coefficient is 52 eps off, twice the bound), 1.1 .. 2.4 after.
"""
import numpy as np
import scipy.linalg as sla

from oracle import matgen

EPS = np.finfo(np.float64).eps
TAU = 4.0  # kClocGateTau (rbl_api.cpp)


def _cholqr2(U):
    R1 = np.linalg.cholesky(U.T @ U).T
    Q1 = sla.solve_triangular(R1, U.T, trans="T", lower=False).T
    R2 = np.linalg.cholesky(Q1.T @ Q1).T
    Q = sla.solve_triangular(R2, Q1.T, trans="T", lower=False).T
    return Q, R1, R2


def _gate(R1):
    """E = max_c sum_j |u_j| |R1^-1[j][c]| (k_cloc_gate)."""
    Rinv = sla.solve_triangular(R1, np.eye(R1.shape[0]), lower=False)
    return float((np.linalg.norm(R1, axis=0) @ np.abs(Rinv)).max())


def _ld(X):
    return X.astype(np.longdouble)


def test_derived_coefficient_tracks_the_direct_gram():
    n, b, steps, k = 6000, 8, 30, 10
    A = matgen.hashwindow_csr(n, 16, 0.7734, 20261015, matgen.planted_spectrum(k)).tocsr()
    omega = np.random.default_rng(1).standard_normal((n, b))
    Q = [_cholqr2(A @ omega)[0]]
    Bprev = None
    G = None            # derived Q_{i-1}^T Q_i, formed by step i - 1
    worst = 0.0         # max over steps of derived error / (8 direct error + 8 eps)
    routes = {"3term": 0, "reorth": 0, "gated": 0}
    sizes, diffs, emax = [], [], 0.0
    for i in range(1, steps + 1):
        Qi = Q[i - 1]
        Qm = Q[i - 2] if i >= 2 else None
        derived = G
        if i >= 4 and i % 2 == 0:                       # partial reorth, block CGS
            W = np.hstack(Q[: i - 2])
            Ci, Cm = W.T @ Qi, W.T @ Qm
            Qi -= W @ Ci
            Qm -= W @ Cm
            if derived is not None:
                derived = derived - Cm.T @ Ci
                routes["reorth"] += 1
            sizes.append((float(np.abs(Ci).max()), float(np.abs(Cm).max())))
        elif derived is not None:
            routes["3term"] += 1
        if i >= 2:
            direct = Qm.T @ Qi
            ref = np.asarray(_ld(Qm).T @ _ld(Qi))
            e_der = float(np.abs(_ld(derived) - ref).max())
            e_dir = float(np.abs(_ld(direct) - ref).max())
            worst = max(worst, e_der / (8 * e_dir + 8 * EPS))
            diffs.append(float(np.abs(derived - direct).max()) / EPS)
            assert e_der <= 8 * e_dir + 8 * EPS, (i, e_der, e_dir)
            Qi -= Qm @ derived
        U = A @ Qi
        if i >= 2:
            U -= Qm @ Bprev.T
        U -= Qi @ (Qi.T @ U)
        M = Qi.T @ U
        Qn, R1, R2 = _cholqr2(U)
        E = _gate(R1)
        emax = max(emax, E)
        if E <= TAU:
            G = sla.solve_triangular(R2, sla.solve_triangular(R1, M.T, trans="T", lower=False),
                                     trans="T", lower=False).T
        else:                                            # the gate refuses: the QR's cross Gram
            G = Qi.T @ Qn
            routes["gated"] += 1
        Bprev = R2 @ R1
        Q.append(Qn)
    print(f"derived error / (8 direct error + 8 eps): worst ratio {worst:.3f}; "
          f"|derived - direct| <= {max(diffs):.1f} eps; routes {routes}; largest gate value E = "
          f"{emax:.1f}; |Ci| <= {max(s[0] for s in sizes):.1e}, |Cm| <= {max(s[1] for s in sizes):.1e}")
    assert worst <= 1.0
    assert routes["3term"] > 0 and routes["reorth"] > 0
