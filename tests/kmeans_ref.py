"""Reference for the device k-means (Context.kmeans_run / kmeans_seed, csrc/kmeans.hip): everything in
numpy.longdouble from direct differences.  No GPU, nothing of the library.

Lloyd, exactly the device's loop.  C_0 given; at iteration t = 0, 1, ...:
  1. assign to C_t: label_i = the j with the smallest (d2(i, j), j) — np.argmin, the first minimum;
     counts_t, inertia_t = sum_i d2(i, label_i), changed_t = #{i: label_i != the label of t - 1};
  2. stop, converged = 1, if t >= 1 and changed_t = 0;
  3. stop, converged = 2, if t >= 1, tol > 0 and |C_t - C_{t-1}|_F^2 <= tol;
  4. stop, converged = 0, if t = max_iter;
  5. C_{t+1}: the mean of every cluster; an empty cluster keeps its centre.
What returns is the triple (labels_t, C_t, inertia_t) with counts_t and n_iter = t.

k-means++ (plain): round 0 picks min(floor(u_0 n), n - 1); round r keeps w_i = min over the picked points
of d2(i, .), 0 by index for a picked point, and picks the smallest i with cumsum_i > u_r total — the
smallest index not yet picked if total = 0.

The device takes the distance in Gram form; the bound on it is the one of knn_ref:
    |d2_dev - d2| <= (d + 4) u (|x_i|^2 + |c_j|^2),    u = 2^-53.
The device's labels equal the reference's wherever the best and the second-best distance of every point
are further apart than that (``Lloyd.separation``, in units of the bound); the seeding's picks wherever
u_r total stays clear of every prefix sum (``seed``'s second result, relative to the total).
"""
from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -53
LD = np.longdouble

# (n, d, c, c_true): the 16- and 64-row edges, every fragment capacity KS from 1 to 64, d = 1, c = 2 and
# c = 256, c not a multiple of 16, clusters that go empty
SHAPES = [(65, 1, 2, 2), (130, 4, 3, 3), (200, 3, 2, 2), (257, 16, 5, 5), (1000, 17, 16, 8),
          (1025, 64, 33, 33), (640, 256, 64, 16), (4099, 5, 256, 40)]
EMPTY_SHAPES = [(640, 256, 64, 16), (4099, 5, 256, 40)]
SEEDS = (0, 1, 2)


def generate(n, d, c, c_true):
    """(X, C0) of a shape: c_true Gaussian blobs, the starting centres c equally spaced points."""
    rng = np.random.default_rng(1000 * n + c)
    mu = 3.0 * rng.standard_normal((c_true, d))
    X = mu[np.arange(n) % c_true] + 0.5 * rng.standard_normal((n, d))
    C0 = X[np.arange(c) * (n // c)]
    return X, C0.copy()


def sq_dists(X, C):
    """|x_i - c_j|^2 in longdouble from direct differences, n x c."""
    X = np.asarray(X, dtype=LD)
    C = np.asarray(C, dtype=LD)
    out = np.empty((X.shape[0], C.shape[0]), dtype=LD)
    for j in range(C.shape[0]):
        df = X - C[j]
        out[:, j] = (df * df).sum(axis=1)
    return out


def bound(X, C):
    """(d + 4) u (|x_i|^2 + |c_j|^2), n x c, fp64."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    return (X.shape[1] + 4.0) * U * ((X * X).sum(axis=1)[:, None] + (C * C).sum(axis=1)[None, :])


def assign(X, C):
    """(labels int32, d2 of the label longdouble, gap / bound of every point): the gap between the best
    and the second-best distance over the larger of the two pairs' bounds (inf for one centre)."""
    d2 = sq_dists(X, C)
    lab = np.argmin(d2, axis=1)
    rows = np.arange(d2.shape[0])
    best = d2[rows, lab]
    if d2.shape[1] == 1:
        return lab.astype(np.int32), best, np.full(d2.shape[0], np.inf)
    rest = d2.copy()
    rest[rows, lab] = np.inf
    second = np.argmin(rest, axis=1)
    B = bound(X, C)
    sep = (rest[rows, second] - best).astype(np.float64) / np.maximum(B[rows, lab], B[rows, second])
    return lab.astype(np.int32), best, sep


@dataclass
class State:
    """Iteration t as the device would return it."""
    labels: np.ndarray
    centers: np.ndarray          # C_t, longdouble
    inertia: LD
    counts: np.ndarray
    changed: int
    prev_labels: np.ndarray      # the labels C_t is the mean of (None at t = 0)
    prev_centers: np.ndarray     # C_{t-1} (None at t = 0)


@dataclass
class Lloyd:
    states: list = field(default_factory=list)
    converged: int = 0
    separation: float = np.inf   # min over points and iterations of gap / bound
    max_empty: int = 0

    @property
    def n_iter(self):
        return len(self.states) - 1

    @property
    def last(self):
        return self.states[-1]


def means(X, labels, C):
    """The next centres in longdouble: cluster means, an empty cluster keeping its row of C."""
    XL = np.asarray(X, dtype=LD)
    Cn = np.array(C, dtype=LD)
    for j in range(Cn.shape[0]):
        m = labels == j
        if m.any():
            Cn[j] = XL[m].sum(axis=0) / LD(int(m.sum()))
    return Cn


def lloyd(X, C0, max_iter=300, tol=0.0):
    c = np.asarray(C0).shape[0]
    run = Lloyd()
    C, Cprev, prev = np.asarray(C0, dtype=LD), None, None
    t = 0
    while True:
        lab, best, sep = assign(X, C)
        counts = np.bincount(lab, minlength=c).astype(np.int64)
        changed = X.shape[0] if prev is None else int((lab != prev).sum())
        run.states.append(State(lab, C, best.sum(), counts, changed, prev, Cprev))
        run.separation = min(run.separation, float(sep.min()))
        run.max_empty = max(run.max_empty, int((counts == 0).sum()))
        if t >= 1 and changed == 0:
            run.converged = 1
            return run
        if t >= 1 and tol > 0.0 and ((C - Cprev) ** 2).sum() <= tol:
            run.converged = 2
            return run
        if t == max_iter:
            return run
        Cprev, prev = C, lab
        C = means(X, lab, C)
        t += 1


def seed(X, uniforms):
    """(picked int32, the smallest |u_r total - cumsum_i| / total over all i and r >= 1 with total > 0)."""
    X = np.asarray(X, dtype=LD)
    n = X.shape[0]
    u = np.asarray(uniforms, dtype=np.float64)
    picked = [min(int(np.floor(u[0] * n)), n - 1)]
    w = np.full(n, np.inf, dtype=LD)
    sep = np.inf
    for r in range(1, u.size):
        df = X - X[picked[-1]]
        w = np.minimum(w, (df * df).sum(axis=1))
        w[picked] = 0
        cs = np.cumsum(w)
        total = cs[-1]
        if total == 0:
            taken = set(picked)
            picked.append(next(i for i in range(n) if i not in taken))
            continue
        target = LD(u[r]) * total
        sep = min(sep, float((np.abs(target - cs) / total).min()))
        picked.append(int(np.argmax(cs > target)))
    return np.array(picked, dtype=np.int32), sep


def lloyd_float64(X, C0, max_iter=300):
    """The same loop (tol = 0) in plain float64 Python loops: (labels, centres, n_iter, converged)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.array(C0, dtype=np.float64)
    n, c = X.shape[0], C.shape[0]
    prev, t = None, 0
    while True:
        lab = [0] * n
        for i in range(n):
            bd, bj = np.inf, -1
            for j in range(c):
                dd = 0.0
                for k in range(X.shape[1]):
                    dd += (X[i, k] - C[j, k]) ** 2
                if dd < bd:
                    bd, bj = dd, j
            lab[i] = bj
        if t >= 1 and lab == prev:
            return np.array(lab, dtype=np.int32), C, t, 1
        if t == max_iter:
            return np.array(lab, dtype=np.int32), C, t, 0
        Cn = C.copy()
        for j in range(c):
            rows = [i for i in range(n) if lab[i] == j]
            if rows:
                Cn[j] = X[rows].sum(axis=0) / len(rows)
        C, prev = Cn, lab
        t += 1


def lattice(side=6, d=3, copies=1):
    """The integer lattice {0 .. side - 1}^d, row-major, each point listed `copies` times in a row."""
    g = np.stack(np.meshgrid(*[np.arange(side)] * d, indexing="ij"), axis=-1).reshape(-1, d).astype(np.float64)
    return np.repeat(g, copies, axis=0)


# centres on lattice points and at midpoints: (1,1,1) is at 3 from both (0,0,0) and (2,2,2), (2,2,3) at
# 0.75 from (2.5,2.5,2.5) and ... — many exact ties, every quantity exact in float64
LATTICE_CENTRES = np.array([[0.0, 0.0, 0.0], [2.0, 2.0, 2.0], [2.5, 2.5, 2.5], [5.0, 5.0, 5.0], [0.0, 0.0, 5.0],
                            [3.0, 3.0, 3.0], [2.5, 0.5, 4.5]])


def lattice_step_float64(X, C):
    """One assignment and one update in float64 NumPy, exact on the lattice: (labels, counts, inertia,
    the next centres)."""
    d2 = ((X[:, None, :] - C[None, :, :]) ** 2).sum(axis=2)
    lab = np.argmin(d2, axis=1).astype(np.int32)
    counts = np.bincount(lab, minlength=C.shape[0]).astype(np.int64)
    Cn = C.copy()
    for j in range(C.shape[0]):
        if counts[j]:
            Cn[j] = X[lab == j].sum(axis=0) / float(counts[j])
    return lab, counts, float(d2[np.arange(X.shape[0]), lab].sum()), Cn, d2


def three_blobs(n, d, rng, scale=4.0):
    """The driver test's points: centres scale e_c, c = 0, 1, 2; X[i] = centre[i % 3] + 0.35 N(0,1) / sqrt(d)."""
    centres = scale * np.eye(3, d)
    return centres[np.arange(n) % 3] + 0.35 * rng.standard_normal((n, d)) / np.sqrt(d)


def same_partition(a, b):
    """Two labelings describe one partition (up to a permutation of the label names)."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
