"""Extended-precision host reference for the equality-QP solve (K2), for tests/test_qp_ref_host.py and
tests/test_gpu_solve_accuracy.py.  NumPy and the standard library only; nothing under aggforce_amd/ imports it.

    min 1/2 x'Px  s.t.  Ax = b      <=>      [P A'; A 0] [x; lam] = [0; b]

``kkt_ref`` solves the KKT system once in float64 (np.linalg.solve, also handed back as the LAPACK yardstick) and then
refines it.  The residuals are exact up to one final rounding: every matrix product is split into float64 products
that cannot round (Ozaki's error-free transformation: row-scaled pieces of the matrix times column-scaled pieces of
the iterate, each an integer multiple of its scale with at most ``beta`` bits, 2 beta + log2(k) <= 53), and the
partial results are summed in three-fold precision (Ogita, Rump & Oishi's SumK).  The iterate is carried as an
unevaluated pair hi + lo (double-double).  The refinement stops once the correction falls below 2^-80 of the iterate
(the residual is exact, so that is far below what float64 rounding of the result needs) and raises if it does not get
there within 10 steps: such a case is too ill-conditioned for this reference and a test must not use it.
"""
from collections import namedtuple

import numpy as np

U = 2.0 ** -53
TOL = 2.0 ** -80
MAX_STEPS = 10

Ref = namedtuple("Ref", "x x_hi x_lo lam_hi lam_lo x_lapack steps")


# ---- error-free products and accurate sums ---------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def sum_k(terms, k=3):
    """fl(exact sum of the equally shaped float64 arrays in ``terms``) as if computed in k-fold precision (SumK)."""
    p = [np.asarray(t, dtype=np.float64) for t in terms]
    if len(p) == 1:
        return p[0].copy()
    for _ in range(k - 1):
        for i in range(1, len(p)):
            p[i], p[i - 1] = _two_sum(p[i], p[i - 1])
    acc = p[0].copy()
    for t in p[1:-1]:
        acc = acc + t
    return acc + p[-1]


def _beta(k):
    """bits per piece for exact float64 sums of k products of two pieces"""
    return (53 - int(np.ceil(np.log2(max(k, 2))))) // 2


def split(M, axis, beta):
    """Pieces whose sum is M exactly.  Along ``axis`` (1: per row, 0: per column) every piece is an integer multiple of
    2^(e - beta) with magnitude <= 2^e for one e per row (column): a product of a row piece and a column piece
    summed over k <= 2^(53 - 2 beta) terms is exact in float64, whatever the order of the sum."""
    R = np.array(M, dtype=np.float64, copy=True)
    if not np.all(np.isfinite(R)):
        raise ValueError("split: non-finite input")
    pieces = []
    for _ in range(12):
        mx = np.max(np.abs(R), axis=axis, keepdims=True)
        if not np.any(mx > 0):
            return pieces
        e = np.frexp(np.where(mx > 0, mx, 1.0))[1].astype(np.float64)  # |R| <= 2^e along the axis
        sigma = np.where(mx > 0, 0.75 * np.exp2(e + 53 - beta), 0.0)  # 1.5 * 2^(e + 52 - beta): one binade for R + sigma
        piece = (R + sigma) - sigma
        pieces.append(piece)
        R = R - piece
    raise AssertionError("split did not terminate")


class ExactMatrix:
    """A float64 matrix whose products with float64 column blocks are returned as lists of exact float64 terms."""

    def __init__(self, M):
        self.M = np.ascontiguousarray(M, dtype=np.float64)
        self.beta = _beta(self.M.shape[1])
        self.pieces = split(self.M, 1, self.beta)

    def terms(self, *xs):
        """float64 arrays whose exact sum is M @ (sum of xs)"""
        xp = [q for x in xs for q in split(np.asarray(x, dtype=np.float64).reshape(self.M.shape[1], -1), 0, self.beta)]
        if not xp:
            return [np.zeros((self.M.shape[0], np.asarray(xs[0]).reshape(self.M.shape[1], -1).shape[1]))]
        X = np.concatenate(xp, axis=1)
        w = xp[0].shape[1]
        out = []
        for P in self.pieces:
            Y = P @ X
            out.extend(Y[:, i * w:(i + 1) * w] for i in range(len(xp)))
        return out or [np.zeros((self.M.shape[0], w))]


def exact_matmul(M, *xs):
    """fl(M @ sum(xs)) from exact products (one rounding)"""
    return sum_k(ExactMatrix(M).terms(*xs))


# ---- the reference solves ----------------------------------------------------------------------------------------------
def independent_rows(A, rtol=1e-9):
    """Indices of a maximal set of linearly independent rows of A, first come first kept (Gram-Schmidt, twice)."""
    A = np.asarray(A, dtype=np.float64)
    Q = np.zeros((0, A.shape[1]))
    keep = []
    for i, a in enumerate(A):
        r = a.copy()
        for _ in range(2):
            r = r - Q.T @ (Q @ r)
        nr = np.linalg.norm(r)
        if nr > rtol * max(np.linalg.norm(a), 1e-300):
            Q = np.vstack([Q, r / nr])
            keep.append(i)
    return np.asarray(keep, dtype=np.int64)


def _refine(Kmat, rhs):
    """Solution of Kmat y = rhs (columns): float64 solve, then refinement with exact residuals and a double-double
    iterate.  Returns (hi, lo, y_lapack, steps)."""
    y0 = np.linalg.solve(Kmat, rhs)
    if not np.all(np.isfinite(y0)):
        raise ValueError("reference: the float64 solve is not finite")
    EK = ExactMatrix(Kmat)
    Kinv = np.linalg.inv(Kmat) if Kmat.shape[0] > 600 else None
    hi, lo = y0.copy(), np.zeros_like(y0)
    for step in range(1, MAX_STEPS + 1):
        r = sum_k([rhs] + [-t for t in EK.terms(hi, lo)])
        d = Kinv @ r if Kinv is not None else np.linalg.solve(Kmat, r)
        s, e = _two_sum(hi, d)
        hi, lo = _two_sum(s, e + lo)
        if np.max(np.abs(d)) <= TOL * np.max(np.abs(hi)):
            return hi, lo, y0, step
    raise ValueError(f"reference refinement did not converge in {MAX_STEPS} steps (last correction "
                     f"{np.max(np.abs(d)) / np.max(np.abs(hi)):.1e} of the iterate): too ill-conditioned for this reference")


def kkt_ref(P, A, B, cols=None):
    """x = argmin 1/2 x'Px s.t. A x = B[:, c] for the columns c of B in ``cols`` (all by default).  Redundant rows of A
    are dropped first (the right-hand sides must be consistent).  Returns Ref: x (n, k) float64, x_hi/x_lo and
    lam_hi/lam_lo the extended-precision solution (lam for the independent rows), x_lapack the plain float64 solve of
    the same (reduced) KKT system, steps the refinement steps taken."""
    P = np.asarray(P, dtype=np.float64)
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    B = np.asarray(B, dtype=np.float64).reshape(A.shape[0], -1)
    if cols is not None:
        B = B[:, np.asarray(cols)]
    keep = independent_rows(A)
    A, B = A[keep], B[keep]
    n, m = P.shape[0], A.shape[0]
    Kmat = np.zeros((n + m, n + m))
    Kmat[:n, :n] = P
    Kmat[:n, n:] = A.T
    Kmat[n:, :n] = A
    rhs = np.zeros((n + m, B.shape[1]))
    rhs[n:] = B
    hi, lo, y0, steps = _refine(Kmat, rhs)
    return Ref(hi[:n] + lo[:n], hi[:n], lo[:n], hi[n:], lo[n:], y0[:n], steps)


def pinned_ref(P, pins, cols=None):
    """The one-hot case that aggf_eq_qp_solve_pinned solves: x[pins[j]] = delta_jc, x_f = -P_ff^-1 P[f, pins[c]].
    Returns Ref with x (n, k) (the pinned entries included; lam empty)."""
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[0]
    pins = np.asarray(pins, dtype=np.int64)
    cols = np.arange(len(pins)) if cols is None else np.asarray(cols)
    free = np.setdiff1d(np.arange(n), pins)
    rhs = -P[np.ix_(free, pins[cols])]
    hi_f, lo_f, y0_f, steps = _refine(P[np.ix_(free, free)], rhs)
    hi, lo, y0 = (np.zeros((n, len(cols))) for _ in range(3))
    for full, part in ((hi, hi_f), (lo, lo_f), (y0, y0_f)):
        full[free] = part
    for j, c in enumerate(cols):
        hi[pins[c], j] = y0[pins[c], j] = 1.0
    empty = np.zeros((0, len(cols)))
    return Ref(hi + lo, hi, lo, empty, empty, y0, steps)


def backward_error(P, A, B, X):
    """Normwise backward error of candidate solutions X (n, k) -- or an (hi, lo) pair -- of the KKT system, the largest
    over the columns:  eta = max(|r1| / (|P| |x| + |A| |lam|), |r2| / (|A| |x| + |b|))  (infinity norms) with
    lam = argmin |P x + A' lam|, r1 = P x + A' lam, r2 = A x - b; P x, r1 and r2 from exact products."""
    P = np.asarray(P, dtype=np.float64)
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    B = np.asarray(B, dtype=np.float64).reshape(A.shape[0], -1)
    xs = tuple(np.asarray(x, dtype=np.float64).reshape(P.shape[0], -1) for x in (X if isinstance(X, tuple) else (X,)))
    EP, EA, EAt = ExactMatrix(P), ExactMatrix(A), ExactMatrix(A.T)
    p_terms = EP.terms(*xs)
    Px = sum_k(p_terms)
    lam = -np.linalg.lstsq(A.T, Px, rcond=None)[0]
    r1 = sum_k(p_terms + EAt.terms(lam))
    r2 = sum_k(EA.terms(*xs) + [-B])
    nP, nA = np.max(np.sum(np.abs(P), axis=1)), np.max(np.sum(np.abs(A), axis=1))
    x_inf = np.max(np.abs(sum_k(xs)), axis=0)
    e1 = np.max(np.abs(r1), axis=0) / np.maximum(nP * x_inf + nA * np.max(np.abs(lam), axis=0), 1e-300)
    e2 = np.max(np.abs(r2), axis=0) / np.maximum(nA * x_inf + np.max(np.abs(B), axis=0), 1e-300)
    return float(np.max(np.maximum(e1, e2)))


def forward_error(X, Xref):
    """max over columns of max|x - x_ref| / max|x_ref|"""
    X, Xref = np.asarray(X, dtype=np.float64), np.asarray(Xref, dtype=np.float64)
    return float(np.max(np.max(np.abs(X - Xref), axis=0) / np.maximum(np.max(np.abs(Xref), axis=0), 1e-300)))


def null_basis(A):
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    _, sv, Vt = np.linalg.svd(A, full_matrices=True)
    rank = int(np.sum(sv > sv[0] * max(A.shape) * U)) if sv.size else 0
    return Vt[rank:].T


def reduced_cond(P, A):
    """kappa_2(Z'PZ), Z a null-space basis of A (inf if Z'PZ is not positive definite)"""
    Z = null_basis(A)
    w = np.linalg.eigvalsh(Z.T @ np.asarray(P, dtype=np.float64) @ Z)
    return float(w[-1] / w[0]) if w[0] > 0 else float("inf")


# ---- problem generators (deterministic in the seed) ----------------------------------------------------------------
def spectrum_gram(n, kappa, null_ones=False, seed=0):
    """Q diag(logspace(0, -log10 kappa)) Q' with a random orthogonal Q; null_ones: the all-ones vector is an exact
    null vector (zero net force) and the spectrum is laid on its complement."""
    rng = np.random.default_rng(seed)
    if null_ones:
        Q, _ = np.linalg.qr(np.column_stack([np.ones(n), rng.standard_normal((n, n - 1))]))
        Q[:, 0] = 1.0 / np.sqrt(n)
        lam = np.concatenate([[0.0], np.logspace(0, -np.log10(kappa), n - 1)])
    else:
        Q, R = np.linalg.qr(rng.standard_normal((n, n)))
        Q = Q * np.sign(np.diag(R))
        lam = np.logspace(0, -np.log10(kappa), n)
    G = (Q * lam) @ Q.T
    G = 0.5 * (G + G.T)
    if null_ones:  # G 1 = 0 to rounding: remove the row means symmetrically
        G = G - G.mean(axis=1, keepdims=True)
        G = G - G.mean(axis=0, keepdims=True)
        G = 0.5 * (G + G.T)
    return G


def gram_cond(G, null_ones=False):
    """kappa_2 of G, on the complement of the all-ones vector if null_ones"""
    w = np.linalg.eigvalsh(G)
    if null_ones:
        w = np.sort(np.abs(w))[1:]
    return float(w[-1] / w[0])


def network_forces(T, N, seed=0):
    """Forces (T, N, 3) of a harmonic network at kT = 1: bonds (i, i+1) of stiffness 10^U(2,4), N // 2 random
    cross-links of stiffness 10^U(-1,1); thermal displacements over the non-zero modes of the stiffness Laplacian,
    f = -K u, mean removed per frame (zero net force: the Gram is singular along ones and stiff along the bonds)."""
    rng = np.random.default_rng(seed)
    Kl = np.zeros((N, N))

    def spring(i, j, k):
        Kl[i, i] += k
        Kl[j, j] += k
        Kl[i, j] -= k
        Kl[j, i] -= k

    for i in range(N - 1):
        spring(i, i + 1, 10.0 ** rng.uniform(2, 4))
    for _ in range(N // 2):
        i, j = rng.choice(N, size=2, replace=False)
        spring(i, j, 10.0 ** rng.uniform(-1, 1))
    w, V = np.linalg.eigh(Kl)
    V, w = V[:, 1:], w[1:]  # the translation mode (ones) carries no force
    xi = rng.standard_normal((T, 3, N - 1)) / np.sqrt(w)
    u = np.einsum("ik,tdk->tid", V, xi)
    f = -np.einsum("ij,tjd->tid", Kl, u)
    return f - f.mean(axis=1, keepdims=True)


def deficient_gram(n, rank, seed=0):
    """R'R with R of ``rank`` Gaussian rows"""
    R = np.random.default_rng(seed).standard_normal((rank, n))
    return R.T @ R


def pin_rows(n, m, seed=0):
    """(pins, A): m distinct one-hot rows (slice maps)"""
    pins = np.random.default_rng(seed).choice(n, size=m, replace=False).astype(np.int32)
    A = np.zeros((m, n))
    A[np.arange(m), pins] = 1.0
    return pins, A


def com_rows(n, m, seed=0, touched=None):
    """centre-of-mass rows over disjoint groups of 1-4 variables (of ``touched``, default all) with unequal weights
    (summing to 1)"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(np.arange(n) if touched is None else np.asarray(touched))
    if len(order) < m:
        raise ValueError("com_rows: fewer variables than rows")
    A = np.zeros((m, n))
    o = 0
    for i in range(m):
        size = min(int(rng.integers(1, 5)), len(order) - o - (m - i - 1))
        w = rng.uniform(1.0, 16.0, size=size)
        A[i, order[o:o + size]] = w / w.sum()
        o += size
    return A


def redundant_rows(n, m, seed=0, touched=None):
    """sparse rows over ``touched`` variables (default: a random third) of rank about half their number, half of them
    repeated: consistent but dependent rows as the featurised fit samples them.  Returns (A, B) with B = A X0 (m, m).
    Small integers (times one power of two) throughout, so that A and B are exact: the dependent rows of B are then consistent to the last
    bit (with rounded products they would not be, and the reference, which keeps the independent rows only, would
    solve a problem that differs from the device's by that rounding)."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.choice(n, size=max(2, n // 3), replace=False)) if touched is None else np.asarray(touched)
    A = np.zeros((m, n))
    basis = rng.integers(-4, 5, size=(max(1, min(m, len(t) // 2)), len(t))).astype(np.float64)
    A[:, t] = rng.integers(-3, 4, size=(m, basis.shape[0])).astype(np.float64) @ basis
    A *= 2.0 ** -float(np.frexp(np.max(np.abs(A)))[1])  # entries below 1 in magnitude, still exact
    A[m // 2:] = A[: m - m // 2]
    B = A @ rng.integers(-8, 9, size=(n, m)).astype(np.float64)
    return A, B
