"""CPU: the extended-precision equality-QP reference (tests/qp_ref.py) against exact rational arithmetic, and its
problem generators against what they promise.  The GPU solve tests (test_gpu_solve_accuracy.py) rest on these."""
from fractions import Fraction

import numpy as np
import pytest

import qp_ref as Q

U = Q.U


def exact_solve(M, R):
    """M^-1 R in Fractions (the float64 inputs converted exactly), by Gaussian elimination with a non-zero pivot."""
    n, k = M.shape[0], R.shape[1]
    a = [[Fraction(float(v)) for v in M[i]] + [Fraction(float(v)) for v in R[i]] for i in range(n)]
    for c in range(n):
        p = next(i for i in range(c, n) if a[i][c] != 0)
        a[c], a[p] = a[p], a[c]
        for i in range(n):
            if i != c and a[i][c] != 0:
                f = a[i][c] / a[c][c]
                a[i] = [x - f * y for x, y in zip(a[i], a[c])]
    return [[a[i][n + j] / a[i][i] for j in range(k)] for i in range(n)]


def to_f64(F):
    return np.array([[float(v) for v in row] for row in F])


def exact_kkt(P, A, B):
    n, m = P.shape[0], A.shape[0]
    Kmat = np.block([[P, A.T], [A, np.zeros((m, m))]])
    rhs = np.vstack([np.zeros((n, B.shape[1])), B])
    return to_f64(exact_solve(Kmat, rhs)[:n])


def assert_ulps(got, exact, what):
    err = np.abs(got - exact) / np.maximum(np.abs(exact), 1e-300)
    assert np.all(err <= 4 * U), f"{what}: worst componentwise error {np.max(err) / U:.2f} u (bound 4 u)"


@pytest.mark.parametrize("kappa", [1e2, 1e8, 1e12])
@pytest.mark.parametrize("null_ones", [False, True])
@pytest.mark.parametrize("kind", ["pins", "com", "dense"])
def test_kkt_ref_is_correctly_rounded(kappa, null_ones, kind):
    n, m = 10, 3
    seed = int(np.log10(kappa)) * 10 + null_ones
    P = Q.spectrum_gram(n, kappa, null_ones, seed=seed)
    if kind == "pins":
        _, A = Q.pin_rows(n, m, seed)
    elif kind == "com":
        A = Q.com_rows(n, m, seed)
    else:
        A = np.random.default_rng(seed).standard_normal((m, n))
    B = np.eye(m) if kind != "dense" else np.random.default_rng(seed + 1).standard_normal((m, 2))
    ref = Q.kkt_ref(P, A, B)
    assert_ulps(ref.x, exact_kkt(P, A, B), f"kkt_ref {kind} kappa={kappa:.0e} null_ones={null_ones}")
    assert ref.steps <= Q.MAX_STEPS
    # one column only: the same values
    one = Q.kkt_ref(P, A, B, cols=[B.shape[1] - 1])
    assert np.array_equal(one.x[:, 0], ref.x[:, -1])


@pytest.mark.parametrize("kappa", [1e2, 1e8, 1e12])
@pytest.mark.parametrize("null_ones", [False, True])
def test_pinned_ref_is_correctly_rounded(kappa, null_ones):
    n, m = 13, 4
    P = Q.spectrum_gram(n, kappa, null_ones, seed=7 + int(np.log10(kappa)))
    pins, A = Q.pin_rows(n, m, seed=3)
    ref = Q.pinned_ref(P, pins)
    free = np.setdiff1d(np.arange(n), pins)
    exact = np.zeros((n, m))
    exact[free] = to_f64(exact_solve(P[np.ix_(free, free)], -P[np.ix_(free, pins)]))
    exact[pins, np.arange(m)] = 1.0
    assert_ulps(ref.x, exact, f"pinned_ref kappa={kappa:.0e} null_ones={null_ones}")
    # the general reference agrees on the same problem
    assert_ulps(Q.kkt_ref(P, A, np.eye(m)).x, exact, "kkt_ref on one-hot rows")


def test_redundant_rows_are_reduced():
    n, m = 11, 6
    P = Q.spectrum_gram(n, 1e6, True, seed=5)
    A, B = Q.redundant_rows(n, m, seed=5)
    keep = Q.independent_rows(A)
    assert len(keep) == np.linalg.matrix_rank(A) < m
    ref = Q.kkt_ref(P, A, B)
    assert_ulps(ref.x, exact_kkt(P, A[keep], B[keep]), "kkt_ref with redundant rows")
    assert np.max(np.abs(A @ ref.x - B)) < 64 * U * np.max(np.abs(B))


def test_exact_products_are_correctly_rounded():
    rng = np.random.default_rng(1)
    M = rng.standard_normal((7, 9)) * np.exp2(rng.integers(-30, 30, size=(7, 9)))
    x = rng.standard_normal((9, 2)) * np.exp2(rng.integers(-20, 20, size=(9, 2)))
    xl = x * 2.0 ** -60 * rng.standard_normal((9, 2))
    got = Q.exact_matmul(M, x, xl)
    for i in range(7):
        for j in range(2):
            ex = sum(Fraction(float(M[i, k])) * (Fraction(float(x[k, j])) + Fraction(float(xl[k, j]))) for k in range(9))
            assert got[i, j] == float(ex)


def test_refinement_refuses_a_hopeless_system():
    P = Q.spectrum_gram(12, 1e18, seed=2)  # kappa u > 1: the float64 corrections do not contract
    with pytest.raises(ValueError, match="converge|finite"):
        Q.pinned_ref(P, np.array([11]))


def test_backward_error_of_exact_and_perturbed_solutions():
    n, m = 10, 3
    P = Q.spectrum_gram(n, 1e8, True, seed=11)
    A = Q.com_rows(n, m, seed=11)
    B = np.eye(m)
    x = exact_kkt(P, A, B)
    eta0 = Q.backward_error(P, A, B, x)
    assert eta0 <= 4 * U, f"correctly rounded solution: eta = {eta0 / U:.2f} u"
    rng = np.random.default_rng(0)
    s = rng.choice([-1.0, 1.0], size=n)
    etas = []
    for delta in (1e-12, 1e-10):
        xp = x.copy()
        xp[:, 1] *= 1 + delta * s
        etas.append(Q.backward_error(P, A, B, xp))
    assert etas[0] > 1e-3 * 1e-12 and etas[0] > 20 * eta0, etas
    assert 50 < etas[1] / etas[0] < 200, etas  # proportional to the planted perturbation
    # the extended-precision pair of the reference is judged at least as well as its float64 rounding
    ref = Q.kkt_ref(P, A, B)
    assert Q.backward_error(P, A, B, (ref.x_hi, ref.x_lo)) <= 4 * U


@pytest.mark.parametrize("n,kappa", [(14, 1e2), (64, 1e6), (200, 1e10), (300, 1e12)])
@pytest.mark.parametrize("null_ones", [False, True])
def test_spectrum_gram_delivers(n, kappa, null_ones):
    G = Q.spectrum_gram(n, kappa, null_ones, seed=n)
    assert np.array_equal(G, G.T)
    if null_ones:
        assert np.max(np.abs(G @ np.ones(n))) <= 4 * n * U * np.max(np.abs(G))
    assert 0.5 * kappa <= Q.gram_cond(G, null_ones) <= 2 * kappa


def test_network_forces_deliver():
    T, N = 60, 40
    f = Q.network_forces(T, N, seed=3)
    assert f.shape == (T, N, 3)
    F = f.transpose(0, 2, 1).reshape(3 * T, N)
    G = F.T @ F
    assert np.max(np.abs(G @ np.ones(N))) <= 8 * N * U * np.max(np.abs(G)) * np.sqrt(3 * T)
    assert np.max(np.abs(f.sum(axis=1))) <= 64 * N * U * np.max(np.abs(f))
    kappa = Q.gram_cond(G, True)
    assert kappa > 1e3  # stiff bonds against soft cross-links
    # stiff along the bonds: the Rayleigh quotient of a bond stretch far above that of a slow mode
    bond = np.zeros(N)
    bond[[5, 6]] = [1.0, -1.0]
    slow = np.linspace(-1, 1, N)
    assert bond @ G @ bond / (bond @ bond) > 100 * (slow @ G @ slow) / (slow @ slow)


def test_deficient_gram_rank():
    G = Q.deficient_gram(30, 12, seed=1)
    w = np.linalg.eigvalsh(G)
    assert np.sum(w > 1e-10 * w[-1]) == 12


@pytest.mark.parametrize("gram", ["spectrum", "network"])
def test_reduced_problem_is_positive_definite_for_every_row_kind(gram):
    n, m = 48, 7
    if gram == "spectrum":
        P = Q.spectrum_gram(n, 1e10, True, seed=4)
    else:
        f = Q.network_forces(40, n, seed=4)
        F = f.transpose(0, 2, 1).reshape(-1, n)
        P = F.T @ F
    _, Apin = Q.pin_rows(n, m, seed=4)
    Ared, _ = Q.redundant_rows(n, m, seed=4)
    for A in (Apin, Q.com_rows(n, m, seed=4), Ared):
        kr = Q.reduced_cond(P, A)
        assert np.isfinite(kr) and kr < 1e13
    # a Gram singular on the feasible set is reported as such
    assert Q.reduced_cond(Q.deficient_gram(n, 10, seed=4), Apin) == float("inf")
