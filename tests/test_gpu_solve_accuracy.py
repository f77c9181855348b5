"""GPU: every entry point of the equality-QP solve (K2) against the extended-precision reference of tests/qp_ref.py, at
the 64-wide step and 256-wide outer-panel edges and at condition numbers up to 1e12, where a blocked Cholesky with
explicitly inverted diagonal blocks loses accuracy first.

Bounds per case (u = 2^-53), fixed before any run:
  * no false breakdown: stats[0] == 0 wherever np.linalg.cholesky of the host-formed P~ = P/s + A'A succeeds;
  * normwise backward error (qp_ref.backward_error) eta <= 4 n u;
  * forward error max|x - x_ref| / max|x_ref| per column <= 10 x that of a plain float64 np.linalg.solve of the same
    KKT system + 64 u ("no worse than LAPACK", which calibrates itself across kappa);  with schur_reg > 0 (which
    perturbs the problem by design) the forward bound plus an allowance for the shift that the test derives, and no
    backward-error bound;
  * stats[1] = the exact max|A X' - B| of the returned X, up to 1e-3 of it and the rounding of the float64 product
    that forms it on the device (slack = n u max |A||X'|); stats[1] <= stats[2] + slack whenever n_refine > 0.
Every message carries n, m, kappa, eta / (n u) and the forward-error ratio (error / bound)."""
import warnings

import numpy as np
import pytest
import torch

import qp_ref as Q

pytestmark = pytest.mark.gpu

from aggforce_amd import LinearMap, Trajectory, qp_linear_map  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd.qp import qplinear  # noqa: E402

U = Q.U
NS = [63, 64, 65, 255, 256, 257, 511, 513, 1025, 2047]
MS = [1, 17, 64, 65, 130]
KAPPAS = [1e2, 1e6, 1e10, 1e12]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.cpu().numpy()


def sample_cols(k, n):
    """all right-hand sides, or 16 spread over them (first and last included) from n = 2048 on"""
    return np.arange(k) if n < 2048 or k <= 16 else np.unique(np.linspace(0, k - 1, 16).round().astype(int))


def rows(kind, n, m, seed):
    if kind == "pins":
        return Q.pin_rows(n, m, seed)[1]
    if kind == "com":
        return Q.com_rows(n, m, seed)
    return np.random.default_rng(seed).standard_normal((m, n))


def cholesky_ok(P, A, s):
    try:
        np.linalg.cholesky(P / s + A.T @ A)
        return True
    except np.linalg.LinAlgError:
        return False


def judge(tag, X, P, A, B, ref, kappa, st=None, n_refine=None, extra=0.0):
    """X (n, k): the device's solutions of the columns B (m, k); ref the reference of the same columns."""
    n, m = P.shape[0], A.shape[0]
    eta = Q.backward_error(P, A, B, X)
    fe = Q.forward_error(X, ref.x)
    bound = 10 * Q.forward_error(ref.x_lapack, ref.x) + 64 * U + extra
    msg = (f"{tag}: n={n} m={m} kappa={kappa:.0e} eta/(n u)={eta / (n * U):.3g} forward={fe:.3e} "
           f"lapack={Q.forward_error(ref.x_lapack, ref.x):.3e} ratio={fe / bound:.3g}")
    print("ACCURACY", msg)
    if extra == 0.0:
        assert eta <= 4 * n * U, msg
    assert fe <= bound, msg
    if st is not None and n_refine is not None:
        r = np.max(np.abs(Q.sum_k(Q.ExactMatrix(A).terms(X) + [-B])))
        slack = n * U * np.max(np.abs(A) @ np.abs(X)) + U * np.max(np.abs(B))
        assert abs(st[1] - r) <= 1e-3 * r + slack, f"{msg}: stats[1]={st[1]:.3e}, exact residual {r:.3e}"
        if n_refine > 0:  # (at the rounding floor of the product that forms it, the residual is noise either way)
            assert st[1] <= st[2] + slack, f"{msg}: refinement raised the constraint residual {st[2]:.3e} -> {st[1]:.3e}"
    return eta / (n * U), fe / bound


# ---- K.eq_qp_solve, n_refine 0 / 1 / 3 ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_general_solve_against_reference(n):
    i = NS.index(n)
    ms = [m for m in MS if m < n]
    for j, kappa in enumerate(KAPPAS):
        m, null_ones, kind = ms[(i + j) % len(ms)], j % 2 == 1, ("com", "dense", "pins")[(i + j) % 3]
        seed = 100 * i + j
        G = Q.spectrum_gram(n, kappa, null_ones, seed)
        A = rows(kind, n, m, seed)
        B = np.eye(m) if kind != "dense" else np.random.default_rng(seed).standard_normal((m, min(m, 9)))
        l2 = 0.0 if j < 2 else 1e-14  # (a shift below every eigenvalue but the smallest: no change of kappa)
        P = G + l2 * np.eye(n)
        s = np.max(np.diag(P))
        assert cholesky_ok(P, A, s), f"n={n} kappa={kappa:.0e}: host Cholesky of P~ fails -- the case is not usable"
        ref = Q.kkt_ref(P, A, B)
        for n_refine in (0, 1, 3):
            X, st = K.eq_qp_solve(dev(G), l2, None, dev(A), dev(B), n_refine=n_refine)
            st = host(st)
            assert st[0] == 0, f"false breakdown at pivot {st[0]}: n={n} m={m} kappa={kappa:.0e} {kind}"
            assert st[3] == s
            judge(f"general[{kind},n_refine={n_refine}]", host(X).T, P, A, B, ref, kappa, st, n_refine)


# ---- K.eq_qp_solve_pinned ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_pinned_solve_against_reference(n):
    i = NS.index(n)
    ms = [m for m in MS if m < n]
    for j, kappa in enumerate(KAPPAS):
        m, null_ones = ms[(i + 2 * j + 1) % len(ms)], j % 2 == 0
        seed = 100 * i + j + 50
        G = Q.spectrum_gram(n, kappa, null_ones, seed)
        pins, A = Q.pin_rows(n, m, seed)
        s = np.max(np.diag(G))
        assert cholesky_ok(G, A, s)
        ref = Q.pinned_ref(G, pins)
        X, st = K.eq_qp_solve_pinned(dev(G), 0.0, None, dev(pins))
        st = host(st)
        assert st[0] == 0 and st[1] == 0 and st[3] == s, f"n={n} m={m} kappa={kappa:.0e}: stats {st}"
        X = host(X).T
        assert np.array_equal(X[pins], np.eye(m))
        judge("pinned", X, G, A, np.eye(m), ref, kappa)


# ---- the c3 size: n = 4096, m = 256, pinned and general, 16 sampled right-hand sides --------------------------------
@pytest.mark.parametrize("kappa", [1e6, 1e10])
def test_c3_sized_solves_against_reference(kappa):
    n, m = 4096, 256
    G = Q.spectrum_gram(n, kappa, True, seed=4096)
    pins, A = Q.pin_rows(n, m, seed=4096)
    cols = sample_cols(m, n)
    s = np.max(np.diag(G))
    Xp, sp = K.eq_qp_solve_pinned(dev(G), 0.0, None, dev(pins))
    sp = host(sp)
    assert sp[0] == 0
    judge("pinned c3", host(Xp)[cols].T, G, A, np.eye(m)[:, cols], Q.pinned_ref(G, pins, cols), kappa)
    Ac = Q.com_rows(n, m, seed=4097)
    assert cholesky_ok(G, Ac, s)
    Xg, sg = K.eq_qp_solve(dev(G), 0.0, None, dev(Ac), dev(np.eye(m)), n_refine=1)
    sg = host(sg)
    assert sg[0] == 0
    B = np.eye(m)[:, cols]
    judge("general c3", host(Xg)[cols].T, G, Ac, B, Q.kkt_ref(G, Ac, np.eye(m), cols), kappa)


# ---- K.eq_qp_solve_batched -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "AtA", "AtA+perm+first_col", "schur_reg"])
@pytest.mark.parametrize("n,m", [(65, 17), (257, 64), (513, 130)])
def test_batched_solve_against_reference(variant, n, m):
    rng = np.random.default_rng(n * 7 + m)
    kappas = [1e2, 1e10, 1e12]
    p = len(kappas)
    Gs = np.stack([Q.spectrum_gram(n, k, q % 2 == 1, seed=n + q) for q, k in enumerate(kappas)])
    As, Bs, perms = [], [], []
    touched = np.sort(rng.choice(n, size=min(n - 1, max(m + 8, n // 3)), replace=False))
    untouched = np.setdiff1d(np.arange(n), touched)
    for q in range(p):
        if variant == "schur_reg":
            A, B = Q.redundant_rows(n, m, seed=n + q, touched=touched)
            B = B[:, :5]
        elif variant == "AtA+perm+first_col":
            A, B = Q.com_rows(n, m, seed=n + q, touched=touched), np.eye(m)
        else:
            A, B = rows(("com", "dense", "pins")[q], n, m, seed=n + q), np.eye(m)
        As.append(A)
        Bs.append(B)
        perms.append(np.concatenate([rng.permutation(untouched), rng.permutation(touched)]).astype(np.int32))
    As, Bs = np.stack(As), np.stack(Bs)
    kw = dict(schur_reg=0.0, n_refine=1)
    if variant == "schur_reg":
        kw = dict(schur_reg=1e-12, n_refine=3)
    if variant.startswith("AtA"):
        kw["AtA"] = dev(np.einsum("pki,pkj->pij", As, As))
    if variant == "AtA+perm+first_col":
        kw["perm"] = dev(np.stack(perms))
        kw["a_first_col"] = len(untouched)
    X, st = K.eq_qp_solve_batched(dev(Gs), 0.0, None, dev(As), dev(Bs), **kw)
    X, st = host(X), host(st)
    for q, kappa in enumerate(kappas):
        G, A, B = Gs[q], As[q], Bs[q]
        s = np.max(np.diag(G))
        assert st[q, 3] == s
        ref = Q.kkt_ref(G, A, B)
        if variant != "schur_reg":
            assert cholesky_ok(G, A, s)
            assert st[q, 0] == 0, f"false breakdown, problem {q}, {variant}: stats {st[q]}"
            judge(f"batched[{variant}]", X[q].T, G, A, B, ref, kappa, st[q], kw["n_refine"])
            continue
        # schur_reg > 0 perturbs the problem by design: S + delta I with delta = reg trace(S) scales the Schur component
        # along an eigenvalue sigma of S by sigma / (sigma + delta); every refinement step on the constraint residual
        # multiplies what is left by rho = delta / (sigma_min + delta) (sigma_min: the smallest non-zero eigenvalue).
        # The components are P~-orthogonal, so |dx|_P~ <= rho^(k+1) |x|_P~, hence
        #     |dx|_inf <= rho^(n_refine + 1) sqrt(kappa(P~)) sqrt(n) |x|_inf.
        Pt = G / s + A.T @ A
        wS = np.linalg.eigvalsh(A @ np.linalg.solve(Pt, A.T))
        r = len(Q.independent_rows(A))
        delta = 1e-12 * np.sum(wS)
        rho = delta / (wS[m - r] + delta)
        wP = np.linalg.eigvalsh(Pt)
        allowance = rho ** (kw["n_refine"] + 1) * np.sqrt(wP[-1] / wP[0]) * np.sqrt(n)
        assert st[q, 0] == 0
        judge(f"batched[{variant}] (allowance {allowance:.1e})", X[q].T, G, A, B, ref, kappa, extra=allowance)
        assert np.max(np.abs(A @ X[q].T - B)) < 1e-9 * np.max(np.abs(B))


# ---- exact metamorphic checks: scaling by a power of two, and no cross-talk between problems ---------------------------
@pytest.mark.parametrize("n,m", [(130, 17), (513, 65)])
def test_power_of_two_scaling_is_bit_exact(n, m):
    G = Q.spectrum_gram(n, 1e8, True, seed=n)
    d = np.random.default_rng(n).uniform(1, 4, size=n)
    l2 = 0.25
    A = Q.com_rows(n, m, seed=n)
    pins, _ = Q.pin_rows(n, m, seed=n)
    B = np.eye(m)
    base = {
        "general": K.eq_qp_solve(dev(G), l2, dev(d), dev(A), dev(B), n_refine=1),
        "pinned": K.eq_qp_solve_pinned(dev(G), l2, dev(d), dev(pins)),
        "batched": K.eq_qp_solve_batched(dev(G[None]), l2, dev(d), dev(A[None]), dev(B[None]), n_refine=1),
    }
    for k in (-40, 40):
        f = 2.0 ** k
        got = {
            "general": K.eq_qp_solve(dev(G * f), l2 * f, dev(d), dev(A), dev(B), n_refine=1),
            "pinned": K.eq_qp_solve_pinned(dev(G * f), l2 * f, dev(d), dev(pins)),
            "batched": K.eq_qp_solve_batched(dev(G[None] * f), l2 * f, dev(d), dev(A[None]), dev(B[None]), n_refine=1),
        }
        for name, (X, st) in got.items():
            X0, st0 = base[name]
            assert torch.equal(X, X0), f"{name}: solve(2^{k} G) differs from solve(G)"
            st, st0 = host(st).reshape(-1), host(st0).reshape(-1)
            assert np.array_equal(st[:3], st0[:3]) and st[3] == st0[3] * f, (name, k, st, st0)
    # one batch holding G, 2^40 G and 2^-40 G: three bit-identical X (the per-problem strides keep them apart)
    Gs = np.stack([G, G * 2.0 ** 40, G * 2.0 ** -40])
    As, Bs = np.stack([A] * 3), np.stack([B] * 3)
    for kw in ({}, {"AtA": dev(np.stack([A.T @ A] * 3))}):
        X, st = K.eq_qp_solve_batched(dev(Gs), 0.0, None, dev(As), dev(Bs), n_refine=1, **kw)
        assert torch.equal(X[0], X[1]) and torch.equal(X[0], X[2]), kw.keys()
        assert np.array_equal(host(st)[:, 3], np.max(np.diag(G)) * np.array([1.0, 2.0 ** 40, 2.0 ** -40]))


# ---- end to end: qp_linear_map on MD-shaped forces, the Gram taken from the library itself ------------------------------
def network_case(T, N, n_cg, kind, bonds, seed):
    forces = Q.network_forces(T, N, seed)
    rng = np.random.default_rng(seed)
    sites = np.sort(rng.choice(np.arange(0, N, 2), size=n_cg, replace=False))
    if kind == "slice":
        cmap = LinearMap([[int(a)] for a in sites], n_fg_sites=N)
    else:
        M = np.zeros((n_cg, N))
        for i, a in enumerate(sites):
            M[i, a] = 0.7
            M[i, (a + 1) % N] = 0.3
        cmap = LinearMap(M)
    cons = {frozenset([2 * i + 1, 2 * i + 2]) for i in range(0, N // 2 - 1, 3)} if bonds else None
    return forces, cmap, cons


@pytest.mark.parametrize("kind", ["slice", "com"])
@pytest.mark.parametrize("bonds", [False, True])
def test_qp_linear_map_end_to_end_against_reference(kind, bonds):
    N, n_cg = 300, 12
    forces, cmap, cons = network_case(200, N, n_cg, kind, bonds, seed=7 + 2 * bonds + (kind == "com"))
    l2 = 0.0
    prob = qplinear.LinearProblem(cmap, cons, "cuda")
    assert (prob.pins is not None) == (kind == "slice")
    G = host(prob.gram(K.as_device(forces)))
    sizes = host(prob.sizes)
    P = G + l2 * np.diag(sizes)
    A = prob.A
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a well-posed fit must not warn
        W = qp_linear_map(Trajectory(coords=forces, forces=forces), cmap, cons, l2).force_map.standard_matrix
    first = np.array([np.flatnonzero(prob.goa == g)[0] for g in range(prob.n_red)])
    X = np.asarray(W)[:, first].T
    assert np.array_equal(np.asarray(W), X.T[:, prob.goa])
    ref = Q.kkt_ref(P, A, np.eye(n_cg))
    kappa = Q.reduced_cond(P, A)
    judge(f"qp_linear_map[{kind},bonds={bonds}]", X, P, A, np.eye(n_cg), ref, kappa)


# ---- rank-deficient sweep: P singular on the feasible set, l2 = 0 -------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 700])
@pytest.mark.parametrize("kind", ["slice", "com"])
def test_rank_deficient_fits_warn_and_return_the_shifted_solution(n, kind):
    """3T < n_free: every case must warn, and W must be the solution of the problem that the retry solves
    (l2 + 1e-10 s, the same l2_diag).  A case that does not warn is a breakdown missed on the sign of rounding noise."""
    n_cg = 8
    warned, worst = 0, (0.0, 0.0)
    seeds = range(16)
    for seed in seeds:
        if seed % 2 == 0:  # few frames of the harmonic network through qp_linear_map
            T = (n - n_cg) // 3 - 1 - seed % 5
            forces, cmap, _ = network_case(T, n, n_cg, kind, False, seed=1000 * n + seed)
            prob = qplinear.LinearProblem(cmap, None, "cuda")
            G = host(prob.gram(K.as_device(forces)))
            with warnings.catch_warnings(record=True) as wl:
                warnings.simplefilter("always")
                W = qp_linear_map(Trajectory(coords=forces, forces=forces), cmap, None, 0.0).force_map.standard_matrix
            X = np.asarray(W).T
        else:  # a Gram of low rank through the same solve (LinearProblem.solve, what qp_linear_map calls)
            _, cmap, _ = network_case(1, n, n_cg, kind, False, seed=1000 * n + seed)
            prob = qplinear.LinearProblem(cmap, None, "cuda")
            G = Q.deficient_gram(n, (n - n_cg) // 2 + seed, seed=seed)
            with warnings.catch_warnings(record=True) as wl:
                warnings.simplefilter("always")
                X = host(prob.solve(dev(G), 0.0)).T
        msgs = [str(w.message) for w in wl]
        warned += any("singular" in w and "not unique" in w for w in msgs)
        s = np.max(np.diag(G))
        P = G + (0.0 + 1e-10 * s) * np.diag(host(prob.sizes))
        A = prob.A
        ref = Q.kkt_ref(P, A, np.eye(n_cg))
        e, f = judge(f"rank-deficient[{kind},seed={seed},warned={bool(msgs)}]", X, P, A, np.eye(n_cg), ref,
                     Q.reduced_cond(P, A))
        worst = (max(worst[0], e), max(worst[1], f))
    print(f"ACCURACY rank-deficient n={n} {kind}: {warned} of {len(seeds)} cases warned; worst eta/(n u) "
          f"{worst[0]:.3g}, forward ratio {worst[1]:.3g}")
    assert warned == len(seeds), f"n={n} {kind}: only {warned} of {len(seeds)} singular fits warned"
