"""Map validation on the GPU (aggforce_amd.jaxmapval, K7) against the NumPy float64 restatement in mapval_ref.py.

Tolerances are in units of the L1 scale of the summed terms: 1e-11 in float64, 1e-3 in float32 (against the oracle
evaluated on the float32-rounded inputs).  The reference tests' parameters are inner=6, outer=12, width=0.5 with
sq_args, i.e. offsets in [36, 144) and width 0.25 on squared distances; coordinates in a 10-wide box put many pairs
near the offsets."""
import numpy as np
import pytest
import torch

import mapval_ref as ref
from aggforce_amd import jaxmapval as mv
from aggforce_amd import _lib

pytestmark = pytest.mark.gpu

KW = dict(inner=6.0, outer=12.0, width=0.5)
TOL = {np.float64: 1e-11, np.float32: 1e-3}


def _data(T, n, seed, dtype=np.float64, fdtype=None, box=10.0):
    rng = np.random.default_rng(seed)
    X = (box * rng.random((T, n, 3))).astype(dtype)
    F = (30.0 * rng.standard_normal((T, n, 3))).astype(fdtype or dtype)
    return X, F


def _tol(*arrays):
    return TOL[np.float32] if all(a.dtype == np.float32 for a in arrays) else TOL[np.float64]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T", [1, 7, 1000])
@pytest.mark.parametrize("n", [1, 2, 3, 10, 63, 64, 65, 257])
def test_sq_gaussian_forces_and_energies_match_oracle(n, T, dtype):
    X, _ = _data(T, n, 1000 * n + T, dtype)
    # float32 forms x = |r_i - r_j|^2 to ~1e-7 relative: with width 0.25 on x ~ 100 that alone moves g by ~1e-3 at the
    # edge of the Gaussian, so the narrow case is checked in float64 and float32 takes a medium width
    narrow = (60.0, 0.25) if dtype == np.float64 else (60.0, 5.0)
    floor = 1e-300 if dtype == np.float64 else 1e-30  # float32 exp2 results below the normal range lose bits
    for offset, width in ((50.0, 30.0), narrow):
        G = mv.sq_gaussian_forces(X, offset, width)
        E = mv.sq_gaussian_energies(X, offset, width)
        assert isinstance(G, np.ndarray) and G.dtype == dtype and G.shape == X.shape
        assert isinstance(E, np.ndarray) and E.dtype == dtype and E.shape == (T,)
        Gr, scale = ref.forces(X.astype(np.float64), offset, width, scale=True)
        Er = ref.literal_energies(X.astype(np.float64), offset, width)
        tol = _tol(X)
        assert np.all(np.abs(G - Gr) <= tol * scale + floor), (offset, width, np.abs(G - Gr).max())
        assert np.all(np.abs(E - Er) <= tol * Er + floor), (offset, width)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sq_gaussian_forces_past_the_lds_tile(dtype):
    """n = 1100 > 1024 sites: the j loop runs over two LDS stages, a frame spans several site blocks."""
    X, F = _data(2, 1100, 77, dtype, box=20.0)
    offset, width = 150.0, 40.0
    G = mv.sq_gaussian_forces(torch.from_numpy(X).cuda(), offset, width)
    assert G.is_cuda and G.dtype == torch.from_numpy(X).dtype
    E = mv.sq_gaussian_energies(torch.from_numpy(X).cuda(), offset, width)
    Gr, scale = ref.forces(X.astype(np.float64), offset, width, scale=True)
    Er = ref.literal_energies(X.astype(np.float64), offset, width)
    tol = _tol(X)
    floor = 1e-300 if dtype == np.float64 else 1e-30
    assert np.all(np.abs(G.cpu().numpy() - Gr) <= tol * scale + floor)
    assert np.all(np.abs(E.cpu().numpy() - Er) <= tol * Er + floor)
    # the fused reductions past the tile too
    P = mv.random_force_proj(X, F, 37, np.random.default_rng(5), average=False, inner=10.0, outer=14.0, width=6.0)
    Pr, Ps = ref.random_force_proj(X, F, 37, 5, 10.0, 14.0, 6.0)
    assert np.all(np.abs(np.array(P) - Pr) <= tol * Ps)
    R = mv.random_residual_shift(X, F, 37, np.random.default_rng(5), inner=10.0, outer=14.0, width=6.0)
    Rr, Rs = ref.random_residual_shift(X, F, 37, 5, 10.0, 14.0, 6.0)
    assert np.all(np.abs(np.array(R) - Rr) <= tol * Rs)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("S", [1, 37, 1000])
def test_fused_projection_and_shift_match_oracle(S, average, dtype):
    X, F = _data(200, 10, S, dtype)
    tol = _tol(X, F)
    Pr, Ps = ref.random_force_proj(X, F, S, 42, **KW)
    Rr, Rs = ref.random_residual_shift(X, F, S, 42, **KW)
    P = mv.random_force_proj(X, F, S, np.random.default_rng(42), average=average, **KW)
    R = mv.random_residual_shift(X, F, S, np.random.default_rng(42), average=average, **KW)
    if average:
        assert isinstance(P, float) and isinstance(R, float)
        assert abs(P - Pr.mean()) <= tol * Ps.mean()
        assert abs(R - Rr.mean()) <= tol * Rs.mean()
    else:
        assert isinstance(P, list) and len(P) == S and all(isinstance(v, float) for v in P)
        assert isinstance(R, list) and len(R) == S and all(isinstance(v, float) for v in R)
        assert np.all(np.abs(np.array(P) - Pr) <= tol * Ps)
        assert np.all(np.abs(np.array(R) - Rr) <= tol * Rs)
    assert np.max(Ps) > 0 and np.max(Rs) > 0  # the offsets met pairs


@pytest.mark.parametrize("xd,fd", [(np.float32, np.float64), (np.float64, np.float32), (np.float32, np.float32),
                                   (np.float64, np.float64)])
def test_every_dtype_pair_is_launched(xd, fd):
    """Mixed pairs compute in float64 from the inputs as given: float64 tolerance against the rounded inputs."""
    X, F = _data(50, 12, 3, xd, fd)
    tol = _tol(X, F)
    P = mv.random_force_proj(X, F, 37, np.random.default_rng(1), average=False, **KW)
    Pr, Ps = ref.random_force_proj(X, F, 37, 1, **KW)
    assert np.all(np.abs(np.array(P) - Pr) <= tol * Ps)
    R = mv.random_residual_shift(X, F, 37, np.random.default_rng(1), **KW)
    Rr, Rs = ref.random_residual_shift(X, F, 37, 1, **KW)
    assert np.all(np.abs(np.array(R) - Rr) <= tol * Rs)
    ip = mv.mscg_ip(F, X)
    want = (F.astype(np.float64) * X.astype(np.float64)).sum() / F.shape[0]
    assert abs(ip - want) <= 1e-13 * np.abs(F.astype(np.float64) * X).sum() / F.shape[0]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_path_equals_generic_loop(dtype):
    X, F = _data(300, 16, 9, dtype)
    tol = _tol(X)
    Xd, Fd = torch.from_numpy(X).cuda(), torch.from_numpy(F).cuda()

    def generic(coords, randg=None, **kw):
        return mv.rsqpg_forces(coords, randg=randg, **kw)

    for fn in (mv.random_force_proj, mv.random_residual_shift):
        fused = fn(Xd, Fd, 64, np.random.default_rng(3), average=False, **KW)
        loop = fn(Xd, Fd, 64, np.random.default_rng(3), method=generic, average=False, **KW)
        _, scale = (ref.random_force_proj if fn is mv.random_force_proj else ref.random_residual_shift)(X, F, 64, 3, **KW)
        assert np.all(np.abs(np.array(fused) - np.array(loop)) <= tol * scale), fn.__name__


@pytest.mark.parametrize("shift", [False, True])
def test_uniform_forces_method_matches_oracle(shift):
    X, F = _data(100, 7, 4)
    fn = mv.random_residual_shift if shift else mv.random_force_proj
    got = fn(X, F, 9, np.random.default_rng(8), method=mv.random_uniform_forces, average=False)
    want, scale = ref.uniform_forces_loop(F, 9, 8, X.shape, shift)
    assert np.all(np.abs(np.array(got) - want) <= 1e-13 * scale)
    avg = fn(X, F, 9, np.random.default_rng(8), method=mv.random_uniform_forces, average=True)
    assert abs(avg - want.mean()) <= 1e-13 * scale.mean()


def test_projection_is_linear_in_the_forces_and_shift_identity():
    X, F1 = _data(400, 20, 21)
    _, F2 = _data(400, 20, 22)
    S = 50
    p1 = np.array(mv.random_force_proj(X, F1, S, np.random.default_rng(6), average=False, **KW))
    p2 = np.array(mv.random_force_proj(X, F2, S, np.random.default_rng(6), average=False, **KW))
    p12 = np.array(mv.random_force_proj(X, 2.0 * F1 - 3.0 * F2, S, np.random.default_rng(6), average=False, **KW))
    _, s1 = ref.random_force_proj(X, F1, S, 6, **KW)
    _, s2 = ref.random_force_proj(X, F2, S, 6, **KW)
    assert np.all(np.abs(p12 - (2.0 * p1 - 3.0 * p2)) <= 1e-11 * (2.0 * s1 + 3.0 * s2))
    # shift_s = gsq_s / (3 n T) - 2 P_s / (3 n), with gsq_s = sum |G_s|^2 from the forces entry point
    T, n, _ = X.shape
    sh = np.array(mv.random_residual_shift(X, F1, S, np.random.default_rng(6), **KW))
    offs, w = ref.offsets(6, S, **KW)
    gsq = np.array([(mv.sq_gaussian_forces(X, o, w) ** 2).sum() for o in offs])
    _, rs = ref.random_residual_shift(X, F1, S, 6, **KW)
    assert np.all(np.abs(sh - (gsq / (3 * n * T) - 2.0 * p1 / (3 * n))) <= 1e-11 * rs)


def test_coincident_sites_and_single_frame():
    X, F = _data(1, 6, 31)
    X[0, 3] = X[0, 1]  # two sites on top of each other
    X[0, 5] = X[0, 1]
    for offset, width in ((0.0, 1.0), (40.0, 20.0)):
        G = mv.sq_gaussian_forces(X, offset, width)
        Gr, scale = ref.forces(X, offset, width, scale=True)
        assert np.all(np.isfinite(G)) and np.all(np.abs(G - Gr) <= 1e-11 * scale + 1e-300)
        E = mv.sq_gaussian_energies(X, offset, width)
        np.testing.assert_allclose(E, ref.literal_energies(X, offset, width), rtol=1e-13)
    P = mv.random_force_proj(X, F, 37, np.random.default_rng(2), average=False, inner=0.0, outer=8.0, width=3.0)
    Pr, Ps = ref.random_force_proj(X, F, 37, 2, 0.0, 8.0, 3.0)
    assert np.all(np.abs(np.array(P) - Pr) <= 1e-11 * Ps)
    R = mv.random_residual_shift(X, F, 37, np.random.default_rng(2), inner=0.0, outer=8.0, width=3.0)
    Rr, Rs = ref.random_residual_shift(X, F, 37, 2, 0.0, 8.0, 3.0)
    assert np.all(np.abs(np.array(R) - Rr) <= 1e-11 * Rs)
    # one site: no pairs, nothing to project
    X1, F1 = _data(5, 1, 3)
    assert mv.random_force_proj(X1, F1, 4, np.random.default_rng(0), average=False, **KW) == [0.0] * 4
    assert mv.random_residual_shift(X1, F1, 4, np.random.default_rng(0), **KW) == [0.0] * 4


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nan_propagates(dtype):
    X, F = _data(20, 8, 12, dtype)
    X[3, 2, 1] = np.nan
    G = mv.sq_gaussian_forces(X, 50.0, 30.0)
    assert np.all(np.isnan(G[3])) and np.all(np.isfinite(np.delete(G, 3, axis=0)))
    E = mv.sq_gaussian_energies(X, 50.0, 30.0)
    assert np.isnan(E[3]) and np.all(np.isfinite(np.delete(E, 3)))
    assert all(np.isnan(v) for v in mv.random_force_proj(X, F, 5, np.random.default_rng(0), average=False, **KW))
    assert all(np.isnan(v) for v in mv.random_residual_shift(X, F, 5, np.random.default_rng(0), **KW))
    X2, F2 = _data(20, 8, 12, dtype)
    F2[0, 0, 0] = np.nan
    assert all(np.isnan(v) for v in mv.random_force_proj(X2, F2, 5, np.random.default_rng(0), average=False, **KW))
    assert np.isnan(mv.mscg_ip(F2, X2))


def test_two_calls_are_bit_identical():
    X, F = _data(3000, 64, 5)
    Xd, Fd = torch.from_numpy(X).cuda(), torch.from_numpy(F).cuda()
    for fn in (mv.random_force_proj, mv.random_residual_shift):
        a = fn(Xd, Fd, 1000, np.random.default_rng(1), average=False, **KW)
        b = fn(Xd, Fd, 1000, np.random.default_rng(1), average=False, **KW)
        assert a == b, fn.__name__
    Ga = mv.sq_gaussian_forces(Xd, 50.0, 0.25)
    Gb = mv.sq_gaussian_forces(Xd, 50.0, 0.25)
    assert torch.equal(Ga, Gb)
    Ea = mv.sq_gaussian_energies(Xd, 50.0, 0.25)
    assert torch.equal(Ea, mv.sq_gaussian_energies(Xd, 50.0, 0.25))


def test_fused_path_makes_one_kernel_pass():
    """The default method reduces every sample in one launch of the fused kernel (+ one slab reduction)."""
    X, F = _data(100, 10, 6)
    for fn, name in ((mv.random_force_proj, "gauss_proj_kernel"), (mv.random_residual_shift, "gauss_shift_kernel")):
        _lib.load().aggf_coverage_reset()
        fn(X, F, 1000, np.random.default_rng(0), **KW)
        hits = {k: v for k, v in _lib.coverage(names=True).items() if v[1]}
        fused = sum(v[1] for v in hits.values() if name in v[0])
        assert fused == 1, hits
        assert not any("gauss_site_forces_kernel" in v[0] for v in hits.values())
