"""Map validation under periodic boundaries on the GPU: the periodic forms of the K7 kernels (csrc/aggf_mapval.hip,
template argument PBC) through ``jaxmapval.random_force_proj`` / ``random_residual_shift`` with ``box=`` and the
``aggforce_amd.pbc`` functions.

1. Bit for bit against the open kernels on dyadic inputs: a trajectory whose sites were each moved by their own lattice
   vectors gives, under the box, exactly what the open kernels give on the unmoved one (the wrap recovers the unmoved
   displacement exactly in float32 and float64: tests/featpbc_cases.py).
2. Against the float64 restatement (tests/mapval_pbc_ref.py) on sites spread over the whole cell, with the tolerances of
   tests/test_gpu_mapval.py: 1e-11 (float64) or 1e-3 (float32) times the L1 scale of the summed terms.
3. The public calls.  4. A frame whose box is bad."""
import numpy as np
import pytest
import torch

import cell_ref
import mapval_pbc_ref as pref
import mapval_ref as ref
from featpbc_cases import dyadic_box
from pbc_ref import MARGIN
from aggforce_amd import _kernels as K
from aggforce_amd import _lib
from aggforce_amd import jaxmapval as mv
from aggforce_amd import pbc
from aggforce_amd.jaxutil import _as_box

pytestmark = pytest.mark.gpu

TOL = {np.float64: 1e-11, np.float32: 1e-3}
DYADIC_CELL = np.array([[8.0, 0, 0], [2.0, 8.0, 0], [-4.0, 2.0, 16.0]])
PAIRS = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_box(box, X):
    """What ``K.gauss_proj`` takes: the normalised box on X's device in X's dtype."""
    return _as_box(box, X.shape[0]).to(device=X.device, dtype=X.dtype).contiguous()


# ------------------------------------------------------------------ 1. bit for bit against the open kernels
def dyadic_case(T, n, kind, seed):
    """(X unmoved, X with every site moved by its own lattice vectors, F, box as the functions take it)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 512, size=(T, n, 3)) / 128.0
    F = rng.integers(-512, 512, size=(T, n, 3)) / 16.0
    k = rng.integers(-2, 3, size=(T, n, 3)).astype(np.float64)
    k[0, 0], k[-1, -1] = [2.0, -2.0, 1.0], [-2.0, 2.0, -2.0]  # (the extremes are there whatever the draw)
    if kind == "cell":
        return X, X + k @ DYADIC_CELL, F, pbc.Cell(DYADIC_CELL)
    box = dyadic_box(T, kind == "frames", rng)
    return X, X + k * (box[:, None, :] if box.ndim == 2 else box), F, box


# (7, 3): several frames per workgroup and per LDS stage, splits that cut frames; (2, 1100): past the LDS tile, one pair
DYADIC = [(T, n, kind, xd, fd) for T, n in ((7, 3), (7, 65)) for kind in ("box", "frames", "cell") for xd, fd in PAIRS]
DYADIC += [(2, 1100, kind, np.float32, np.float64) for kind in ("box", "frames", "cell")]


@pytest.mark.parametrize("T,n,kind,xd,fd", DYADIC)
def test_periodic_kernels_equal_the_open_kernels_bit_for_bit_on_moved_dyadic_sites(T, n, kind, xd, fd):
    X0, X1, F, box = dyadic_case(T, n, kind, 100 * n + T)
    assert np.abs(X1 - X0).max() >= 16.0
    Xo, Xm, Fd = dev(X0.astype(xd)), dev(X1.astype(xd)), dev(F.astype(fd))
    assert torch.equal(Xo.double().cpu(), torch.from_numpy(X0)) and torch.equal(Xm.double().cpu(), torch.from_numpy(X1))
    b = device_box(box, Xm)
    width = 4.0
    for offset in (3.0, 17.5):
        G, E = pbc.sq_gaussian_forces(Xm, offset, width, box), pbc.sq_gaussian_energies(Xm, offset, width, box)
        assert torch.equal(G, mv.sq_gaussian_forces(Xo, offset, width)), (offset, "forces")
        assert torch.equal(E, mv.sq_gaussian_energies(Xo, offset, width)), (offset, "energies")
        assert bool(torch.isfinite(G).all()) and float(G.abs().max()) > 0
    for S in (1, 37, 1030):  # 1030: two offset chunks
        o = dev(np.random.default_rng(S).uniform(1.0, 30.0, S))
        assert torch.equal(K.gauss_proj(Xm, Fd, o, width, box=b), K.gauss_proj(Xo, Fd, o, width)), S
        ip, gsq = K.gauss_shift(Xm, Fd, o, width, box=b)
        ip0, gsq0 = K.gauss_shift(Xo, Fd, o, width)
        assert torch.equal(ip, ip0) and torch.equal(gsq, gsq0), S
        assert float(ip0.abs().max()) > 0 and float(gsq0.min()) > 0
    # the open kernels on the moved trajectory see other distances
    assert not torch.equal(mv.sq_gaussian_energies(Xm, 3.0, width), mv.sq_gaussian_energies(Xo, 3.0, width))


# ------------------------------------------------------------------ 2. against the restatement
KINDS = cell_ref.KINDS + ["box", "frames_box"]
T2, N2, INNER, WIDTH = 200, 10, 2.0, 0.5
_cases = {}


def spread_case(kind, dtype):
    """Tie-free sites uniform over the cell, forces, and the box -- as the functions take it and as the restatement
    does -- with every number as stored in ``dtype``; the references, computed once."""
    if (kind, dtype) in _cases:
        return _cases[kind, dtype]
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    stored = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    seed = KINDS.index(kind)
    if kind == "box":
        L = stored([10.0, 11.0, 12.5])
        H, box, rbox = np.diag(L), L, L
    elif kind == "frames_box":
        L = stored(np.array([10.0, 11.0, 12.5]) * (1 + 0.03 * np.random.default_rng(5).uniform(-1, 1, (T2, 3))))
        H, box, rbox = np.stack([np.diag(r) for r in L]), L, L
    else:
        H = stored(cell_ref.cell_of(kind, T2, seed))
        box, rbox = pbc.Cell(H), pref.Tri(H)
    Hf = np.broadcast_to(H, (T2, 3, 3))

    def make(k):
        return (np.einsum("tnk,tkj->tnj", np.random.default_rng(1000 * seed + k).random((T2, N2, 3)), Hf),)

    (X,), tie = cell_ref.tie_free_sites(make, lambda x: x[:, :, None, :] - x[:, None, :, :], H, tdt)
    assert tie > MARGIN[tdt]
    F = stored(30.0 * np.random.default_rng(seed).standard_normal((T2, N2, 3)))
    outer = min(5.0, cell_ref.safe_radius(H))
    kw = dict(inner=INNER, outer=outer, width=WIDTH)
    _, _, moved = pref.displacements(X, rbox)
    off = np.triu(np.ones((N2, N2), dtype=bool), 1)
    case = dict(X=X, F=F, box=box, rbox=rbox, kw=kw, moved=float(moved[:, off].mean()),
                proj=pref.random_force_proj(X, F, 37, 42, box=rbox, **kw),
                shift=pref.random_residual_shift(X, F, 37, 42, box=rbox, **kw))
    _cases[kind, dtype] = case
    return case


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", KINDS)
def test_periodic_map_validation_matches_the_restatement(kind, dtype):
    c = spread_case(kind, dtype)
    X, F, box, kw, tol = c["X"].astype(dtype), c["F"].astype(dtype), c["box"], c["kw"], TOL[dtype]
    print(f"{kind} {np.dtype(dtype).name}: {c['moved']:.3f} of the pairs have a nearer image, outer {kw['outer']:.4g}")
    assert c["moved"] >= 0.4
    floor = 1e-300 if dtype == np.float64 else 1e-30  # float32 exp2 results below the normal range lose bits
    offs, w = ref.offsets(42, 2, **kw)
    # One field, entry by entry.  A term is (x - o) g(x) d, and float32 forms x to a few 1e-7 of its size: a pair with
    # x within that of the offset has a term of relative error 1, and with width 0.25 on squared distances it can be
    # most of its site's L1 scale.  As in tests/test_gpu_mapval.py the narrow field is checked entry by entry in
    # float64, and float32 takes a medium width, under which many pairs share every entry; the fused sums below run
    # the narrow fields in both precisions.
    if dtype == np.float32:
        w = 5.0
    for offset in offs:
        G, E = pbc.sq_gaussian_forces(X, offset, w, box), pbc.sq_gaussian_energies(X, offset, w, box)
        assert isinstance(G, np.ndarray) and G.dtype == dtype and E.dtype == dtype and E.shape == (T2,)
        Gr, scale = pref.forces(c["X"], offset, w, c["rbox"], scale=True)
        Er = pref.literal_energies(c["X"], offset, w, c["rbox"])
        print(f"  forces {np.max(np.abs(G - Gr) / (scale + floor)):.3g}, energies {np.max(np.abs(E - Er) / Er):.3g} "
              f"of the scale (tolerance {tol:g})")
        assert scale.max() > 0
        assert np.all(np.abs(G - Gr) <= tol * scale + floor)
        assert np.all(np.abs(E - Er) <= tol * Er + floor)
    (Pr, Ps), (Rr, Rs) = c["proj"], c["shift"]
    assert Ps.max() > 0 and Rs.max() > 0  # the offsets met pairs
    P = np.array(mv.random_force_proj(X, F, 37, np.random.default_rng(42), average=False, box=box, **kw))
    R = np.array(mv.random_residual_shift(X, F, 37, np.random.default_rng(42), box=box, **kw))
    print(f"  proj {np.max(np.abs(P - Pr) / Ps):.3g}, shift {np.max(np.abs(R - Rr) / Rs):.3g} of the scale")
    assert np.all(np.abs(P - Pr) <= tol * Ps)
    assert np.all(np.abs(R - Rr) <= tol * Rs)
    # and the open functions measure something else on these sites
    Po = np.array(mv.random_force_proj(X, F, 37, np.random.default_rng(42), average=False, **kw))
    assert np.any(np.abs(Po - Pr) > tol * Ps)


# ------------------------------------------------------------------ 3. the public calls
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["skew", "frames_box"])
def test_public_calls_types_generic_loop_one_launch_and_repeatability(kind, dtype):
    c = spread_case(kind, dtype)
    X, F, box, kw, tol = c["X"].astype(dtype), c["F"].astype(dtype), c["box"], c["kw"], TOL[dtype]
    Xd, Fd = dev(X), dev(F)
    for fn, name, (want, scale) in ((mv.random_force_proj, "gauss_proj_kernel", c["proj"]),
                                    (mv.random_residual_shift, "gauss_shift_kernel", c["shift"])):
        _lib.load().aggf_coverage_reset()
        vals = fn(X, F, 37, np.random.default_rng(42), average=False, box=box, **kw)
        hits = {k: v for k, v in _lib.coverage(names=True).items() if v[1]}
        assert sum(v[1] for v in hits.values() if name in v[0]) == 1, hits  # one pass of the fused kernel
        assert not any("gauss_site_forces_kernel" in v[0] for v in hits.values())
        assert isinstance(vals, list) and len(vals) == 37 and all(isinstance(v, float) for v in vals)
        avg = fn(X, F, 37, np.random.default_rng(42), average=True, box=box, **kw)
        assert isinstance(avg, float) and abs(avg - want.mean()) <= tol * scale.mean()
        # device tensors in, and twice: bit-identical
        a = fn(Xd, Fd, 37, np.random.default_rng(42), average=False, box=box, **kw)
        assert a == vals and a == fn(Xd, Fd, 37, np.random.default_rng(42), average=False, box=box, **kw)
        # pbc.rsqpg_forces as the method is the fused path; a lambda around it is the generic loop over it
        assert fn(X, F, 37, np.random.default_rng(42), method=pbc.rsqpg_forces, average=False, box=box, **kw) == vals
        _lib.load().aggf_coverage_reset()
        loop = fn(Xd, Fd, 37, np.random.default_rng(42), average=False, box=box, **kw,
                  method=lambda coords, randg=None, **k: pbc.rsqpg_forces(coords, randg=randg, **k))
        hits = {k: v for k, v in _lib.coverage(names=True).items() if v[1]}
        assert sum(v[1] for v in hits.values() if "gauss_site_forces_kernel" in v[0]) == 37, hits
        assert np.all(np.abs(np.array(vals) - np.array(loop)) <= tol * scale), fn.__name__
    G = pbc.rsqpg_forces(Xd, randg=np.random.default_rng(1), box=box, **kw)
    assert G.is_cuda and G.dtype == Xd.dtype and G.shape == Xd.shape
    assert torch.equal(G, pbc.rsqpg_forces(Xd, randg=np.random.default_rng(1), box=box, **kw))
    offset = np.random.default_rng(1).random() * (kw["outer"] ** 2 - INNER**2) + INNER**2
    assert torch.equal(G, pbc.sq_gaussian_forces(Xd, offset, WIDTH**2, box))


# ------------------------------------------------------------------ 4. a frame whose box is bad
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("bad", [0.0, -3.0, float("nan"), float("inf")])
def test_a_bad_frame_is_nan_and_no_other_frame_is(bad, dtype):
    T, n, t_bad = 20, 8, 3
    rng = np.random.default_rng(12)
    L = np.array([10.0, 11.0, 12.5]) * (1 + 0.03 * rng.uniform(-1, 1, (T, 3)))
    X = (rng.random((T, n, 3)) * L[:, None, :]).astype(dtype)
    F = (30.0 * rng.standard_normal((T, n, 3))).astype(dtype)
    kw = dict(inner=2.0, outer=4.5, width=0.5)
    good = dev(L.astype(dtype))
    broken = good.clone()
    broken[t_bad, 1] = bad
    rows = torch.diag_embed(good).reshape(T, 9).clone()
    rows[:, 3] = 0.7  # bx: a cell on the GPU, taken as it is
    rows_bad = rows.clone()
    rows_bad[t_bad, 4 if np.isfinite(bad) else 6] = bad  # by not positive, or cx not finite
    tri, tri_broken = pbc.Cell(rows.reshape(T, 3, 3)), pbc.Cell(rows_bad.reshape(T, 3, 3))
    for ok_box, bad_box in ((good, broken), (tri, tri_broken)):
        G = pbc.sq_gaussian_forces(X, 9.0, 3.0, bad_box)
        E = pbc.sq_gaussian_energies(X, 9.0, 3.0, bad_box)
        assert np.all(np.isnan(G[t_bad])) and np.isnan(E[t_bad])
        keep = np.arange(T) != t_bad
        assert np.array_equal(G[keep], pbc.sq_gaussian_forces(X, 9.0, 3.0, ok_box)[keep])
        assert np.array_equal(E[keep], pbc.sq_gaussian_energies(X, 9.0, 3.0, ok_box)[keep])
        assert np.all(np.isfinite(G[keep])) and np.all(np.isfinite(E[keep]))
        for fn in (mv.random_force_proj, mv.random_residual_shift):
            vals = fn(X, F, 5, np.random.default_rng(0), average=False, box=bad_box, **kw)
            assert len(vals) == 5 and all(np.isnan(v) for v in vals), fn.__name__
            fine = fn(X, F, 5, np.random.default_rng(0), average=False, box=ok_box, **kw)
            opened = fn(X, F, 5, np.random.default_rng(0), average=False, **kw)
            assert all(np.isfinite(v) for v in fine) and fine != opened  # a box does not give the open result
