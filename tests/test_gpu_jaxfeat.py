"""qp.jaxfeat's array functions on the GPU (K10, aggforce_amd/_autograd.py: Basis / BasisDot): every kernel
instantiation against the float64 restatement of tests/jaxfeat_ref.py, special values, gradcheck / gradgradcheck, the
g7 autodiff fixture through gb_subfeat / gb_subfeat_jac, the two divergence methods against torch's own Jacobians, the
collapsed form's memory, determinism, and a hand-written featuriser through qp_feat_linear_map."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jaxfeat_ref as ref  # noqa: E402
from test_jaxfeat_host import g7_cases  # noqa: E402

from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd import _lib  # noqa: E402
from aggforce_amd.qp import jaxfeat  # noqa: E402
from aggforce_amd.qp.jaxfeat import (channel_allocate, clipped_gauss, gaussian_dist_basis, gb_subfeat,  # noqa: E402
                                     gb_subfeat_jac)

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
TOL = {F32: 2e-5, F64: 1e-12}  # (tests/test_gpu_distances.py)
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-5)  # (tests/test_gpu_distances.py)
NP_OF = {F32: np.float32, F64: np.float64}


def dev(a, dtype=F64, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=grad)


def host(t):
    return t.detach().cpu().double().numpy()


def close(got, want, tol, what, skip=None):
    """|got - want| <= tol * max|want| on every element (but those of ``skip``: at most 0.1 %)."""
    got = host(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return
    err = np.abs(got - want)
    if skip is not None:
        assert skip.shape == want.shape and skip.mean() <= 1e-3, (what, float(skip.mean()))
        err = np.where(skip, 0.0, err)
    scale = max(float(np.max(np.abs(want))), 1e-300)
    worst = float(np.max(err)) / (tol * scale)
    print(f"{what}: error {worst:.3g} x the {tol:g} bound")
    assert worst <= 1.0, f"{what}: error {worst:.3g} x the {tol:g} bound"


def launched():
    torch.cuda.synchronize()
    return sorted(p.split("(")[0].replace("void aggf::", "") for p, c in _lib.coverage(names=True).values() if c > 0)


def reset():
    torch.cuda.synchronize()
    _lib.load().aggf_coverage_reset()


def make_spec(dtype, n_basis, clip, channels=None, n_slots=None, width=1.3):
    cen = ref.centers(8.0, 0.5, n_basis, 0.5, NP_OF[dtype])
    return K.BasisSpec(dev(cen, dtype), width, clip, channels, n_slots), cen


# ------------------------------------------------------------------ 1. every K10 instantiation vs the restatement
# K9's odd sizes: one element, neither a multiple of 64 nor of a panel; the last axis is the site axis of the slotted forms
D_SHAPES = [(1, 1, 1), (3, 5, 67), (2, 65, 257)]


def dists_of(shape, dtype, seed, view=False):
    """Distances in [0, 9): beyond both ends of the grid [0.5, 8].  ``view``: a non-contiguous view of a wider array."""
    rng = np.random.default_rng(seed)
    if not view:
        return dev(9 * rng.random(shape), dtype)
    wide = dev(9 * rng.random(shape[:-1] + (2 * shape[-1] + 1,)), dtype)
    return wide[..., 1::2]


def site_channels(n_sites, n_slots):
    """Slots 0..n_slots-1 but slot 1 (left empty), and every fifth site dropped (channel == n_slots)."""
    ch = np.arange(n_sites) % n_slots
    ch[ch == 1] = 0
    ch[::5] = n_slots
    return tuple(int(c) for c in ch)


CASES = [(shape, False) for shape in D_SHAPES] + [((3, 5, 67), True)]


@pytest.mark.parametrize("q", [0, 1, 2, 3])
@pytest.mark.parametrize("n_basis", [1, 3, 10, 17])
@pytest.mark.parametrize("clip", [1e-3, None], ids=["clip", "noclip"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_k10_every_kernel_matches_the_restatement(dtype, clip, n_basis, q):
    k = "float" if dtype == F32 else "double"
    tol = TOL[dtype]
    for case, (shape, view) in enumerate(CASES):
        seed = 7000 + 100 * case + 10 * q + n_basis
        d = dists_of(shape, dtype, seed, view)
        assert d.is_contiguous() != view
        dc, r = d.contiguous(), host(d)
        rng = np.random.default_rng(seed + 1)
        s = dev(rng.standard_normal(shape), dtype)
        n_sites, n_slots = shape[-1], 4
        channels = site_channels(n_sites, n_slots)
        plain, cen = make_spec(dtype, n_basis, clip)
        slotted, _ = make_spec(dtype, n_basis, clip, channels, n_slots)
        # float32, q >= 1: an element whose exp(-z^2) lies within 1e-5 clip of the clip may take the other branch
        flip = ref.near_clip(r, cen, 1.3, clip) if dtype == F32 and q > 0 else None
        flip_row = None
        if flip is not None:
            flip_row = ref.channel_allocate(flip.reshape((-1,) + flip.shape[-2:]), channels, n_slots).reshape(
                flip.shape[:-1] + (-1,))
        # K10a: unscaled, scaled, slotted (an empty slot, dropped sites)
        reset()
        e0 = K.gbasis_expand(dc, plain, q)
        e1 = K.gbasis_expand(dc, plain, q, s)
        e2 = K.gbasis_expand(dc, slotted, q, s)
        assert launched() == [f"gb_expand_kernel<{k}, false>", f"gb_expand_kernel<{k}, true>"]
        close(e0, ref.expand(r, cen, 1.3, clip, q), tol, f"expand {shape}", flip)
        close(e1, ref.expand(r, cen, 1.3, clip, q, host(s)), tol, f"scaled expand {shape}", flip)
        want = ref.expand(r, cen, 1.3, clip, q, host(s), channels, n_slots)
        close(e2, want, tol, f"slotted expand {shape}", flip_row)
        blocks = host(e2).reshape(-1, n_sites, n_slots, n_basis)
        assert not blocks[:, :, 1].any() and not blocks[:, ::5].any()  # exact zeros: the empty slot, the dropped sites
        # K10b: the three forms of H.  An element whose branch may flip is left out as a whole.
        g = ref.basis(r, cen, 1.3, clip, q)
        flip_e = None if flip is None else flip.any(-1)
        h_elem = dev(rng.standard_normal(shape + (n_basis,)), dtype)
        h_row = dev(rng.standard_normal(shape + (n_slots * n_basis,)), dtype)
        h_slot = dev(rng.standard_normal((n_slots, n_basis)), dtype)
        reset()
        c0 = K.gbasis_contract(h_elem, dc, plain, q, K.GB_H_ELEM)
        c1 = K.gbasis_contract(h_row, dc, slotted, q, K.GB_H_ROW)
        c2 = K.gbasis_contract(h_slot, dc, slotted, q, K.GB_H_SLOT)
        assert launched() == [f"gb_contract_kernel<{k}, {form}>" for form in (0, 1, 2)]
        close(c0, (host(h_elem) * g).sum(-1), tol, f"contract, H per element {shape}", flip_e)
        ch = np.asarray(channels)
        kept = ch < n_slots
        col = np.where(kept, ch, 0)[:, None] * n_basis + np.arange(n_basis)[None, :]       # (n_sites, n_basis)
        picked = np.take_along_axis(host(h_row), np.broadcast_to(col, shape + (n_basis,)), axis=-1)
        close(c1, np.where(kept, (picked * g).sum(-1), 0.0), tol, f"contract, H in slotted rows {shape}", flip_e)
        close(c2, np.where(kept, (host(h_slot)[np.where(kept, ch, 0)] * g).sum(-1), 0.0), tol,
              f"contract, H per slot {shape}", flip_e)
        # K10c: the scaled sum per slot, and one slot of everything
        reset()
        s0 = K.gbasis_sum(dc, slotted, q, s)
        s1 = K.gbasis_sum(dc, plain, q)
        assert launched() == [f"gb_chansum_kernel<{k}>", f"gb_chansum_reduce_kernel<{k}>"]
        terms = g * host(s)[..., None]
        per_site = terms.reshape(-1, n_sites, n_basis).sum(0)
        want = np.stack([per_site[ch == sl].sum(0) for sl in range(n_slots)])
        want1 = g.reshape(-1, n_basis).sum(0)[None, :]
        if flip is not None and flip.any():  # the left-out elements' terms are taken out of both sides' difference
            jump = np.abs(np.where(flip, ref.basis(r, cen, 1.3, None, q), 0.0))
            slack = float((jump * np.abs(host(s))[..., None]).sum()), float(jump.sum())
        else:
            slack = 0.0, 0.0
        assert not host(s0)[1].any()
        for got, ref_sum, extra, what in ((s0, want, slack[0], "scaled sum per slot"), (s1, want1, slack[1], "sum")):
            err = float(np.max(np.abs(host(got) - ref_sum)))
            lim = tol * max(float(np.max(np.abs(ref_sum))), 1e-300) + extra
            print(f"{what} {shape}: error {err / lim:.3g} x the bound")
            assert host(got).shape == ref_sum.shape and err <= lim, (what, shape, err, lim)
        if q == 0:  # the public function on the same (possibly non-contiguous) tensor: the same launch
            assert torch.equal(gaussian_dist_basis(d, 8.0, 0.5, n_basis, 1.3, 0.5, clip), e0)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("T", [1, 1100])
def test_channel_sum_over_one_frame_and_over_more_frames_than_workgroups(dtype, T):
    """1100 frames: more than the 512 frame chunks, so a workgroup sums several frames and the second pass adds 367
    partials; one frame: one chunk.  Terms are non-negative (q = 0): the bound is TOL of the sum itself."""
    n_sites, n_slots, n_basis = 9, 5, 6
    channels = site_channels(n_sites, n_slots)
    spec, cen = make_spec(dtype, n_basis, 1e-3, channels, n_slots)
    d = dists_of((T, n_sites), dtype, 31 + T)
    got = K.gbasis_sum(d, spec, 0)
    per_site = ref.basis(host(d), cen, 1.3, 1e-3).sum(0)
    want = np.stack([per_site[np.asarray(channels) == sl].sum(0) for sl in range(n_slots)])
    close(got, want, TOL[dtype], f"channel sum, {T} frames")


# ------------------------------------------------------------------ 2. special values
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_special_values(dtype):
    kw = dict(outer=6.0, inner=1.0, n_basis=4, width=0.7, dist_power=1.0)
    # r = 0 and r far outside the grid: exact zeros with the clip, the plain values without
    r = dev([0.0, 1.0, 3.5, 40.0, 1e6], dtype, grad=True)
    out = gaussian_dist_basis(r, **kw)
    want = ref.basis(host(r), ref.centers(6.0, 1.0, 4, 1.0, NP_OF[dtype]), 0.7, 1e-3)
    close(out, want, TOL[dtype], "values at 0 and far outside")
    assert not host(out)[3:].any() and host(out)[1, 0] == pytest.approx(1 - 1e-3)
    (g,) = torch.autograd.grad(out.sum(), r)
    assert not host(g)[3:].any() and np.isfinite(host(g)).all()
    # NaN and infinities propagate as in the plain-torch body of the same function
    bad = dev([np.nan, np.inf, -np.inf, 2.0], dtype)
    for clip in (1e-3, None):
        got = gaussian_dist_basis(bad, clip=clip, **kw)
        plain = jaxfeat._plain_basis(bad, jaxfeat._grid(dtype, 6.0, 1.0, 4, 1.0), 0.7, clip)
        assert torch.isnan(got[0]).all() and not torch.isnan(got[1:]).any()
        assert torch.allclose(got, plain, rtol=TOL[dtype], atol=TOL[dtype], equal_nan=True)
        one = clipped_gauss(bad, 2.0, width=0.7, clip=clip)
        assert torch.allclose(one, jaxfeat._plain_basis(bad, (2.0,), 0.7, clip)[..., 0], rtol=TOL[dtype],
                              atol=TOL[dtype], equal_nan=True)
    # a site on top of the cg site: weight 0 in the divergence and in every gradient, nothing non-finite
    pts = dev([[[1.0, 2.0, 3.0], [2.0, 2.0, 3.0], [1.0, 4.0, 3.5]]], dtype, grad=True)
    cg = pts.detach()[:, :1].clone()
    div = gb_subfeat_jac(pts, cg, (0, 1, 0), 2, None, outer=3.0, n_basis=3)
    feats = gb_subfeat(pts, cg, (0, 1, 0), 2, None, outer=3.0, n_basis=3)
    (g,) = torch.autograd.grad(feats.sum() + (div**2).sum(), pts)
    assert np.isfinite(host(div)).all() and np.isfinite(host(g)).all() and not host(g)[0, 0].any()


# ------------------------------------------------------------------ 3. gradcheck / gradgradcheck (float64)
def clip_margin(r, cen, width, clip=1e-3):
    """Smallest distance of any r to a point where some exp(-z^2) crosses the clip."""
    edge = width * np.sqrt(np.log(1 / clip))
    r, cen = np.asarray(r, dtype=np.float64), np.asarray(cen, dtype=np.float64)
    return float(np.min(np.abs(np.abs(r[..., None] - cen) - edge)))


def test_basis_gradcheck_and_gradgradcheck():
    """Inputs at least 1e-3 from the clip boundary of every centre (a finite difference of step 1e-6 must not straddle
    the kink), which the test asserts of its own draw."""
    rng = np.random.default_rng(11)
    r = 5 * rng.random((2, 3, 5)) + 0.2
    kw = dict(outer=5.0, n_basis=4, width=0.8)
    assert clip_margin(r, ref.centers(5.0, 0, 4), 0.8) >= 1e-3
    x = dev(r, grad=True)

    def fn(d):
        return gaussian_dist_basis(d, **kw)

    assert torch.autograd.gradcheck(fn, (x,), **GC)
    assert torch.autograd.gradgradcheck(fn, (x,), **GC)
    assert torch.autograd.gradcheck(lambda d: clipped_gauss(d, 2.0, 0.8), (x,), **GC)


SUB_CHANNELS = (0, 1, 1, 2, 3, 0)  # max_channels = 3: the last label is dropped


def subfeat_inputs():
    rng = np.random.default_rng(12)
    pts = 3 * rng.random((2, 6, 3)) + 1
    cg = 3 * rng.random((2, 2, 3)) + 1
    smear = np.eye(6) + 0.15 * rng.standard_normal((6, 6))
    return pts, cg, smear


@pytest.mark.parametrize("collapse", [False, True], ids=["full", "collapse"])
@pytest.mark.parametrize("channelize", [False, True], ids=["bins", "channels"])
def test_gb_subfeat_gradcheck_and_gradgradcheck(collapse, channelize):
    """In points, cg_points and smear_mat at T = 2, N = 6, n_basis = 3.  The smeared distances of the draw stay 1e-3
    away from every clip boundary and from zero (asserted)."""
    pts, cg, smear = subfeat_inputs()
    kw = dict(outer=4.0, n_basis=3, width=0.9)
    _, _, r = ref.site_distances(pts, cg, smear)
    assert clip_margin(r, ref.centers(4.0, 0, 3), 0.9) >= 1e-3 and r.min() > 0.1
    x, c, s = dev(pts, grad=True), dev(cg, grad=True), dev(smear, grad=True)

    def fn(p, g, m):
        return gb_subfeat(p, g, SUB_CHANNELS, 3, m, collapse=collapse, channelize=channelize, **kw)

    want = ref.gb_subfeat(pts, cg, SUB_CHANNELS, 3, smear, ref.centers(4.0, 0, 3), 0.9, 1e-3, collapse, channelize)
    close(fn(x, c, s), want, TOL[F64], "gb_subfeat")
    assert torch.autograd.gradcheck(fn, (x, c, s), **GC)
    assert torch.autograd.gradgradcheck(fn, (x, c, s), **GC)


# ------------------------------------------------------------------ 4. the g7 fixture on the device
def test_g7_through_gb_subfeat_and_gb_subfeat_jac(golden):
    """Features and both divergences of every site of the four cases, with the fixture's labels and max(ids) channels,
    to the bounds tests/test_gpu_feat.py uses for this fixture; gb_feat's own arrays agree to the same bounds."""
    from aggforce_amd import LinearMap
    from aggforce_amd.qp import gb_feat

    from conftest import cons_in_insertion_order

    g = golden("g7_gbfeat_autodiff.npz")
    for name, coords, cmat, ids, smear, kw in g7_cases(g):
        pts = dev(coords, F32)
        cg = torch.einsum("cf,tfd->tcd", dev(cmat, F32), pts)
        cons = cons_in_insertion_order(g[f"{name}__cons"])
        own = {m: gb_feat(coords, LinearMap(cmat), cons, lazy=False, div_method=m, **kw) for m in ("reorder", "basic")}
        for c in range(cmat.shape[0]):
            site = cg[:, c:c + 1, :]
            feats = gb_subfeat(pts, site, ids, max(ids), smear, **kw)
            want = g[f"{name}__feats"][c]
            assert feats.dtype == F32 and tuple(feats.shape) == want.shape
            assert np.max(np.abs(host(feats) - want)) < 5e-6, (name, c)
            assert np.max(np.abs(host(feats) - own["reorder"]["feats"][c])) < 5e-6, (name, c)
            for method, key in (("reorder", "divs"), ("basic", "divs_basic")):
                div = gb_subfeat_jac(pts, site, ids, max(ids), smear, method=method, **kw)
                want = g[f"{name}__{key}"][c]
                assert tuple(div.shape) == want.shape
                assert np.max(np.abs(host(div) - want)) < 1e-4, (name, c, method)
                assert np.max(np.abs(host(div) - own[method]["divs"][c])) < 1e-4, (name, c, method)


# ------------------------------------------------------------------ 5. the two divergence methods
def test_divergence_methods_match_their_jacobians_and_differ():
    """A non-symmetric smear matrix separates the two methods: "basic" is the Jacobian of the channelised collapsed
    features, "reorder" the Jacobian before channelising put through channel_allocate -- both summed over the sites."""
    rng = np.random.default_rng(21)
    T, N = 3, 7
    channels, mc = (2, 0, 1, 0, 3, 2, 1), 3
    pts, cg = dev(3 * rng.random((T, N, 3)) + 1), dev(3 * rng.random((T, 1, 3)) + 1)
    smear = dev(np.eye(N) + 0.3 * rng.random((N, N)))
    kw = dict(outer=4.0, n_basis=3, width=1.2)
    jacobian = torch.autograd.functional.jacobian
    jac = jacobian(lambda x: gb_subfeat(x, cg, channels, mc, smear, collapse=True, **kw), pts)
    basic = torch.swapaxes(jac.sum(dim=2), 0, 1)
    jac = jacobian(lambda x: gb_subfeat(x, cg, channels, mc, smear, collapse=True, channelize=False, **kw), pts)
    reorder = torch.swapaxes(channel_allocate(jac, channels, mc, jac_shape=True).sum(dim=2), 0, 1)
    got_b = gb_subfeat_jac(pts, cg, channels, mc, smear, method="basic", **kw)
    got_r = gb_subfeat_jac(pts, cg, channels, mc, smear, method="reorder", **kw)
    assert float((got_b - basic).abs().max()) < 1e-10
    assert float((got_r - reorder).abs().max()) < 1e-10
    assert float((got_b - got_r).abs().max()) > 1e-3
    cen = ref.centers(4.0, 0, 3)
    for got, method in ((got_b, "basic"), (got_r, "reorder")):
        want = ref.gb_subfeat_jac(host(pts), host(cg), channels, mc, host(smear), cen, 1.2, 1e-3, method)
        assert np.max(np.abs(host(got) - want)) < 1e-10


# ------------------------------------------------------------------ 6. no one-hot array
def test_collapsed_form_never_builds_the_one_hot_array():
    """T = 2000, N = 64, 64 channels, n_basis = 8, float32: the one-hot array would be 262 MB against 1.5 MB of
    coordinates; forward and backward of the collapsed form stay under 16 MB of new allocations."""
    rng = np.random.default_rng(22)
    T, N, nb = 2000, 64, 8
    channels = tuple(range(N))
    pts = dev(6 * rng.random((T, N, 3)), F32, grad=True)
    cg = dev(6 * rng.random((T, 1, 3)), F32)
    smear = dev(np.eye(N) + 0.01 * rng.random((N, N)), F32)
    h = dev(rng.standard_normal(N * nb), F32)
    kw = dict(outer=8.0, n_basis=nb)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = gb_subfeat(pts, cg, channels, N, smear, collapse=True, **kw)
    (grad,) = torch.autograd.grad((out * h).sum(), pts)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak allocation rose by {rise / 2**20:.2f} MiB")
    assert rise < 16 * 2**20
    assert out.shape == (N * nb,) and grad.shape == pts.shape
    full = gb_subfeat(pts, cg, channels, N, smear, **kw)
    assert full.shape == (T, N, N * nb)
    close(out, host(full.double().sum(dim=(0, 1))), TOL[F32], "collapsed vs summed")
    (grad_full,) = torch.autograd.grad((full.double().sum(dim=(0, 1)) * h.double()).sum(), pts)
    close(grad, host(grad_full), TOL[F32], "gradient of the collapsed form")


# ------------------------------------------------------------------ 7. determinism
def test_channel_sum_and_backward_are_bit_identical_run_to_run():
    rng = np.random.default_rng(23)
    T, N = 700, 33
    channels = site_channels(N, 6)
    pts_np, cg_np = 6 * rng.random((T, N, 3)), 6 * rng.random((T, 1, 3))
    h = dev(rng.standard_normal(6 * 5), F32)
    runs = []
    for _ in range(2):
        pts, cg = dev(pts_np, F32, grad=True), dev(cg_np, F32, grad=True)
        out = gb_subfeat(pts, cg, channels, 6, None, collapse=True, outer=8.0, n_basis=5)
        gp, gc = torch.autograd.grad((out * h).sum(), (pts, cg))
        runs.append((out.detach().clone(), gp.clone(), gc.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 8. a hand-written featuriser, end to end
def test_hand_written_featuriser_fits_as_gb_feat_does(golden):
    """The general protocol of qp_feat_linear_map fed from gb_subfeat / gb_subfeat_jac gives the mapped forces of the
    built-in gb_feat, to the float32 bound of tests/test_gpu_contract.py's generic-featuriser test."""
    from aggforce_amd import LinearMap, Trajectory
    from aggforce_amd.constraints import reduce_constraint_sets
    from aggforce_amd.map import smear_map
    from aggforce_amd.qp import gb_feat, id_feat, qp_feat_linear_map
    from aggforce_amd.util import Curry

    from conftest import cons_in_insertion_order

    g = golden("g7_gbfeat_autodiff.npz")
    coords, cmat = g["groups__coords"], g["groups__cmat"]
    cons = cons_in_insertion_order(g["groups__cons"])
    kw = dict(outer=8.0, n_basis=5)

    def featuriser(points, cmap, constraints):
        ids = tuple(int(i) for i in id_feat(points, cmap, constraints, return_ids=True))
        smear = smear_map(reduce_constraint_sets(constraints), cmap.n_fg_sites, return_mapping_matrix=True)
        pts = dev(points, F32)
        sites = [dev(cmap(points), F32)[:, c:c + 1] for c in range(cmap.n_cg_sites)]
        return {"feats": [gb_subfeat(pts, s, ids, max(ids), smear, **kw).cpu().numpy() for s in sites],
                "divs": [gb_subfeat_jac(pts, s, ids, max(ids), smear, **kw).cpu().numpy() for s in sites],
                "names": None}

    rng = np.random.default_rng(24)
    forces = (20 * rng.standard_normal(coords.shape)).astype(np.float32)
    traj, cmap = Trajectory(coords=coords, forces=forces), LinearMap(cmat)
    frames = [rng.choice(coords.shape[0], size=1, replace=False) for _ in range(cmat.shape[0])]
    fits = [qp_feat_linear_map(traj, cmap, f, 0.6955215, constraints=cons, frame_indices=frames, l2_regularization=10.0)
            for f in (featuriser, Curry(gb_feat, **kw))]
    mine, builtin = (np.asarray(tm(traj).forces, dtype=np.float64) for tm in fits)
    err = float(np.max(np.abs(mine - builtin)) / np.max(np.abs(builtin)))
    print(f"mapped forces differ by {err:.3g} (relative)")
    assert err < 1e-3
