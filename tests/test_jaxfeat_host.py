"""qp.jaxfeat's array functions on CPU tensors (plain torch, no GPU): values against the float64 restatement of
tests/jaxfeat_ref.py, the g7 autodiff fixture, and the reference's signatures."""
import inspect

import numpy as np
import pytest
import torch

import jaxfeat_ref as ref
from conftest import cons_in_insertion_order

from aggforce_amd.constraints import reduce_constraint_sets
from aggforce_amd.map import smear_map
from aggforce_amd.qp import jaxfeat
from aggforce_amd.qp.jaxfeat import (channel_allocate, clipped_gauss, gaussian_dist_basis, gb_subfeat,  # noqa: F401
                                     gb_subfeat_jac)

F32, F64 = torch.float32, torch.float64
# float64 CPU: a few ulp of values <= 1; float32: exp and the subtraction of clip, each 2^-24 relative to 1
TOL = {F32: 1e-6, F64: 1e-14}


def test_all_lists_the_six_names():
    assert sorted(jaxfeat.__all__) == sorted(["gb_feat", "clipped_gauss", "gaussian_dist_basis", "channel_allocate",
                                              "gb_subfeat", "gb_subfeat_jac"])


def test_signatures_are_the_references():
    def sig(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]

    E, P, VK = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.VAR_KEYWORD
    assert sig(clipped_gauss) == [("inp", E, P), ("center", E, P), ("width", 1.0, P), ("clip", 1e-3, P)]
    assert sig(gaussian_dist_basis) == [("dists", E, P), ("outer", E, P), ("inner", 0, P), ("n_basis", 10, P),
                                        ("width", 1.0, P), ("dist_power", 0.5, P), ("clip", 1e-3, P)]
    assert sig(channel_allocate) == [("feats", E, P), ("channels", E, P), ("max_channels", E, P),
                                     ("jac_shape", False, P)]
    assert sig(gb_subfeat) == [("points", E, P), ("cg_points", E, P), ("channels", E, P), ("max_channels", E, P),
                               ("smear_mat", E, P), ("collapse", False, P), ("channelize", True, P), ("kwargs", E, VK)]
    assert sig(gb_subfeat_jac) == [("points", E, P), ("cg_points", E, P), ("channels", E, P), ("max_channels", E, P),
                                   ("smear_mat", None, P), ("method", "reorder", P), ("kwargs", E, VK)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("clip", [1e-3, None], ids=["clip", "noclip"])
def test_clipped_gauss_and_basis_values(dtype, clip):
    rng = np.random.default_rng(3)
    r = torch.tensor(9 * rng.random((3, 4, 7)), dtype=dtype)
    rd = r.double().numpy()
    got = clipped_gauss(r, 2.5, width=0.8, clip=clip)
    assert got.dtype == dtype and got.shape == r.shape
    assert np.max(np.abs(got.double().numpy() - ref.basis(rd, [2.5], 0.8, clip)[..., 0])) <= TOL[dtype]
    for n_basis, power, inner in ((10, 0.5, 0.0), (1, 0.5, 1.5), (4, 1.0, 1.0), (3, 2.0, 0.5)):
        got = gaussian_dist_basis(r, 8.0, inner=inner, n_basis=n_basis, width=1.3, dist_power=power, clip=clip)
        assert got.dtype == dtype and got.shape == r.shape + (n_basis,)
        cen = ref.centers(8.0, inner, n_basis, power, np.float32 if dtype == F32 else np.float64)
        assert np.max(np.abs(got.double().numpy() - ref.basis(rd, cen, 1.3, clip))) <= TOL[dtype]
    # defaults, NumPy in -> tensor out
    got = gaussian_dist_basis(rd, 8.0)
    assert isinstance(got, torch.Tensor) and got.dtype == F64
    assert np.max(np.abs(got.numpy() - ref.basis(rd, ref.centers(8.0), 1.0, 1e-3))) <= TOL[F64]


def test_basis_gradient_on_cpu_is_the_hermite_form():
    rng = np.random.default_rng(4)
    r = torch.tensor(6 * rng.random((2, 5)), dtype=F64, requires_grad=True)
    out = gaussian_dist_basis(r, 6.0, n_basis=4, width=0.9)
    h = torch.tensor(rng.standard_normal(out.shape))
    (g,) = torch.autograd.grad((out * h).sum(), r)
    want = (ref.basis(r.detach().numpy(), ref.centers(6.0, 0, 4), 0.9, 1e-3, 1) * h.numpy()).sum(-1)
    assert np.max(np.abs(g.numpy() - want)) < 1e-13


CHANNELS = (3, 0, 5, 0, 2, 6, 3)  # non-consecutive, repeated, one equal to max_channels = 6 (dropped)


def test_channel_allocate_both_layouts():
    rng = np.random.default_rng(5)
    feats = rng.standard_normal((4, 7, 3))
    got = channel_allocate(torch.tensor(feats), CHANNELS, 6)
    want = ref.channel_allocate(feats, CHANNELS, 6)
    assert got.shape == (4, 7, 18) and np.array_equal(got.numpy(), want)
    assert not got.numpy()[:, 5].any()                       # channel == max_channels: nothing
    assert np.array_equal(got.numpy()[:, 2, 15:18], feats[:, 2])
    jac = rng.standard_normal((3, 4, 7, 2))
    got = channel_allocate(torch.tensor(jac), CHANNELS, 6, jac_shape=True)
    assert got.shape == (18, 4, 7, 2) and np.array_equal(got.numpy(), ref.channel_allocate(jac, CHANNELS, 6, True))
    # float32 stays float32; max(channels) as max_channels drops the last label
    got = channel_allocate(torch.tensor(feats, dtype=F32), CHANNELS, max(CHANNELS))
    assert got.dtype == F32 and got.shape == (4, 7, 18)


def test_channel_allocate_passes_gradients():
    rng = np.random.default_rng(6)
    feats = torch.tensor(rng.standard_normal((2, 7, 3)), requires_grad=True)
    h = torch.tensor(rng.standard_normal((2, 7, 18)))
    (g,) = torch.autograd.grad((channel_allocate(feats, CHANNELS, 6) * h).sum(), feats)
    want = np.zeros((2, 7, 3))
    for site, ch in enumerate(CHANNELS):
        if ch < 6:
            want[:, site] = h.numpy()[:, site, 3 * ch:3 * ch + 3]
    assert np.array_equal(g.numpy(), want)
    jac = torch.tensor(rng.standard_normal((3, 2, 7, 2)), requires_grad=True)
    (g,) = torch.autograd.grad(channel_allocate(jac, CHANNELS, 6, jac_shape=True).sum(), jac)
    want = np.ones((3, 2, 7, 2))
    want[:, :, 5] = 0
    assert np.array_equal(g.numpy(), want)


def g7_cases(g):
    """(name, coords, cmat, ids, smear matrix or None, basis kwargs) of the fixture's cases."""
    for name in [str(n) for n in g["names"]]:
        outer, inner, n_basis, width, dist_power = g[f"{name}__kw"]
        coords, cmat, ids = g[f"{name}__coords"], g[f"{name}__cmat"], g[f"{name}__ids"]
        cons = cons_in_insertion_order(g[f"{name}__cons"])
        smear = smear_map(reduce_constraint_sets(cons), coords.shape[1], return_mapping_matrix=True) if cons else None
        kw = dict(outer=float(outer), inner=float(inner), n_basis=int(n_basis), width=float(width),
                  dist_power=float(dist_power))
        yield name, coords, cmat, tuple(int(i) for i in ids), smear, kw


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_g7_features_from_cpu_tensors(golden, dtype):
    """gaussian_dist_basis + channel_allocate on CPU tensors reproduce the autodiff fixture's features (smeared points
    and distances formed with NumPy here), to the bound tests/test_oracle_golden.py uses for it."""
    g = golden("g7_gbfeat_autodiff.npz")
    n_cases = 0
    for name, coords, cmat, ids, smear, kw in g7_cases(g):
        c64 = coords.astype(np.float64)
        cg = np.einsum("cf,tfd->tcd", cmat, c64)
        for c in range(cmat.shape[0]):
            _, _, r = ref.site_distances(c64, cg[:, c:c + 1], smear)
            basis = gaussian_dist_basis(torch.tensor(r, dtype=dtype), **kw)
            feats = channel_allocate(basis, ids, max(ids))
            want = g[f"{name}__feats"][c]
            assert feats.shape == want.shape == (coords.shape[0], coords.shape[1], kw["n_basis"] * max(ids))
            assert np.max(np.abs(feats.double().numpy() - want)) < 5e-6, (name, c)
        n_cases += 1
    assert n_cases == 4


def test_cpu_gb_subfeat_without_smearing_matches_the_restatement():
    """smear_mat=None keeps the whole composition on the CPU: features, their collapsed forms and both divergences."""
    rng = np.random.default_rng(8)
    pts, cg = 4 * rng.random((3, 7, 3)) + 1, 4 * rng.random((3, 2, 3)) + 1
    kw = dict(outer=5.0, n_basis=3, width=1.1)
    cen = ref.centers(5.0, 0, 3)
    for collapse in (False, True):
        for channelize in (False, True):
            got = gb_subfeat(torch.tensor(pts), torch.tensor(cg), CHANNELS, 6, None, collapse=collapse,
                             channelize=channelize, **kw)
            want = ref.gb_subfeat(pts, cg, CHANNELS, 6, None, cen, 1.1, 1e-3, collapse, channelize)
            assert got.shape == want.shape and np.max(np.abs(got.numpy() - want)) < 1e-13
    got = gb_subfeat(torch.tensor(pts[0]), torch.tensor(cg[:1]), CHANNELS, 6, None, **kw)
    assert got.shape == (7, 18)
    assert np.max(np.abs(got.numpy() - ref.gb_subfeat(pts[:1], cg[:1], CHANNELS, 6, None, cen, 1.1)[0])) < 1e-13
    for method in ("reorder", "basic"):
        got = gb_subfeat_jac(torch.tensor(pts), torch.tensor(cg), CHANNELS, 6, None, method=method, **kw)
        want = ref.gb_subfeat_jac(pts, cg, CHANNELS, 6, None, cen, 1.1, 1e-3, method)
        assert got.shape == (3, 18, 3) and np.max(np.abs(got.numpy() - want)) < 1e-13
    with pytest.raises(ValueError, match="Unknown method"):
        gb_subfeat_jac(torch.tensor(pts), torch.tensor(cg), CHANNELS, 6, None, method="other", **kw)
