"""CPU: argument handling of the periodic-box forms of gb_feat and its kernels' wrappers, and the constructions that
tests/test_gpu_feat_pbc.py rests on (tests/featpbc_cases.py) checked in NumPy float32.  Nothing here launches a
kernel: every refusal asked for comes before any device work."""
import numpy as np
import pytest
import torch

import featpbc_cases as cases
from aggforce_amd import LinearMap, Trajectory
from aggforce_amd.agg import project_forces_grid_cv
from aggforce_amd import _kernels as K
from aggforce_amd.qp import Multifeaturize, gb_feat, id_feat, qp_feat_linear_map
from aggforce_amd.qp import gbfeat
from aggforce_amd.qp.jaxfeat import gb_subfeat, gb_subfeat_jac
from aggforce_amd.util import Curry
from oracle import aggforce_oracle as orc


def small():
    rng = np.random.default_rng(0)
    coords = (4 * rng.random((6, 8, 3))).astype(np.float32)
    forces = rng.standard_normal((6, 8, 3)).astype(np.float32)
    cmap = LinearMap(orc.list_mapping_matrix([[0, 1], [4, 7]], 8))
    return coords, forces, cmap, {frozenset([1, 2])}


# ------------------------------------------------------------------ the constructions


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dyadic_shifts_are_exact_and_never_on_a_tie(per_frame, dtype):
    """The kernels' wrap, in NumPy arithmetic of the kernels' dtype, takes the shifted displacement back to the
    unshifted one bit for bit; no component of an unshifted displacement reaches half a box length."""
    Pg, cg, box, Pg_s = cases.dyadic_groups(7, 20, 3, per_frame, seed=5)
    for a in (Pg, cg, box, Pg_s):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)  # float32 holds every input exactly
    rows = box[:, None, None, :] if per_frame else box[None, None, None, :]
    d0 = (Pg[:, None].astype(dtype) - cg[:, :, None].astype(dtype))
    ds = (Pg_s[:, None].astype(dtype) - cg[:, :, None].astype(dtype))
    assert np.all(np.abs(d0) < rows / 2) and np.all(np.abs(d0).sum(axis=-1) > 0)
    assert not np.array_equal(ds, d0) and np.abs((ds - d0) / rows).max() == 2.0
    got = cases.min_image(ds, np.broadcast_to(rows, ds.shape), dtype)
    assert got.dtype == dtype and np.array_equal(got, d0)
    if per_frame:
        assert len({tuple(r) for r in box}) > 3 and all(len(set(r)) > 1 for r in box[:2])
    else:
        assert len(set(box)) == 3


@pytest.mark.parametrize("per_frame", [False, True])
def test_random_groups_have_many_nearer_images_and_few_ties(per_frame):
    for G, seed in ((20, 11), (75, 12)):
        Pg, cg, box = cases.random_groups(7, G, 3, per_frame, seed)
        d_mi, share, near_tie = cases.image_statistics(Pg, cg, box)
        rows = box[:, None, None, :] if per_frame else box[None, None, None, :]
        assert share >= 0.25 and near_tie.mean() < 0.01
        assert np.all(np.abs(d_mi) <= rows / 2 + 1e-12)


@pytest.mark.parametrize("per_frame", [False, True])
def test_dyadic_molecules_wrap_splits_molecules_and_moves_keep_them(per_frame):
    U, forces, box, wrapped, moved = cases.dyadic_molecules(40, per_frame, seed=3)
    rows = box[:, None, :] if per_frame else box[None, None, :]
    for a in (U, wrapped, moved):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    assert np.all((wrapped >= 0) & (wrapped < rows))
    i, j = cases.BONDS[:, 0], cases.BONDS[:, 1]
    assert np.any(np.abs(wrapped[:, i] - wrapped[:, j]) > rows / 2)      # bonds through a face
    assert np.array_equal(moved[:, i] - moved[:, j], U[:, i] - U[:, j])   # whole molecules
    # group means and beads never coincide (r > 0), and open distances in `moved` are not those of U
    smear = orc.smear_matrix(orc.reduce_constraint_sets(cases.CONS), cases.N_ATOMS).astype(np.float64)
    cmat = orc.list_mapping_matrix(cases.BEADS, cases.N_ATOMS)
    p, c = np.einsum("tfd,cf->tcd", U, smear), np.einsum("tfd,cf->tcd", U, cmat)
    assert np.linalg.norm(p[:, None] - c[:, :, None], axis=-1).min() > 0
    pm, cm = np.einsum("tfd,cf->tcd", moved, smear), np.einsum("tfd,cf->tcd", moved, cmat)
    _, share, _ = cases.image_statistics(pm, cm, box)
    assert share >= 0.25


# ------------------------------------------------------------------ refusals


def test_gb_feat_refuses_a_bad_box_before_any_device_work(monkeypatch):
    coords, forces, cmap, cons = small()
    monkeypatch.setattr(K, "as_device", lambda *a, **k: pytest.fail("device work before the box was checked"))
    for bad in (np.ones(2), np.ones((5, 3)), np.ones((6, 2)), np.ones((1, 3)), "abc"):
        with pytest.raises(ValueError, match="box"):
            gb_feat(coords, cmap, cons, outer=6.0, box=bad)
    for bad in ([4.0, -1.0, 4.0], [4.0, 0.0, 4.0], [4.0, np.inf, 4.0], [np.nan, 4.0, 4.0]):
        with pytest.raises(ValueError, match="positive and finite"):
            gb_feat(coords, cmap, cons, outer=6.0, box=bad)
    with pytest.raises(ValueError, match="constant"):
        gb_feat(coords, cmap, cons, outer=6.0, box=torch.full((3,), 5.0, requires_grad=True))
    # the array functions normalise the box the same way
    for f in (gb_subfeat, gb_subfeat_jac):
        with pytest.raises(ValueError, match="box"):
            f(torch.from_numpy(coords), torch.from_numpy(coords[:, :1]), [0] * 8, 1, None, box=np.ones((5, 3)), outer=6.0)


def test_a_bound_box_is_still_recognised_by_the_fused_paths():
    box = np.array([5.0, 6.0, 7.0])
    gb = Curry(gb_feat, outer=6.0, n_basis=4, box=box)
    use_id, kw = gbfeat.recognise([id_feat, gb])
    assert use_id and kw["box"] is box
    feat = Multifeaturize([id_feat, gb])
    assert feat.fused_fit is not None and feat.fused_cv is not None
    assert gbfeat.bound_box(feat) is box and gbfeat.bound_box(gb) is box
    assert gbfeat.bound_box(Multifeaturize([id_feat])) is None and gbfeat.bound_box(id_feat) is None
    assert gbfeat.recognise([id_feat, Curry(gb_feat, outer=6.0, nonsense=1)]) is None


def test_a_per_frame_box_is_refused_under_comm_and_in_cross_validation(monkeypatch):
    coords, forces, cmap, cons = small()
    monkeypatch.setattr(K, "as_device", lambda *a, **k: pytest.fail("device work before the refusal"))
    per_frame = np.full((6, 3), 5.0)
    feat = Multifeaturize([id_feat, Curry(gb_feat, outer=6.0, n_basis=4, box=per_frame)])
    with pytest.raises(ValueError, match="per-frame box"):
        qp_feat_linear_map(Trajectory(coords=coords, forces=forces), cmap, feat, 0.6, constraints=cons, comm=object())
    with pytest.raises(ValueError, match="per-frame box"):
        gbfeat.cv_id_gb(coords, forces, cmap, 0.6, 2, cons, [1.0], [np.arange(3), np.arange(3, 6)], None, True,
                        dict(outer=6.0, box=per_frame))
    for reuse in (True, False):  # the one-pass form and the loop alike
        with pytest.raises(ValueError, match="per-frame box"):
            project_forces_grid_cv({"l2_regularization": [1.0, 10.0]}, coords, forces, n_folds=2, reuse_gram=reuse,
                                   coord_map=cmap, constrained_inds=cons, method=qp_feat_linear_map, featurizer=feat,
                                   kbt=0.6)
    with pytest.raises(ValueError, match="per-frame box"):  # a featuriser that is itself on the grid
        project_forces_grid_cv({"featurizer": [Multifeaturize([id_feat]), feat]}, coords, forces, n_folds=2,
                               coord_map=cmap, constrained_inds=cons, method=qp_feat_linear_map, kbt=0.6)


@pytest.mark.parametrize("name", ["gb_channels", "gb_regmat_cols", "gb_apply", "gb_apply_cols", "gb_distance_range"])
def test_kernel_wrappers_check_the_box_first(name, monkeypatch):
    """Dtype, device, contiguity and shape of the box (``_box_arg``) are checked before the library is touched."""
    monkeypatch.setattr(K, "lib", lambda: pytest.fail("library call before the box was checked"))
    T, G = 5, 4
    Pg, cg, Fg = torch.zeros((T, G, 3)), torch.zeros((T, 2, 3)), torch.zeros((T, G, 3))
    sizes, cen = torch.ones(G), torch.ones(3)
    R3 = torch.zeros((T, 128, 3))
    cols = torch.zeros(2, dtype=torch.int32)
    call = {
        "gb_channels": lambda b: K.gb_channels(Pg, cg, 0, sizes, G, cen, 1.0, 1e-3, box=b),
        "gb_regmat_cols": lambda b: K.gb_regmat_cols(Fg, Pg, cg, 0, sizes, G, cols, cen, 1.0, 1e-3, 0.6, R3, box=b),
        "gb_apply": lambda b: K.gb_apply(Fg, Pg, cg, sizes, G, G, cen, 1.0, 1e-3, torch.zeros((2, 16), dtype=torch.float64), box=b),
        "gb_apply_cols": lambda b: K.gb_apply_cols(Fg, Pg, cg, sizes, G, cen, 1.0, 1e-3, (None, None, None, None), box=b),
        "gb_distance_range": lambda b: K.gb_distance_range(Pg, cg, G, box=b),
    }[name]
    good = torch.ones((T, 3))
    strided = torch.ones((T, 6))[:, ::2]
    assert tuple(strided.shape) == (T, 3) and not strided.is_contiguous()
    for bad in (torch.ones(2), torch.ones((T + 1, 3)), good.double(), strided, [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="box must be a contiguous"):
            call(bad)
