"""CPU: triclinic cells in gb_feat -- what tests/test_gpu_feat_cell.py relies on, without a GPU.

(1) The constructions of tests/featcell_cases.py in the NumPy references (tests/cell_ref.py, tests/nearest_ref.py):
the dyadic shifts are undone exactly by both images, the displacements outside the brick only by the nearest one, the
random inputs meet the caps and conditions the GPU test asserts.  (2) The refusals, each before any device work.
(3) ``gb_subfeat`` / ``gb_subfeat_jac`` on CPU tensors with a ``Cell``, against ``cell_ref.torch_wrap`` /
``nearest_ref.torch_wrap``."""
import numpy as np
import pytest
import torch

import cell_ref as R
import featcell_cases as C
import jaxfeat_ref as J
import nearest_ref as NR
from aggforce_amd import Cell, LinearMap, Trajectory
from aggforce_amd import _kernels as K
from aggforce_amd.agg import project_forces_grid_cv
from aggforce_amd.qp import Multifeaturize, gb_feat, gbfeat, id_feat, qp_feat_linear_map
from aggforce_amd.qp.jaxfeat import gb_subfeat, gb_subfeat_jac
from aggforce_amd.util import Curry

def exact_in(a, dtype):
    return np.array_equal(np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64), a)


# ------------------------------------------------------------------ the constructions
@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", C.SHAPES)
def test_dyadic_lattice_shifts_are_undone_exactly_by_both_images(T, G, n_cg, n_basis, per_frame):
    Pg, cg, H, moved = C.dyadic_groups(T, G, n_cg, per_frame, seed=5)
    d0, dm = C.displacements(Pg, cg), C.displacements(moved, cg)
    assert exact_in(Pg, np.float32) and exact_in(cg, np.float32) and exact_in(moved, np.float32) and exact_in(dm, np.float32)
    assert np.array_equal(R.wrap(dm, H), d0)
    image, _, gap = NR.nearest(dm, H)
    assert np.array_equal(image, d0) and gap.min() > 0.25
    assert np.abs(dm - d0).max() >= 16.0 and R.tie_distance(dm, H) > 1e-3
    # strictly inside the brick and strictly inside the image radius of every frame's cell
    Hf = C.frames_of(H, T)
    assert (np.abs(d0) < (np.diagonal(Hf, axis1=1, axis2=2) / 2)[:, None, None, :]).all()
    assert np.linalg.norm(d0, axis=-1).max() < NR.image_radius(Hf)
    # some displacements go through the 27-candidate search (longer than min(ax, by, cz) / 2)
    assert (np.sum(d0 * d0, axis=-1) > (Hf[:, 2, 2] ** 2 / 4)[:, None, None]).mean() > 0.03
    # 2e4 displacements per scale, as in the issue
    rng = np.random.default_rng(0)
    for s in C.DYADIC_SCALES:
        Hs = s * NR.DYADIC_NEAR
        d = (rng.integers(0, 256, size=(1, 20000, 3)) / 64.0) - (2 * rng.integers(0, 256, size=(1, 20000, 3)) + 1) / 128.0
        m = d + rng.integers(-2, 3, size=(1, 20000, 3)).astype(np.float64) @ Hs
        assert np.array_equal(R.wrap(m, Hs), d) and np.array_equal(NR.nearest(m, Hs)[0], d)


@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", C.SHAPES)
def test_displacements_outside_the_brick_are_recovered_by_the_nearest_image_only(T, G, n_cg, n_basis, per_frame):
    Pg, cg, H, moved = C.outside_brick_groups(T, G, n_cg, per_frame, seed=6)
    d0, dm = C.displacements(Pg, cg), C.displacements(moved, cg)
    assert exact_in(moved, np.float32) and exact_in(dm, np.float32)
    cz = C.frames_of(H, T)[:, 2, 2][:, None, None]
    assert (np.abs(d0[..., :2]) <= 1).all() and (np.abs(d0[..., 2]) > cz / 2).all() and (np.abs(d0[..., 2]) <= cz / 2 + 1).all()
    radius = np.array([NR.image_radius(h) for h in C.frames_of(H, T)])          # every frame's own
    assert (np.linalg.norm(d0, axis=-1) < radius[:, None, None]).all()
    image, pick, gap = NR.nearest(dm, H)
    assert np.array_equal(image, d0) and gap.min() >= 0.75 and (pick != 0).all()
    assert np.any(R.wrap(dm, H) != d0, axis=-1).all()  # the brick image differs in every case


@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", C.SHAPES)
@pytest.mark.parametrize("kind", C.KINDS)
def test_random_groups_meet_the_caps_and_conditions(kind, T, G, n_cg, n_basis, per_frame):
    Pg, cg, H = C.random_groups(kind, T, G, n_cg, per_frame, C.seed_of(G))
    assert exact_in(Pg, np.float32) and exact_in(H, np.float32)
    assert NR.is_reduced(H) and NR.image_radius(H) >= C.OUTER * (1 - 0.03) - 1e-6
    for near in (False, True):
        _, out, share, picked = C.image_statistics(Pg, cg, H, near)
        assert out.mean() <= 0.02 and share >= 0.5 and picked >= 0.10, (near, out.mean(), share, picked)


def test_near_groups_stay_within_the_safe_radius():
    for T, G, n_cg, _ in C.SHAPES:
        Pg, cg, H = C.near_groups(T, G, n_cg, seed=13)
        d = C.displacements(Pg, cg)
        b = R.wrap(d, H)
        assert np.linalg.norm(b, axis=-1).max() < 4.2 < R.safe_radius(H) and np.abs(d - b).max() > 5.0
        assert (NR.nearest(d, H)[1] == 0).all() and R.tie_distance(d, H) > 1e-3


def test_dyadic_molecules_are_split_by_the_wrap_and_whole_when_moved():
    for H in (4 * NR.DYADIC_NEAR, 2 * NR.DYADIC_NEAR):
        U, forces, moved, wrapped = C.dyadic_molecules(7, H, seed=3)
        assert exact_in(moved, np.float32) and exact_in(wrapped, np.float32)
        bond = U[:, C.BONDS[:, 1]] - U[:, C.BONDS[:, 0]]
        assert np.linalg.norm(bond, axis=-1).max() < R.safe_radius(H)
        assert np.array_equal(moved[:, C.BONDS[:, 1]] - moved[:, C.BONDS[:, 0]], bond)
        assert np.abs((wrapped[:, C.BONDS[:, 1]] - wrapped[:, C.BONDS[:, 0]]) - bond).max() >= 4.0  # split molecules
        assert wrapped.min() >= 0 and (wrapped < np.diagonal(H)).all()  # the brick-shaped unit cell
        shift = np.einsum("tnk,kj->tnj", wrapped - moved, np.linalg.inv(H))
        assert np.array_equal(shift, np.rint(shift))                     # moved there by lattice vectors
        # every pair displacement of the compact trajectory is its own image: brick in the large cell, nearest in both
        d = U[:, :, None, :] - U[:, None, :, :]
        dm = moved[:, :, None, :] - moved[:, None, :, :]
        assert np.linalg.norm(d, axis=-1).max() < NR.image_radius(H) and np.array_equal(NR.nearest(dm, H)[0], d)
        if H[2, 2] >= 16:
            assert np.array_equal(R.wrap(dm, H), d)
        else:
            assert np.abs(d[..., 2]).max() > H[2, 2] / 2  # (beyond the small cell's brick: the nearest image is needed)


# ------------------------------------------------------------------ the refusals
def small(T=6):
    rng = np.random.default_rng(2)
    coords = rng.random((T, 8, 3)).astype(np.float32)
    forces = rng.standard_normal((T, 8, 3)).astype(np.float32)
    return coords, forces, LinearMap([[0, 1], [2, 3], [4, 5, 6, 7]], n_fg_sites=8), {frozenset([0, 1])}


def no_device(monkeypatch):
    monkeypatch.setattr(K, "as_device", lambda *a, **k: pytest.fail("device work before the refusal"))
    monkeypatch.setattr(K, "lib", lambda: pytest.fail("library call before the refusal"))


def test_outer_beyond_the_image_radius_is_refused_before_any_device_work(monkeypatch):
    coords, forces, cmap, cons = small()
    no_device(monkeypatch)
    brick, near = Cell(2 * NR.DYADIC_NEAR), Cell(2 * NR.DYADIC_NEAR, images="nearest")
    assert brick.image_radius == 4.0 and abs(near.image_radius - np.sqrt(48.0)) < 1e-12
    with pytest.raises(ValueError, match=r"gb_feat: outer=6 reaches beyond image_radius=4 of the triclinic cell"):
        gb_feat(coords, cmap, cons, outer=6.0, box=brick)
    with pytest.raises(ValueError, match=r"gb_feat: outer=7 reaches beyond image_radius=6.9\d* of the triclinic cell"):
        gb_feat(coords, cmap, cons, outer=7.0, box=near)
    traj = Trajectory(coords=coords, forces=forces)
    for fused in (True, False):
        feat = Multifeaturize([id_feat, Curry(gb_feat, outer=6.0, n_basis=4, box=brick)])
        with pytest.raises(ValueError, match="gb_feat.*triclinic"):
            qp_feat_linear_map(traj, cmap, feat, 0.6, constraints=cons, fused=fused)
    pts, cg = torch.from_numpy(coords), torch.from_numpy(coords[:, :1])
    with pytest.raises(ValueError, match=r"gb_subfeat: outer=6 reaches beyond image_radius=4 of the triclinic"):
        gb_subfeat(pts, cg, [0] * 8, 1, None, outer=6.0, box=brick)
    with pytest.raises(ValueError, match=r"gb_subfeat_jac: outer=6 reaches beyond image_radius=4 of the triclinic"):
        gb_subfeat_jac(pts, cg, [0] * 8, 1, outer=6.0, box=brick)
    # per frame: the smallest frame decides
    H = np.stack([4 * NR.DYADIC_NEAR] * 5 + [2 * NR.DYADIC_NEAR])
    with pytest.raises(ValueError, match="image_radius=4 "):
        gb_feat(coords, cmap, cons, outer=6.0, box=Cell(H))


def test_an_orthorhombic_box_has_no_such_rule(monkeypatch):
    """The wrap of an orthorhombic box is the minimum image at any distance: lengths shorter than 2 outer pass the
    host checks (the call then reaches the device, which this machine may not have)."""
    coords, forces, cmap, cons = small()
    reached = []
    monkeypatch.setattr(K, "as_device", lambda *a, **k: reached.append(1) or (_ for _ in ()).throw(RuntimeError("device")))
    with pytest.raises(RuntimeError, match="device"):
        gb_feat(coords, cmap, cons, outer=6.0, box=[4.0, 4.0, 4.0])
    assert reached


def test_a_frame_count_mismatch_is_refused_before_any_device_work(monkeypatch):
    coords, forces, cmap, cons = small(T=6)
    no_device(monkeypatch)
    cells = Cell(np.stack([4 * NR.DYADIC_NEAR] * 4))
    with pytest.raises(ValueError, match="gb_feat.*4 frames for 6 frames"):
        gb_feat(coords, cmap, cons, outer=6.0, box=cells)
    feat = Multifeaturize([id_feat, Curry(gb_feat, outer=6.0, n_basis=4, box=cells)])
    with pytest.raises(ValueError, match="4 frames for 6 frames"):
        qp_feat_linear_map(Trajectory(coords=coords, forces=forces), cmap, feat, 0.6, constraints=cons)
    with pytest.raises(ValueError, match="4 frames for 6 frames"):
        gb_subfeat(torch.from_numpy(coords), torch.from_numpy(coords[:, :1]), [0] * 8, 1, None, outer=6.0, box=cells)


def test_a_per_frame_cell_is_refused_in_cross_validation_and_any_cell_under_comm(monkeypatch):
    coords, forces, cmap, cons = small()
    no_device(monkeypatch)
    const = Cell(4 * NR.DYADIC_NEAR)
    per_frame = Cell(np.stack([4 * NR.DYADIC_NEAR] * 6), images="nearest")
    assert not gbfeat._per_frame(const) and gbfeat._per_frame(per_frame)
    feat_c = Multifeaturize([id_feat, Curry(gb_feat, outer=6.0, n_basis=4, box=const)])
    feat_t = Multifeaturize([id_feat, Curry(gb_feat, outer=6.0, n_basis=4, box=per_frame)])
    assert gbfeat.bound_box(feat_c) is const and feat_c.fused_fit is not None and feat_c.fused_cv is not None
    traj = Trajectory(coords=coords, forces=forces)
    for feat in (feat_c, feat_t):
        for fused in (True, False):
            with pytest.raises(ValueError, match="gb_feat.*triclinic cell.*comm="):
                qp_feat_linear_map(traj, cmap, feat, 0.6, constraints=cons, comm=object(), fused=fused)
    with pytest.raises(ValueError, match="per-frame box or Cell"):
        gbfeat.cv_id_gb(coords, forces, cmap, 0.6, 2, cons, [1.0], [np.arange(3), np.arange(3, 6)], None, True,
                        dict(outer=6.0, box=per_frame))
    for reuse in (True, False):
        with pytest.raises(ValueError, match="project_forces_grid_cv.*per-frame"):
            project_forces_grid_cv({"l2_regularization": [1.0, 10.0]}, coords, forces, n_folds=2, reuse_gram=reuse,
                                   coord_map=cmap, constrained_inds=cons, method=qp_feat_linear_map, featurizer=feat_t,
                                   kbt=0.6)


def test_kernel_wrappers_take_the_rows_of_a_cell_and_check_them_first(monkeypatch):
    """(T, 9) rows pass ``_box_arg`` in every K4 wrapper and route to the ``_cell`` entry with the image selector;
    ``near`` without the rows of a cell is refused before the library is touched."""
    T, G = 5, 4
    Pg, cg = torch.zeros((T, G, 3)), torch.zeros((T, 2, 3))
    assert K._gb_box("gb_channels", None, Pg, False) == (None, None)
    assert K._gb_box("gb_channels", torch.ones((T, 9)), Pg, False) == (9, K.IMAGES_BRICK)
    assert K._gb_box("gb_channels", torch.ones((T, 9)), Pg, True) == (9, K.IMAGES_NEAREST)
    assert K._gb_box("gb_channels", torch.ones((T, 3)), Pg, False) == (3, None)
    assert K._gb_box("gb_channels", torch.ones(3), Pg, False) == (0, None)
    monkeypatch.setattr(K, "lib", lambda: pytest.fail("library call before the box was checked"))
    for bad in (torch.ones(3), torch.ones((T, 3)), torch.ones((T + 1, 9))):
        with pytest.raises(ValueError, match="nearest image needs"):
            K.gb_channels(Pg, cg, 0, torch.ones(G), G, torch.ones(3), 1.0, 1e-3, box=bad, near=True)
        with pytest.raises(ValueError, match="nearest image needs"):
            K.gb_distance_range(Pg, cg, G, box=bad, near=True)
    with pytest.raises(ValueError, match="box must be a contiguous"):
        K.gb_channels(Pg, cg, 0, torch.ones(G), G, torch.ones(3), 1.0, 1e-3, box=torch.ones((T, 9), dtype=torch.float64))


# ------------------------------------------------------------------ the array functions on CPU tensors
def subfeat_system(per_frame, T=5, N=7, seed=51):
    rng = np.random.default_rng(seed)
    H = 2.2 * (R.frame_cells(T) if per_frame else R.SKEW)  # reduced; safe_radius >= 4.37 > outer
    Hf = C.frames_of(H, T)
    ids = np.array([0, 0, 1, 2, 2, 3, 4])
    centre = np.einsum("tgk,tkj->tgj", rng.random((T, 5, 3)), Hf)
    pts = centre[:, ids, :] + 0.3 * rng.random((T, N, 3))
    cg = np.einsum("tgk,tkj->tgj", rng.random((T, 1, 3)), Hf)
    return H, ids, pts, cg


@pytest.mark.parametrize("images", ["brick", "nearest"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
def test_subfeat_and_its_jacobian_on_cpu_tensors_follow_the_reference_wrap(per_frame, images):
    H, ids, pts_h, cg_h = subfeat_system(per_frame)
    T, N, _ = pts_h.shape
    nb, n_ch = 6, 4
    kw = dict(outer=4.0, inner=0.0, n_basis=nb, width=1.0, dist_power=0.5)
    cell = Cell(H, images=images)
    assert cell.image_radius >= 4.0
    wrap_t = NR.torch_wrap if images == "nearest" else R.torch_wrap
    wrap_n = NR.wrap if images == "nearest" else R.wrap
    pts = torch.tensor(pts_h, dtype=torch.float64, requires_grad=True)
    cg = torch.tensor(cg_h, dtype=torch.float64)
    d_ref = wrap_n(pts_h - cg_h, H)
    assert np.abs(d_ref - (pts_h - cg_h)).max() > 1.0  # the cell matters on these inputs
    cen = J.centers(4.0, 0.0, nb, 0.5, np.float64)
    ref = J.channel_allocate(J.basis(np.linalg.norm(d_ref, axis=-1), cen, 1.0, 1e-3), ids, n_ch)
    got = gb_subfeat(pts, cg, ids, n_ch, None, box=cell, **kw)
    assert got.shape == (T, N, n_ch * nb) and np.abs(got.detach().numpy() - ref).max() < 1e-12
    assert np.abs(gb_subfeat(pts, cg, ids, n_ch, None, **kw).detach().numpy() - ref).max() > 1e-2
    # the Jacobian against autograd through the reference's wrap
    r_ref = torch.linalg.vector_norm(wrap_t(pts - cg, H), dim=-1)
    z = (r_ref[..., None] - torch.tensor(cen)) / 1.0
    e = torch.exp(-(z * z))
    basis = torch.clamp(e, min=1e-3) - 1e-3                                      # (T, N, nb)
    onehot = torch.zeros((n_ch, N), dtype=torch.float64)
    keep = np.flatnonzero(ids < n_ch)
    onehot[torch.from_numpy(ids[keep]), torch.from_numpy(keep)] = 1
    collapsed = torch.einsum("tak,ca->ck", basis, onehot).reshape(-1)
    auto = torch.stack([torch.autograd.grad(collapsed[f], pts, retain_graph=True)[0].sum(dim=1)
                        for f in range(n_ch * nb)], dim=1)
    jac = gb_subfeat_jac(pts, cg, ids, n_ch, box=cell, **kw)
    assert float(auto.abs().max()) > 0.1
    assert float((jac - auto).abs().max()) < 1e-10 * float(auto.abs().max())
    # differentiable: the gradient of a functional of the Jacobian exists and is finite
    (g,) = torch.autograd.grad((jac * jac).sum(), pts)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # and through the collapsed features of gb_subfeat itself
    coll = gb_subfeat(pts, cg, ids, n_ch, None, collapse=True, box=cell, **kw)
    auto2 = torch.stack([torch.autograd.grad(coll[f], pts, retain_graph=True)[0].sum(dim=1) for f in range(n_ch * nb)], dim=1)
    assert float((auto2 - auto).abs().max()) < 1e-10 * float(auto.abs().max())
