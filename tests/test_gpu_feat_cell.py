"""GPU: triclinic cells in gb_feat -- the cell forms (brick and nearest image) of the K4 kernels, gb_feat(box=Cell), the
fused fit, the one-pass cross-validation, the fitted map's application and the array functions of qp.jaxfeat.

Evidence of three kinds.  (1) Exact: a diagonal cell gives the box form's bits; on the dyadic inputs of
tests/featcell_cases.py a shift by lattice vectors is undone bit for bit by both images (and a displacement outside
the brick only by the nearest one); within safe_radius the nearest form gives the brick form's bits.  (2) Genuinely
different images: against the NumPy float64 references tests/cell_ref.py / tests/nearest_ref.py put through the
oracle's Gaussian expressions, to the open path's tolerances.  (3) The public level on wrapped trajectories.  The
constructions are checked on the CPU in tests/test_feat_cell_host.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cell_ref as R  # noqa: E402
import featcell_cases as C  # noqa: E402
import featpbc_cases as box_cases  # noqa: E402
import nearest_ref as NR  # noqa: E402
import stream_gate as SG  # noqa: E402
import test_gpu_feat_pbc as base  # noqa: E402  (kernel_operands, open_test_system, molecule_oracle, rel, dev, _fit_kwargs)
from aggforce_amd import Cell, LinearMap, Trajectory, project_forces  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd.qp import Multifeaturize, gb_feat, id_feat, qp_feat_linear_map  # noqa: E402
from aggforce_amd.qp.gbfeat import CLIP, gb_centers  # noqa: E402
from aggforce_amd.util import Curry  # noqa: E402
from oracle import aggforce_oracle as orc  # noqa: E402

KBT = base.KBT
TOL_FEAT, TOL_DIV = base.TOL_FEAT, base.TOL_DIV  # 2e-6, 2e-5: the open path's, float32
TOL_F64 = 1e-10
F32, F64 = torch.float32, torch.float64
DTYPES, SHAPES = base.DTYPES, C.SHAPES
DTYPE_IDS = ["fff", "ffd", "dfd", "fdd", "ddd"]
IMAGES = ["brick", "nearest"]
NAMES = ("gauss", "grad", "regmat", "apply", "apply_cols", "rmin", "rmax")
rel, dev = base.rel, base.dev


def operands(Pg, cg, tf, tg, n_basis, seed=9, outer=6.0):
    return base.kernel_operands(Pg, cg, None, tf, tg, n_basis, seed, outer=outer)


def cell_rows(H, T, tg):
    return dev(C.rows(H, T), tg)


def run_kernels(op, Pg, box, out_dtype, near=False):
    """(gauss, grad, R3, applied, applied from the compact list, rmin, rmax) of all sites: open (box None), under the
    lengths of a box, or under the (T, 9) rows of a cell with the brick or (``near``) the nearest image."""
    Fg = dev(op["Fg_h"], op["tf"])
    G, n_ch, cen = op["G"], op["n_ch"], op["centers"]
    ld = -(-(G + len(op["cols_h"])) // 128) * 128
    kw = dict(box=box, near=near) if near else dict(box=box)
    gauss, grad, R3s = [], [], []
    for site in range(op["n_cg"]):
        g, d = K.gb_channels(Pg, op["cg"], site, op["sizes"], n_ch, cen, 1.0, CLIP, **kw)
        R3 = torch.zeros((op["T"], ld, 3), dtype=out_dtype, device="cuda")
        K.gb_regmat_cols(Fg, Pg, op["cg"], site, op["sizes"], G, op["cols"], cen, 1.0, CLIP, KBT, R3, **kw)
        gauss.append(g), grad.append(d), R3s.append(R3)
    app = K.gb_apply(Fg, Pg, op["cg"], op["sizes"], G, n_ch, cen, 1.0, CLIP, op["coef"], **kw)
    app_c = K.gb_apply_cols(Fg, Pg, op["cg"], op["sizes"], G, cen, 1.0, CLIP, op["compact"], **kw)
    rmin, rmax = K.gb_distance_range(Pg, op["cg"], n_ch, **kw)
    return torch.stack(gauss), torch.stack(grad), torch.stack(R3s), app, app_c, rmin, rmax


# ------------------------------------------------------------------ 1. a diagonal cell is the box form
@pytest.mark.parametrize("images", IMAGES)
@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", SHAPES)
@pytest.mark.parametrize("tf,tg,to", DTYPES, ids=DTYPE_IDS)
def test_a_diagonal_cell_gives_the_box_forms_bits(tf, tg, to, T, G, n_cg, n_basis, per_frame, images):
    """Check 1: ``Cell(diag(L))``, brick and nearest, against ``box=L`` on the random groups of the box test (most
    displacements have a nearer image): torch.equal on all seven outputs of the five kernels."""
    Pg, cg, L = box_cases.random_groups(T, G, n_cg, per_frame, seed=base_seed(G))
    op = operands(Pg, cg, tf, tg, n_basis)
    Lf = np.broadcast_to(L, (T, 3))
    H = np.zeros((T, 3, 3))
    H[:, [0, 1, 2], [0, 1, 2]] = Lf
    boxed = run_kernels(op, op["Pg"], dev(L, tg), to)
    celled = run_kernels(op, op["Pg"], cell_rows(H, T, tg), to, near=images == "nearest")
    open_ = run_kernels(op, op["Pg"], None, to)
    for name, a, b, c in zip(NAMES, boxed, celled, open_):
        assert torch.equal(a, b), name
        assert not torch.equal(a, c), name


def base_seed(G):
    return 11 if G == 20 else 12


# ------------------------------------------------------------------ 2. lattice shifts are undone bit for bit
@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", SHAPES)
@pytest.mark.parametrize("tf,tg,to", DTYPES, ids=DTYPE_IDS)
def test_cell_kernels_undo_a_shift_by_lattice_vectors_bit_for_bit(tf, tg, to, T, G, n_cg, n_basis, per_frame):
    """Check 2: dyadic cells s * DYADIC_NEAR (one for all frames, or s in {2, 4, 8} by frame), every (frame, group)
    moved by i a + j b + k c with counts in [-2, 2]: both forms on the moved input equal the open kernels on the
    unmoved input, and the open kernels on the moved input do not."""
    Pg, cg, H, moved = C.dyadic_groups(T, G, n_cg, per_frame, seed=5)
    op = operands(Pg, cg, tf, tg, n_basis)
    cell = cell_rows(H, T, tg)
    open_ = run_kernels(op, op["Pg"], None, to)
    moved_open = run_kernels(op, dev(moved, tg), None, to)
    for near in (False, True):
        got = run_kernels(op, dev(moved, tg), cell, to, near=near)
        for name, a, b, c in zip(NAMES, open_, got, moved_open):
            assert torch.isfinite(a).all() or name == "rmin", name
            assert torch.equal(a, b), (name, near)
            assert not torch.equal(a, c), name
    assert float(open_[0].abs().max()) > 0.1 and float(open_[6].max()) < 7.0


@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", SHAPES)
@pytest.mark.parametrize("tf,tg,to", DTYPES, ids=DTYPE_IDS)
def test_a_displacement_outside_the_brick_is_recovered_by_the_nearest_form_only(tf, tg, to, T, G, n_cg, n_basis,
                                                                                  per_frame):
    """Check 2b: the unmoved displacement lies outside the brick but inside image_radius (|dx|, |dy| <= 1, |dz| in
    (cz/2, cz/2 + 1]): the nearest form on the moved input reproduces the open bits, the brick form does not."""
    Pg, cg, H, moved = C.outside_brick_groups(T, G, n_cg, per_frame, seed=6)
    op = operands(Pg, cg, tf, tg, n_basis)  # (the unmoved distances lie between cz / 2 = 4 and 5.2 in the smallest cell)
    cell = cell_rows(H, T, tg)
    open_ = run_kernels(op, op["Pg"], None, to)
    near = run_kernels(op, dev(moved, tg), cell, to, near=True)
    brick = run_kernels(op, dev(moved, tg), cell, to, near=False)
    for name, a, b, c in zip(NAMES, open_, near, brick):
        assert torch.equal(a, b), name
        assert not torch.equal(a, c), name
    assert float(open_[0].abs().max()) > 0.1


# ------------------------------------------------------------------ 3. against float64 on the host
def host_oracle(op, cg, d_img, outer=C.OUTER):
    """float64 on the host: the reference image ``d_img`` (T, n_cg, G, 3), then the oracle's Gaussians and derivatives
    (one group per atom, identity smear: the kernel's channels), the regression matrix columns and the applied map
    built from them -- ``host_oracle`` of the orthorhombic test with another image."""
    T, G, n_ch, nb = op["T"], op["G"], op["n_ch"], op["n_basis"]
    gauss = np.zeros((op["n_cg"], T, n_ch, nb))
    grad = np.zeros((op["n_cg"], T, n_ch, nb, 3))
    for site in range(op["n_cg"]):
        feats, divs = orc.gb_feat_site(cg[:, site, None, :] + d_img[:, site], cg[:, site], np.arange(G), np.eye(G),
                                       outer=outer, inner=0.0, n_basis=nb, width=1.0, dist_power=0.5, clip=CLIP,
                                       n_channels=n_ch, dtype=np.float64)
        ch = np.arange(n_ch)
        gauss[site] = feats.reshape(T, G, n_ch, nb)[:, ch, ch, :]
        grad[site] = op["sizes_h"][None, :n_ch, None, None] * divs.reshape(T, n_ch, nb, 3)
    F = op["Fg_h"]
    full = gauss[..., None] * F[None, :, :n_ch, None, :]
    regmat = (full + KBT * grad).reshape(op["n_cg"], T, n_ch * nb, 3)[:, :, op["cols_h"], :]
    c_id, c_gb = op["coef_h"][:, :G], op["coef_h"][:, G:].reshape(op["n_cg"], n_ch, nb)
    applied = np.einsum("cg,tgd->tcd", c_id, F) + np.einsum("cgk,ctgkd->tcd", c_gb, full + grad)
    return gauss, grad, regmat, applied


@pytest.mark.parametrize("images", IMAGES)
@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", SHAPES)
@pytest.mark.parametrize("tg", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_cell_kernels_match_float64_images_on_the_host(kind, tg, T, G, n_cg, n_basis, per_frame, images):
    """Check 3: ``nearest_ref.STANDARD[kind](12.0)``, one cell or breathing by 3 % per frame, group means and sites
    uniform in the cell as stored in float32, outer 6, width 1: against cell_ref.brick / nearest_ref.nearest in float64
    and the oracle's Gaussian expressions.  float32: features to 2e-6, divergences to 2e-5 (the open path's); float64:
    1e-10 relative.  The regression matrix and both applications to the bounds of the orthorhombic test.  Left out:
    triples within 1e-3 of a tie in a brick stage or (nearest form) with a candidate gap below nearest_ref.TIE -- at
    most 2 % (asserted); the image differs from the raw displacement in at least half the triples and pick != 0 in at
    least 10 % (asserted)."""
    near = images == "nearest"
    Pg, cg, H = C.random_groups(kind, T, G, n_cg, per_frame, C.seed_of(G))
    op = operands(Pg, cg, F32, tg, n_basis)
    d_img, left_out, share, picked = C.image_statistics(Pg, cg, H, near)
    assert left_out.mean() <= 0.02 and share >= 0.5 and picked >= 0.10
    gauss_o, grad_o, reg_o, app_o = host_oracle(op, cg, d_img)
    ok = ~np.transpose(left_out, (1, 0, 2))[:, :, :op["n_ch"]]                 # (n_cg, T, n_ch)
    gauss, grad, R3, app, app_c, rmin, rmax = (x.cpu().numpy().astype(np.float64) for x in
                                                run_kernels(op, op["Pg"], cell_rows(H, T, tg), F64, near=near))
    open_gauss = run_kernels(op, op["Pg"], None, F64)[0].cpu().numpy()
    assert np.abs(open_gauss - gauss_o)[ok].max() > 0.05                       # the images really differ
    tol_f, tol_d = (TOL_FEAT, TOL_DIV) if tg == F32 else (TOL_F64 * np.abs(gauss_o).max(), TOL_F64 * np.abs(grad_o).max())
    err_f, err_d = np.abs(gauss - gauss_o)[ok].max(), np.abs(grad - grad_o)[ok].max()
    print(f"{kind} {images}: left out {left_out.mean():.4f}, image differs {share:.3f}, pick != 0 {picked:.3f}; "
          f"features {err_f:.2e} (tol {tol_f:.1e}), divergences {err_d:.2e} (tol {tol_d:.1e})")
    assert err_f < tol_f and err_d < tol_d
    # regression matrix columns (id block = the force sums, exactly)
    Fmax = np.abs(op["Fg_h"]).max()
    nid = op["G"]
    assert np.array_equal(R3[:, :, :nid, :], np.broadcast_to(op["Fg_h"], (n_cg,) + op["Fg_h"].shape))
    ok_cols = np.repeat(ok, n_basis, axis=2)[:, :, op["cols_h"]]
    got = R3[:, :, nid:nid + len(op["cols_h"]), :]
    bound_reg = tol_f * Fmax + KBT * tol_d + 4 * 2.0 ** -24 * np.abs(reg_o).max()
    err_r = np.abs(got - reg_o)[ok_cols].max()
    print(f"regression matrix {err_r:.2e} (bound {bound_reg:.2e})")
    assert err_r < bound_reg
    # the applied map: frames and sites none of whose channels is left out
    clean = np.transpose(ok.all(axis=2))                                       # (T, n_cg)
    assert clean.mean() > 0.3
    weight = np.abs(op["coef_h"][:, nid:]).sum(axis=1).max()
    bound_app = weight * (tol_f * Fmax + tol_d)
    err_a, err_c = np.abs(app - app_o)[clean].max(), np.abs(app_c - app_o)[clean].max()
    print(f"applied {err_a:.2e}, from the compact list {err_c:.2e} (bound {bound_app:.2e})")
    assert err_a < bound_app and err_c < bound_app
    assert rel(app_c, app) < 1e-12
    # the range: that of the image distances
    r_o = np.linalg.norm(d_img, axis=-1)                                       # (T, n_cg, G)
    r_o = np.where(left_out, np.nan, r_o)
    n_ch = op["n_ch"]
    assert np.all(rmin[:, :n_ch] <= np.nanmin(r_o, axis=0)[:, :n_ch] + 1e-5)
    assert np.all(rmax[:, :n_ch] >= np.nanmax(r_o, axis=0)[:, :n_ch] - 1e-5)
    if not left_out.any(axis=0)[:, :n_ch].any():
        assert np.abs(rmin[:, :n_ch] - np.nanmin(r_o, axis=0)[:, :n_ch]).max() < 1e-5


# ------------------------------------------------------------------ 4. within safe_radius the two forms coincide
@pytest.mark.parametrize("T,G,n_cg,n_basis", SHAPES)
@pytest.mark.parametrize("tf,tg,to", DTYPES, ids=DTYPE_IDS)
def test_within_the_safe_radius_the_nearest_form_gives_the_brick_forms_bits(tf, tg, to, T, G, n_cg, n_basis):
    """Check 4: every image shorter than 4.2 < safe_radius 4.9 of the truncated octahedron (group means moved by
    lattice vectors): the search is pruned or finds nothing shorter, and all seven outputs are equal bit for bit."""
    Pg, cg, H = C.near_groups(T, G, n_cg, seed=13)
    op = operands(Pg, cg, tf, tg, n_basis)
    cell = cell_rows(H, T, tg)
    brick = run_kernels(op, op["Pg"], cell, to)
    near = run_kernels(op, op["Pg"], cell, to, near=True)
    open_ = run_kernels(op, op["Pg"], None, to)
    for name, a, b, c in zip(NAMES, brick, near, open_):
        assert torch.equal(a, b), name
        assert not torch.equal(a, c), name
    assert float(brick[6][:, :op["n_ch"]].max()) < 4.2 and float(brick[0].abs().max()) > 0.1


# ------------------------------------------------------------------ 5. a bad cell
@pytest.mark.parametrize("images", IMAGES)
def test_a_bad_cell_poisons_its_frame_and_no_other(images):
    """Check 5: a NaN, zero, negative or infinite diagonal entry, or a NaN off-diagonal entry, in one frame of a cell
    on the device: that frame's features, Gaussian regression columns and applied rows are NaN, the id block is
    untouched, every other frame is bit for bit what a good cell gives, and the distance range of every channel spans
    everything."""
    near = images == "nearest"
    Pg, cg, H = C.random_groups("octahedron", 7, 20, 3, True, seed=11)
    op = operands(Pg, cg, F32, F32, 4)
    cell = cell_rows(H, 7, F32)
    good = run_kernels(op, op["Pg"], cell, F64, near=near)
    nid, n_ch = op["G"], op["n_ch"]
    for frame, entry, value in ((3, 4, float("nan")), (0, 0, 0.0), (6, 8, -4.0), (5, 0, float("inf")), (2, 6, float("nan"))):
        bad_cell = cell.clone()
        bad_cell[frame, entry] = value
        bad = run_kernels(op, op["Pg"], bad_cell, F64, near=near)
        others = [t for t in range(7) if t != frame]
        for name, a, b in zip(("gauss", "grad"), good[:2], bad[:2]):
            assert torch.isnan(b[:, frame]).all() and torch.equal(a[:, others], b[:, others]), name
        assert torch.isnan(bad[2][:, frame, nid:nid + len(op["cols_h"])]).all()
        assert torch.equal(bad[2][:, frame, :nid], good[2][:, frame, :nid])   # the id block holds no distance
        assert torch.equal(bad[2][:, others], good[2][:, others])
        for a, b in zip(good[3:5], bad[3:5]):
            assert torch.isnan(b[frame]).all() and torch.equal(a[others], b[others])
        assert (bad[5][:, :n_ch] == 0).all() and torch.isinf(bad[6][:, :n_ch]).all()
    # an upper-triangular entry is not read
    upper = cell.clone()
    upper[1, 1] = float("nan")
    for a, b in zip(good, run_kernels(op, op["Pg"], upper, F64, near=near)):
        assert torch.equal(a, b)
    # through gb_feat: a cell that lives on the device is not read on the host (no check on the host)
    Hm = 4 * NR.DYADIC_NEAR
    U, forces, moved, wrapped = C.dyadic_molecules(7, Hm, seed=3)
    dcell = torch.from_numpy(np.broadcast_to(Hm, (7, 3, 3)).copy()).cuda()
    dcell[2, 0, 0] = float("nan")
    cmap = LinearMap(orc.list_mapping_matrix(C.BEADS, C.N_ATOMS))
    res = gb_feat(moved.astype(np.float32), cmap, C.CONS, outer=6.0, n_basis=4, lazy=False, box=Cell(dcell, images=images))
    ref = gb_feat(U.astype(np.float32), cmap, C.CONS, outer=6.0, n_basis=4, lazy=False)
    keep = [0, 1, 3, 4, 5, 6]
    for c in range(4):
        assert np.isnan(res["divs"][c][2]).all() and np.array_equal(res["divs"][c][keep], ref["divs"][c][keep])
        assert np.array_equal(res["feats"][c][keep], ref["feats"][c][keep])


# ------------------------------------------------------------------ 6. public level
PUBLIC_CELLS = {"brick": lambda: Cell(4 * NR.DYADIC_NEAR), "nearest": lambda: Cell(2 * NR.DYADIC_NEAR, images="nearest")}


def molecule_oracle(U, n_basis, outer=6.0):
    ids = orc.id_feat_ids(C.N_ATOMS, C.CONS)
    smear = orc.smear_matrix(orc.reduce_constraint_sets(C.CONS), C.N_ATOMS)
    cmat = orc.list_mapping_matrix(C.BEADS, C.N_ATOMS)
    cgs = orc.linearmap_apply(U, cmat)
    return [orc.gb_feat_site(U, cgs[:, c, :], ids, smear, outer=outer, inner=0.0, n_basis=n_basis, width=1.0,
                             dist_power=0.5, n_channels=int(ids.max())) for c in range(4)]


@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("images", IMAGES)
def test_gb_feat_with_a_cell_matches_the_oracle_on_the_unwrapped_trajectory(images, per_frame):
    """Check 6: whole dyadic molecules moved by lattice vectors; with ``box=Cell`` gb_feat gives what the oracle gives
    on the compact trajectory (2e-6 / 2e-5) -- and, the inputs being dyadic, exactly what gb_feat gives there without a
    box; without ``box=`` it does not.  ``Cell(2 * DYADIC_NEAR)`` in the brick form with outer 6 is refused."""
    cell = PUBLIC_CELLS[images]()
    H = cell.vectors.numpy()
    T = 7
    U, forces, moved, wrapped = C.dyadic_molecules(T, H, seed=3)
    if per_frame:
        cell = Cell(np.broadcast_to(H, (T, 3, 3)).copy(), images=images)
    cmap = LinearMap(orc.list_mapping_matrix(C.BEADS, C.N_ATOMS))
    kw = dict(outer=6.0, inner=0.0, n_basis=5, width=1.0, dist_power=0.5, lazy=False)
    res = gb_feat(moved.astype(np.float32), cmap, C.CONS, box=cell, **kw)
    same_ = gb_feat(U.astype(np.float32), cmap, C.CONS, **kw)
    openf = gb_feat(moved.astype(np.float32), cmap, C.CONS, **kw)
    lazy = gb_feat(moved.astype(np.float32), cmap, C.CONS, box=cell, **dict(kw, lazy=True))
    ref = molecule_oracle(U.astype(np.float32), 5)
    for c, (f_o, d_o) in enumerate(ref):
        f, d = res["feats"][c], res["divs"][c]
        assert f.dtype == np.float32 and f.shape == f_o.shape and d.shape == d_o.shape
        assert np.max(np.abs(f - f_o)) < TOL_FEAT and np.max(np.abs(d - d_o)) < TOL_DIV
        assert np.array_equal(f, same_["feats"][c]) and np.array_equal(d, same_["divs"][c])
        assert np.max(np.abs(openf["feats"][c] - f_o)) > 0.05
    assert np.array_equal(next(iter(lazy["feats"])), res["feats"][0])
    with pytest.raises(ValueError, match="gb_feat: outer=6 reaches beyond image_radius=4 of the triclinic cell"):
        gb_feat(moved.astype(np.float32), cmap, C.CONS, box=Cell(2 * NR.DYADIC_NEAR), **kw)
    with pytest.raises(ValueError, match="frames"):
        gb_feat(moved.astype(np.float32), cmap, C.CONS, box=Cell(np.broadcast_to(H, (T + 1, 3, 3)).copy(), images=images), **kw)


@pytest.mark.parametrize("images", IMAGES)
def test_project_forces_on_a_wrapped_trajectory_in_a_cell_matches_the_unwrapped_one(images):
    """Check 6, through project_forces: atoms wrapped into the cell (molecules split over faces), ``box=Cell`` and
    ``bonds=`` to make them whole, the cell bound in the featuriser -- against the compact trajectory without any box:
    coefficients and mapped forces to 2e-4, kept columns identical.  Without the cell in the featuriser the fit is a
    different one (by more than 1e-3).  This is the test that fails without the feature: ``gb_feat`` refused every
    ``Cell``."""
    T = 48
    cell = PUBLIC_CELLS[images]()
    U, forces, moved, wrapped = C.dyadic_molecules(T, cell.vectors.numpy(), seed=3)
    U32, W32, F32h = U.astype(np.float32), wrapped.astype(np.float32), forces.astype(np.float32)
    cmap = LinearMap(orc.list_mapping_matrix(C.BEADS, C.N_ATOMS))
    gbkw = dict(outer=6.0, inner=0.0, n_basis=4, width=1.0)
    fit = base._fit_kwargs(T)
    ref = project_forces(U32, F32h, cmap, constrained_inds=C.CONS, method=qp_feat_linear_map,
                         featurizer=Multifeaturize([id_feat, Curry(gb_feat, **gbkw)]), **fit)
    got = project_forces(W32, F32h, cmap, constrained_inds=C.CONS, method=qp_feat_linear_map, box=cell,
                         bonds=C.BONDS, featurizer=Multifeaturize([id_feat, Curry(gb_feat, box=cell, **gbkw)]), **fit)
    blind = project_forces(W32, F32h, cmap, constrained_inds=C.CONS, method=qp_feat_linear_map, box=cell,
                           bonds=C.BONDS, featurizer=Multifeaturize([id_feat, Curry(gb_feat, **gbkw)]), **fit)
    coef = lambda r: np.stack(r["tmap"].force_map.tags["coef_list"])  # noqa: E731
    print(f"{images}: coefficients {rel(coef(got), coef(ref)):.2e}, mapped forces "
          f"{rel(got['mapped_forces'], ref['mapped_forces']):.2e}; without the cell {rel(coef(blind), coef(ref)):.2e}")
    assert rel(coef(got), coef(ref)) < 2e-4 and rel(got["mapped_forces"], ref["mapped_forces"]) < 2e-4
    assert rel(coef(blind), coef(ref)) > 1e-3 and rel(blind["mapped_forces"], ref["mapped_forces"]) > 1e-3
    assert got["tmap"].force_map.tags["fit_info"]["kept_columns"] == ref["tmap"].force_map.tags["fit_info"]["kept_columns"]
    if images == "nearest":
        with pytest.raises(ValueError, match="gb_feat.*triclinic"):
            project_forces(W32, F32h, cmap, constrained_inds=C.CONS, method=qp_feat_linear_map, box=cell, bonds=C.BONDS,
                           featurizer=Multifeaturize([id_feat, Curry(gb_feat, box=Cell(2 * NR.DYADIC_NEAR), **gbkw)]), **fit)


def cell_for(kind, edge, T, per_frame, images, seed=0):
    H = NR.STANDARD[kind](edge)
    if per_frame:
        H = H[None] * (1 + 0.03 * np.random.default_rng(8000 + seed).uniform(-1, 1, T))[:, None, None]
    return H, Cell(H, images=images)


@pytest.mark.parametrize("images", IMAGES)
@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
def test_fused_fit_matches_the_dense_path_with_a_cell(per_frame, images):
    """Check 6: qp_feat_linear_map fused and dense with the same sampled frames and the same bound cell (the system of
    the orthorhombic test in a truncated octahedron of edge 8: whole molecules anywhere in the cell): coefficients and
    mapped forces to 2e-4; the fitted map applies to other trajectories with a constant cell and to trajectories of
    the fit's own length with a per-frame one, and refuses any other length."""
    T, N = 60, 16
    rng = np.random.default_rng(31)
    H, cell = cell_for("octahedron", 8.0, T, per_frame, images)
    assert cell.image_radius >= 3.0
    Hf = C.frames_of(H, T)
    centre = np.einsum("tmk,tkj->tmj", rng.random((T, 4, 3)), Hf)
    coords = (centre[:, :, None, :] + 0.5 * rng.random((T, 4, 4, 3))).reshape(T, N, 3).astype(np.float32)
    forces = (25 * rng.standard_normal((T, N, 3))).astype(np.float32)
    cmap = LinearMap(orc.list_mapping_matrix(C.BEADS, N))
    smear = orc.smear_matrix(orc.reduce_constraint_sets(C.CONS), N).astype(np.float64)
    Pg = np.einsum("tfd,cf->tcd", coords.astype(np.float64), smear)
    cgs = orc.linearmap_apply(coords.astype(np.float64), cmap.standard_matrix)
    _, _, share, _ = C.image_statistics(Pg, cgs, H, images == "nearest")
    assert share >= 0.25
    feat = Multifeaturize([id_feat, Curry(gb_feat, outer=3.0, inner=0.0, n_basis=4, width=0.5, box=cell)])
    traj = Trajectory(coords=coords, forces=forces)
    fit = base._fit_kwargs(T)
    kbt = fit.pop("kbt")
    fused = qp_feat_linear_map(traj, cmap, feat, kbt, constraints=C.CONS, **fit)
    dense = qp_feat_linear_map(traj, cmap, feat, kbt, constraints=C.CONS, fused=False, **fit)
    cf, cd = np.stack(fused.force_map.tags["coef_list"]), np.stack(dense.force_map.tags["coef_list"])
    print(f"fused against dense: coefficients {rel(cf, cd):.2e}, mapped forces {rel(fused(traj).forces, dense(traj).forces):.2e}")
    assert rel(cf, cd) < 2e-4
    assert rel(fused(traj).forces, dense(traj).forces) < 2e-4
    info = fused.force_map.tags["fit_info"]
    assert max(info["kept_columns"]) < info["n_feat"]
    other = Trajectory(coords=coords[:11], forces=forces[:11])
    if per_frame:
        for m in (fused, dense):
            with pytest.raises(ValueError, match="frames"):
                m(other)
    else:
        assert rel(fused(other).forces, fused(traj).forces[:11]) < 1e-12
        assert rel(dense(other).forces, dense(traj).forces[:11]) < 1e-6


COMPACTION_CELL = np.array([[64.0, 0, 0], [16.0, 72.0, 0], [-20.0, 24.0, 96.0]])


@pytest.mark.parametrize("images", IMAGES)
@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
def test_zero_column_compaction_is_exact_with_a_cell(per_frame, images, monkeypatch):
    """Check 6: column compaction on and off give the same coefficients and mapped forces under a cell, to 1e-7 -- on
    the system of the orthorhombic test (two clusters 40 apart, one sampled frame per site) in a skewed cell whose
    images keep the clusters apart, the second cluster moved by its own lattice vectors in every frame: the kept
    columns are decided by the range of the IMAGE distances."""
    from aggforce_amd.qp import gbfeat

    rng = np.random.default_rng(21)
    T, N = 80, 24
    base_x = np.concatenate([3.0 * rng.random((N // 2, 3)), 3.0 * rng.random((N // 2, 3)) + 40.0])
    coords = base_x[None] + 0.2 * rng.standard_normal((T, N, 3))
    forces = (25 * rng.standard_normal((T, N, 3))).astype(np.float32)
    H = COMPACTION_CELL if not per_frame else COMPACTION_CELL[None] * (1 + 0.05 * rng.random((T, 1, 1)))
    coords[:, N // 2:] += C.lattice(rng.integers(-1, 2, size=(T, 1, 3)), H)
    coords = coords.astype(np.float32)
    cons = {frozenset([1, 2]), frozenset([13, 14]), frozenset([14, 15]), frozenset([20, 23])}
    cmap = LinearMap(orc.list_mapping_matrix([[0, 1], [4, 7], [12, 13], [18, 22]], N))
    feat = Multifeaturize([id_feat, Curry(gb_feat, outer=6.0, inner=0.0, n_basis=5, width=1.0, box=Cell(H, images=images))])
    frames = [np.array([k]) for k in (3, 17, 40, 66)]
    traj = Trajectory(coords=coords, forces=forces)
    small = qp_feat_linear_map(traj, cmap, feat, KBT, constraints=cons, frame_indices=frames, l2_regularization=10.0)
    info = small.force_map.tags["fit_info"]
    assert max(info["kept_columns"]) < 0.7 * info["n_feat"]  # the far cluster's columns are gone
    monkeypatch.setattr(gbfeat, "COMPACT_ZERO_COLUMNS", False)
    full = qp_feat_linear_map(traj, cmap, feat, KBT, constraints=cons, frame_indices=frames, l2_regularization=10.0)
    monkeypatch.undo()
    assert full.force_map.tags["fit_info"]["kept_columns"] == [info["n_feat"]] * 4
    cs, cf = np.stack(small.force_map.tags["coef_list"]), np.stack(full.force_map.tags["coef_list"])
    print(f"compaction on/off: coefficients {rel(cs, cf):.2e}, mapped forces {rel(small(traj).forces, full(traj).forces):.2e}")
    assert rel(cs, cf) < 1e-7
    assert rel(small(traj).forces, full(traj).forces) < 1e-7
    G = info["n_feat"] // 6 + 1  # n_feat = G + 5 (G - 1)
    for c in range(4):
        dead = np.setdiff1d(np.arange(info["n_feat"] - G), info["kept_gauss_columns"][c])
        assert len(dead) > 0 and np.all(cs[c, G + dead] == 0.0) and np.abs(cs[c, G:]).max() > 0


@pytest.mark.parametrize("images,with_id,edge,outer", [("brick", True, 20.0, 8.0), ("nearest", True, 20.0, 8.0),
                                                         ("nearest", False, 30.0, 12.0)])
def test_featurised_grid_cv_one_pass_matches_the_loop_with_a_cell(images, with_id, edge, outer):
    """Check 6: project_forces_grid_cv with a constant cell bound in the featuriser: the one-pass scores equal the
    loop's to 1e-5 (sds 1e-3) -- on the system of the orthorhombic test (240 frames, 4 folds, coordinates in [1, 7)) in a
    truncated octahedron, every connected piece of the system (constraint groups and beads joined) moved by its own
    lattice vectors per frame, so the features are not the open ones (the scores without the cell differ: asserted).

    The cases.  With id features the fit is well conditioned (scores of 2e3, the forces' own scale) and the two routes
    agree to 2e-9: both images at edge 20, outer 8 (the orthorhombic test's).  WITHOUT id features this system's fit is
    ill conditioned whatever measures the distance -- scores of 1e7 to 2e9 -- and the gap between the routes is
    float64 summation order amplified: measured 7e-7 to 3.4e-6 with the OPEN kernels and 6.2e-6 under the
    orthorhombic box (8, 9, 10) on this very system, and 1.2e-5 at edge 20, outer 8, where the images reproduce the
    open displacements and the scores are the open ones to five digits (the moved float32 coordinates round
    differently, nothing else differs).  A bound of 1e-5 on that says nothing about the cell forms.  The gb-only
    featuriser is therefore tested as the orthorhombic test has it, with a basis that reaches every image distance
    (there half the cell's diagonal, 7.8 < outer 8; here all distances stay below 10.4 < outer 12, in a cell of edge
    30 whose safe_radius is 12.2): measured gaps 4e-9 to 1.8e-6."""
    from aggforce_amd import agg

    coords, forces, cons, cmat = base.open_test_system(T=240, seed=21)
    H, cell = cell_for("octahedron", edge, 240, False, images)
    assert cell.image_radius >= outer
    coords = C.move_pieces(coords.astype(np.float64), H, seed=5).astype(np.float32)
    cmap = LinearMap(cmat)
    gb = Curry(gb_feat, outer=outer, inner=0.0, n_basis=4, width=1.0, box=cell)
    feat = Multifeaturize([id_feat, gb] if with_id else [gb])
    grid = {"l2_regularization": [0.5, 10.0, 300.0]}
    calls = {"n": 0}
    real = agg._grid_cv_feat_reuse

    def counted(*a, **k):
        calls["n"] += 1
        out = real(*a, **k)
        assert out is not None
        return out

    def go(reuse, featurizer=feat):
        return agg.project_forces_grid_cv(grid, coords, forces, n_folds=4, rng=np.random.default_rng(3),
                                          reuse_gram=reuse, method_rng=np.random.default_rng(17), coord_map=cmap,
                                          constrained_inds=cons, method=qp_feat_linear_map, featurizer=featurizer,
                                          kbt=KBT, n_constraint_frames=6)

    agg._grid_cv_feat_reuse = counted
    try:
        fast, loop = go(True), go(False)
    finally:
        agg._grid_cv_feat_reuse = real
    assert calls["n"] == 1
    for key in loop["scores"]:
        assert fast["n_runs"][key] == loop["n_runs"][key] == 4
        print(key, f"score {loop['scores'][key]:.4e}, one-pass against loop: "
                   f"{abs(fast['scores'][key] - loop['scores'][key]) / abs(loop['scores'][key]):.2e}")
        assert abs(fast["scores"][key] - loop["scores"][key]) < 1e-5 * abs(loop["scores"][key]), key
        assert abs(fast["sds"][key] - loop["sds"][key]) < 1e-3 * abs(loop["sds"][key]) + 1e-6 * abs(loop["scores"][key]), key
    open_gb = Curry(gb_feat, outer=outer, inner=0.0, n_basis=4, width=1.0)
    blind = go(True, Multifeaturize([id_feat, open_gb] if with_id else [open_gb]))
    assert any(abs(blind["scores"][k] - fast["scores"][k]) > 1e-4 * abs(fast["scores"][k]) for k in fast["scores"])
    # a per-frame cell is refused up front
    per_frame = Cell(np.broadcast_to(H, (240, 3, 3)).copy(), images=images)
    with pytest.raises(ValueError, match="per-frame"):
        go(True, Multifeaturize([id_feat, Curry(gb_feat, outer=outer, n_basis=4, box=per_frame)]))


@pytest.mark.parametrize("images", IMAGES)
@pytest.mark.parametrize("per_frame", [False, True], ids=["cell", "cellT"])
@pytest.mark.parametrize("on_gpu", [True, False], ids=["kernels", "torch"])
def test_subfeat_jacobian_autograd_and_kernel_agree_under_a_cell(per_frame, on_gpu, images):
    """Check 6, float64, 1e-10 relative: gb_subfeat_jac(box=Cell) against torch.autograd of the collapsed
    gb_subfeat(box=Cell, collapse=True), and both against the ``grad`` of K.gb_channels under the cell's rows -- the
    system of the orthorhombic test with its groups anywhere in a skewed cell."""
    from aggforce_amd.qp.jaxfeat import gb_subfeat, gb_subfeat_jac

    T, N, G, nb = 5, 7, 5, 6
    rng = np.random.default_rng(51)
    H = 2.2 * (R.frame_cells(T) if per_frame else R.SKEW)
    cell = Cell(H, images=images)
    assert cell.image_radius >= 4.0
    Hf = C.frames_of(H, T)
    ids = np.array([0, 0, 1, 2, 2, 3, 4])
    centre = np.einsum("tgk,tkj->tgj", rng.random((T, G, 3)), Hf)
    pts_h = centre[:, ids, :] + 0.3 * rng.random((T, N, 3))
    cg_h = np.einsum("tgk,tkj->tgj", rng.random((T, 1, 3)), Hf)
    smear_h = orc.smear_matrix([{0, 1}, {3, 4}], N).astype(np.float64)
    device = "cuda" if on_gpu else "cpu"
    pts = torch.tensor(pts_h, dtype=F64, device=device, requires_grad=True)
    cg = torch.tensor(cg_h, dtype=F64, device=device)
    smear = torch.tensor(smear_h, dtype=F64, device=device)
    kw = dict(outer=4.0, inner=0.0, n_basis=nb, width=1.0, dist_power=0.5)
    n_ch = G - 1
    if not on_gpu:
        sm_pts = torch.einsum("tfd,cf->tcd", pts, smear)
        collapsed = gb_subfeat(sm_pts, cg, ids, n_ch, None, collapse=True, box=cell, **kw)
    else:
        collapsed = gb_subfeat(pts, cg, ids, n_ch, smear, collapse=True, box=cell, **kw)
    assert collapsed.shape == (n_ch * nb,)
    auto = torch.stack([torch.autograd.grad(collapsed[f], pts, retain_graph=True)[0].sum(dim=1) for f in range(n_ch * nb)],
                       dim=1)
    assert float(auto.abs().max()) > 0.1
    p_g, c_g, s_g = (x.detach().cuda() for x in (pts, cg, smear))
    jac = gb_subfeat_jac(p_g, c_g, ids, n_ch, smear_mat=s_g, box=cell, **kw)
    assert rel(jac.cpu().numpy(), auto.cpu().numpy()) < 1e-10
    if not on_gpu:  # the plain-torch route of the Jacobian itself (on the smeared points: both atoms of a group count)
        jac_h = gb_subfeat_jac(torch.einsum("tfd,cf->tcd", pts.detach(), smear), cg, ids, n_ch, box=cell, **kw)
        assert rel(jac_h.numpy(), auto.numpy()) < 1e-10
    order = [0, 2, 3, 5, 6]
    Pg = torch.einsum("tfd,cf->tcd", p_g, s_g)[:, order, :].contiguous()
    sizes = torch.tensor([2, 1, 2, 1, 1], dtype=F32, device="cuda")
    centers = torch.from_numpy(gb_centers(4.0, 0.0, nb, 0.5, np.float64)).cuda()
    gauss, grad = K.gb_channels(Pg, c_g.contiguous(), 0, sizes, n_ch, centers, 1.0, CLIP,
                                box=torch.from_numpy(C.rows(H, T)).cuda(), near=images == "nearest")
    assert rel(grad.reshape(T, n_ch * nb, 3).cpu().numpy(), auto.cpu().numpy()) < 1e-10
    per_site = gb_subfeat(p_g, c_g, ids, n_ch, s_g, box=cell, **kw)
    assert rel(per_site[:, order[:n_ch], :].reshape(T, n_ch, n_ch, nb)[:, range(n_ch), range(n_ch), :].cpu().numpy(),
               gauss.cpu().numpy()) < 1e-12
    open_jac = gb_subfeat_jac(p_g, c_g, ids, n_ch, smear_mat=s_g, **kw)
    assert rel(open_jac.cpu().numpy(), auto.cpu().numpy()) > 1e-2
    # differentiable beyond the first order on the kernel route
    if on_gpu:
        p2 = p_g.clone().requires_grad_(True)
        j2 = gb_subfeat_jac(p2, c_g, ids, n_ch, smear_mat=s_g, box=cell, **kw)
        (g2,) = torch.autograd.grad((j2 * j2).sum(), p2)
        assert bool(torch.isfinite(g2).all()) and float(g2.abs().max()) > 0


# ------------------------------------------------------------------ 7. the caller's stream
class GateCase:
    def __init__(self, name, families, build):
        self.name, self.group, self.entries, self.families = name, "feat_cell", (), tuple(families)
        self.build, self.synchronises, self.env, self.cleanup = build, None, None, None


def gate_cases():
    T, G, n_cg, nb = 9, 40, 3, 6
    Pg_h, cg_h, H = C.random_groups("octahedron", T, G, n_cg, True, seed=12)
    op = operands(Pg_h, cg_h, F64, F64, nb)
    cell_h = C.rows(H, T)
    ld = -(-(G + len(op["cols_h"])) // 128) * 128

    def build_of(fn):
        def build():
            return [dev(Pg_h, F64), dev(cg_h, F64), dev(op["Fg_h"], F64), dev(cell_h, F64)], fn
        return build

    def channels(Pg, cg, Fg, cell):
        return K.gb_channels(Pg, cg, 1, op["sizes"], op["n_ch"], op["centers"], 1.0, CLIP, box=cell, near=True)

    def regmat(Pg, cg, Fg, cell):
        R3 = torch.zeros((T, ld, 3), dtype=F64, device="cuda")
        return K.gb_regmat_cols(Fg, Pg, cg, 1, op["sizes"], G, op["cols"], op["centers"], 1.0, CLIP, KBT, R3, box=cell)

    def apply(Pg, cg, Fg, cell):
        return K.gb_apply(Fg, Pg, cg, op["sizes"], G, op["n_ch"], op["centers"], 1.0, CLIP, op["coef"], box=cell, near=True)

    def apply_cols(Pg, cg, Fg, cell):
        return K.gb_apply_cols(Fg, Pg, cg, op["sizes"], G, op["centers"], 1.0, CLIP, op["compact"], box=cell)

    def build_range():
        return [dev(Pg_h, F32), dev(cg_h, F32), dev(cell_h, F32)], lambda Pg, cg, cell: K.gb_distance_range(
            Pg, cg, op["n_ch"], box=cell, near=True)

    return [GateCase("cell_gb_channels", ["gb_channels_pbc_kernel<double, 3>"], build_of(channels)),
            GateCase("cell_gb_regmat_cols", ["gb_regmat_cols_pbc_kernel<double, double, double, 2>"], build_of(regmat)),
            GateCase("cell_gb_apply", ["gb_apply_pbc_kernel<double, double, 3>"], build_of(apply)),
            GateCase("cell_gb_apply_cols", ["gb_apply_cols_pbc_kernel<double, double, 2>"], build_of(apply_cols)),
            GateCase("cell_gb_distance_range", ["gb_range_pbc_kernel<3>"], build_range)]


def test_the_cell_forms_of_the_feature_kernels_run_on_the_callers_stream_and_never_wait(monkeypatch):
    """Check 7: the method of tests/test_gpu_streams.py (tests/stream_gate.py) on the five new entry points: behind a
    gate that holds the caller's stream the calls return at once, and their results are those of the true data, not of
    the poison."""
    SG.run_behind_gate(gate_cases(), monkeypatch)
