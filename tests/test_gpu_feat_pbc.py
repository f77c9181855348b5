"""GPU: minimum-image distances in gb_feat -- the box forms of the K4 kernels, gb_feat(box=), the fused fit, the
one-pass cross-validation and the fitted map's application under an orthorhombic periodic box.

Two kinds of evidence.  (1) Exact: on the dyadic inputs of tests/featpbc_cases.py a shift by box vectors is undone by
the wrap bit for bit, so every box kernel on shifted input must reproduce the open kernel on the unshifted input with
no tolerance at all.  (2) Genuinely different images: against NumPy float64 d - L rint(d / L) on the host, put through
the oracle's own Gaussian and derivative expressions (``orc.gb_feat_site``), to the tolerances of the open path's
``test_gb_feat_dense_matches_oracle`` (2e-6 features, 2e-5 divergences, float32).  The constructions themselves are
checked on the CPU in tests/test_feat_pbc_host.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import featpbc_cases as cases  # noqa: E402
from aggforce_amd import LinearMap, Trajectory, project_forces  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd.qp import Multifeaturize, gb_feat, id_feat, qp_feat_linear_map  # noqa: E402
from aggforce_amd.qp.gbfeat import CLIP, gb_centers  # noqa: E402
from aggforce_amd.util import Curry  # noqa: E402
from oracle import aggforce_oracle as orc  # noqa: E402

KBT = 0.6955215
TOL_FEAT, TOL_DIV = 2e-6, 2e-5  # test_gpu_feat.py::test_gb_feat_dense_matches_oracle, float32
F32, F64 = torch.float32, torch.float64


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def kernel_operands(Pg, cg, box, tf, tg, n_basis, seed, outer=6.0):
    """What the five kernels take besides positions: group sizes (a few two-atom groups), group force sums, centres,
    a kept-column list, coefficients with zeros (dense and compact) -- G channels, n_id = G."""
    rng = np.random.default_rng(seed)
    T, G, _ = Pg.shape
    n_cg = cg.shape[1]
    sizes_h = np.ones(G, dtype=np.float32)
    sizes_h[[1, 4, G - 2]] = 2.0
    n_ch = G - 1  # (the reference's dropped last channel)
    coef = rng.standard_normal((n_cg, G + n_ch * n_basis)) * (rng.random((n_cg, G + n_ch * n_basis)) < 0.5)
    coef[0, G + 2 * n_basis:G + 3 * n_basis] = 0.0  # a channel none of whose columns is kept
    coef[n_cg - 1, G:] = 0.0                         # a site without Gaussian coefficients
    cols_h = np.flatnonzero(rng.random(n_ch * n_basis) < 0.6).astype(np.int32)
    return dict(T=T, G=G, n_cg=n_cg, n_ch=n_ch, n_basis=n_basis, sizes_h=sizes_h, coef_h=coef, cols_h=cols_h,
                Fg_h=(20 * rng.standard_normal((T, G, 3))).astype(np.float32).astype(np.float64),
                sizes=torch.from_numpy(sizes_h).cuda(),
                centers=torch.from_numpy(gb_centers(outer, 0.0, n_basis, 0.5, np.float32 if tg == F32 else np.float64)).cuda(),
                coef=dev(coef, F64), compact=K.gb_compact_coefficients(coef, G, "cuda"), cols=torch.from_numpy(cols_h).cuda(),
                Pg=dev(Pg, tg), cg=dev(cg, tg), box=None if box is None else dev(box, tg), tf=tf, tg=tg)


def run_kernels(op, Pg, box, out_dtype, Fg=None):
    """(gauss, grad, R3, applied, applied from the compact list, rmin, rmax) of all sites, open (box None) or boxed."""
    Fg = dev(op["Fg_h"], op["tf"]) if Fg is None else Fg
    G, n_ch, cen = op["G"], op["n_ch"], op["centers"]
    ld = -(-(G + len(op["cols_h"])) // 128) * 128
    gauss, grad, R3s = [], [], []
    for site in range(op["n_cg"]):
        g, d = K.gb_channels(Pg, op["cg"], site, op["sizes"], n_ch, cen, 1.0, CLIP, box=box)
        R3 = torch.zeros((op["T"], ld, 3), dtype=out_dtype, device="cuda")
        K.gb_regmat_cols(Fg, Pg, op["cg"], site, op["sizes"], G, op["cols"], cen, 1.0, CLIP, KBT, R3, box=box)
        gauss.append(g), grad.append(d), R3s.append(R3)
    app = K.gb_apply(Fg, Pg, op["cg"], op["sizes"], G, n_ch, cen, 1.0, CLIP, op["coef"], box=box)
    app_c = K.gb_apply_cols(Fg, Pg, op["cg"], op["sizes"], G, cen, 1.0, CLIP, op["compact"], box=box)
    rmin, rmax = K.gb_distance_range(Pg, op["cg"], n_ch, box=box)
    return torch.stack(gauss), torch.stack(grad), torch.stack(R3s), app, app_c, rmin, rmax


# (force dtype, feature dtype, regression-matrix dtype): the five combinations of the dispatch; the fused fit never
# takes a float32 regression matrix, the first row calls the kernel with one
DTYPES = [(F32, F32, F32), (F32, F32, F64), (F64, F32, F64), (F32, F64, F64), (F64, F64, F64)]
# 7 frames: not a multiple of the apply kernels' 4-frame block; 75 groups: the lanes stride past 64 channels;
# n_basis 10: past the 8 coefficients held in registers
SHAPES = [(7, 20, 3, 4), (7, 75, 2, 10)]


@pytest.mark.parametrize("per_frame", [False, True], ids=["box3", "boxT3"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", SHAPES)
@pytest.mark.parametrize("tf,tg,to", DTYPES, ids=["fff", "ffd", "dfd", "fdd", "ddd"])
def test_box_kernels_undo_a_shift_by_box_vectors_bit_for_bit(tf, tg, to, T, G, n_cg, n_basis, per_frame):
    """Check 1: gb_channels, gb_regmat_cols, gb_apply, gb_apply_cols and gb_distance_range with a box, on group
    means moved by their own box vectors (each frame's own lengths), equal the open kernels on the unmoved means:
    torch.equal, no tolerance."""
    Pg, cg, box, Pg_s = cases.dyadic_groups(T, G, n_cg, per_frame, seed=5)
    op = kernel_operands(Pg, cg, box, tf, tg, n_basis, seed=9)
    open_ = run_kernels(op, op["Pg"], None, to)
    boxed = run_kernels(op, dev(Pg_s, tg), op["box"], to)
    moved_open = run_kernels(op, dev(Pg_s, tg), None, to)
    names = ("gauss", "grad", "regmat", "apply", "apply_cols", "rmin", "rmax")
    for name, a, b, c in zip(names, open_, boxed, moved_open):
        assert torch.isfinite(a).all() or name == "rmin", name  # (rmin stays +inf at the dropped last channel)
        assert torch.equal(a, b), name
        assert not torch.equal(a, c), name  # (the shift is seen by the open kernels: the box did the work)
    assert float(open_[0].abs().max()) > 0.1 and float(open_[6].max()) < 7.0


def host_oracle(op, Pg, cg, box):
    """float64 on the host: d - L rint(d / L), then the oracle's Gaussians and derivatives (one group per atom,
    identity smear: the kernel's channels), the regression matrix columns and the applied map built from them."""
    d_mi, share, near_tie = cases.image_statistics(Pg, cg, box)
    T, G, n_ch, nb = op["T"], op["G"], op["n_ch"], op["n_basis"]
    gauss = np.zeros((op["n_cg"], T, n_ch, nb))
    grad = np.zeros((op["n_cg"], T, n_ch, nb, 3))
    for site in range(op["n_cg"]):
        feats, divs = orc.gb_feat_site(cg[:, site, None, :] + d_mi[:, site], cg[:, site], np.arange(G), np.eye(G),
                                       outer=6.0, inner=0.0, n_basis=nb, width=1.0, dist_power=0.5, clip=CLIP,
                                       n_channels=n_ch, dtype=np.float64)
        ch = np.arange(n_ch)
        gauss[site] = feats.reshape(T, G, n_ch, nb)[:, ch, ch, :]
        grad[site] = op["sizes_h"][None, :n_ch, None, None] * divs.reshape(T, n_ch, nb, 3)
    F = op["Fg_h"]
    full = gauss[..., None] * F[None, :, :n_ch, None, :]                       # (n_cg, T, n_ch, nb, 3)
    regmat = (full + KBT * grad).reshape(op["n_cg"], T, n_ch * nb, 3)[:, :, op["cols_h"], :]
    c_id, c_gb = op["coef_h"][:, :G], op["coef_h"][:, G:].reshape(op["n_cg"], n_ch, nb)
    applied = np.einsum("cg,tgd->tcd", c_id, F) + np.einsum("cgk,ctgkd->tcd", c_gb, full + grad)
    return gauss, grad, regmat, applied, share, near_tie


@pytest.mark.parametrize("per_frame", [False, True], ids=["box3", "boxT3"])
@pytest.mark.parametrize("T,G,n_cg,n_basis", SHAPES)
@pytest.mark.parametrize("tg", [F32, F64], ids=["f32", "f64"])
def test_box_kernels_match_float64_minimum_images_on_the_host(tg, T, G, n_cg, n_basis, per_frame):
    """Check 2: group means and sites spread over the whole cell (at least a quarter of the (frame, site, group)
    triples have a component beyond half a box length: asserted), against the host's float64 minimum images and the
    oracle's Gaussian expressions.  Features to 2e-6 and divergences to 2e-5, the open path's tolerances; triples within
    1e-3 of a tie in d / L (under 1 %: asserted) are left out, there float32 and float64 may round to different
    images.  The regression matrix g F + kbt div and the applied map sum_f coef (g F + div) are held to what those
    two tolerances imply for their sums (plus float32 rounding of the products), nothing wider."""
    Pg, cg, box = cases.random_groups(T, G, n_cg, per_frame, seed=11 if G == 20 else 12)
    op = kernel_operands(Pg, cg, box, F32, tg, n_basis, seed=9)
    gauss_o, grad_o, reg_o, app_o, share, near_tie = host_oracle(op, Pg, cg, box)
    assert share >= 0.25 and near_tie.mean() < 0.01
    ok = ~np.transpose(near_tie, (1, 0, 2))[:, :, :op["n_ch"]]                 # (n_cg, T, n_ch)
    gauss, grad, R3, app, app_c, rmin, rmax = (x.cpu().numpy().astype(np.float64) for x in
                                                run_kernels(op, op["Pg"], op["box"], F64))
    open_gauss = run_kernels(op, op["Pg"], None, F64)[0].cpu().numpy()
    assert np.abs(open_gauss - gauss_o)[ok].max() > 0.05                       # the images really differ
    err_f, err_d = np.abs(gauss - gauss_o)[ok].max(), np.abs(grad - grad_o)[ok].max()
    print(f"features {err_f:.2e} (tol {TOL_FEAT}), divergences {err_d:.2e} (tol {TOL_DIV})")
    assert err_f < TOL_FEAT and err_d < TOL_DIV
    # regression matrix columns (id block = the force sums, exactly)
    Fmax = np.abs(op["Fg_h"]).max()
    nid = op["G"]
    assert np.array_equal(R3[:, :, :nid, :], np.broadcast_to(op["Fg_h"], (n_cg,) + op["Fg_h"].shape))
    ok_cols = np.repeat(ok, n_basis, axis=2)[:, :, op["cols_h"]]
    got = R3[:, :, nid:nid + len(op["cols_h"]), :]
    bound_reg = TOL_FEAT * Fmax + KBT * TOL_DIV + 4 * 2.0 ** -24 * np.abs(reg_o).max()
    err_r = np.abs(got - reg_o)[ok_cols].max()
    print(f"regression matrix {err_r:.2e} (bound {bound_reg:.2e})")
    assert err_r < bound_reg
    # the applied map: frames and sites none of whose channels is near a tie
    clean = np.transpose(ok.all(axis=2))                                       # (T, n_cg)
    assert clean.mean() > 0.3
    weight = np.abs(op["coef_h"][:, nid:]).sum(axis=1).max()
    bound_app = weight * (TOL_FEAT * Fmax + TOL_DIV)
    err_a, err_c = np.abs(app - app_o)[clean].max(), np.abs(app_c - app_o)[clean].max()
    print(f"applied {err_a:.2e}, from the compact list {err_c:.2e} (bound {bound_app:.2e})")
    assert err_a < bound_app and err_c < bound_app
    assert rel(app_c, app) < 1e-12                                             # bit-identical terms, order of the sums
    # the range: that of the minimum-image distances, within half the cell's diagonal
    r_o = np.linalg.norm(cases.image_statistics(Pg, cg, box)[0], axis=-1)      # (T, n_cg, G)
    n_ch = op["n_ch"]
    assert np.abs(rmin[:, :n_ch] - r_o.min(axis=0)[:, :n_ch]).max() < 1e-5
    assert np.abs(rmax[:, :n_ch] - r_o.max(axis=0)[:, :n_ch]).max() < 1e-5
    assert rmax[:, :n_ch].max() <= 0.5 * np.linalg.norm(box.max(axis=0) if per_frame else box) * (1 + 1e-6)


def test_a_bad_box_length_poisons_its_frame_and_no_other():
    """A NaN, zero, negative or infinite length in one frame of a box on the device: that frame's features, Gaussian
    regression columns and applied rows are NaN, every other frame is bit for bit what a good box gives, and the
    distance range of every channel spans everything."""
    Pg, cg, box = cases.random_groups(7, 20, 3, True, seed=11)
    op = kernel_operands(Pg, cg, box, F32, F32, 4, seed=9)
    good = run_kernels(op, op["Pg"], op["box"], F64)
    for frame, comp, value in ((3, 1, float("nan")), (0, 0, 0.0), (6, 2, -4.0), (5, 0, float("inf"))):
        bad_box = op["box"].clone()
        bad_box[frame, comp] = value
        bad = run_kernels(op, op["Pg"], bad_box, F64)
        others = [t for t in range(7) if t != frame]
        nid = op["G"]
        for name, a, b in zip(("gauss", "grad"), good[:2], bad[:2]):
            assert torch.isnan(b[:, frame]).all() and torch.equal(a[:, others], b[:, others]), name
        assert torch.isnan(bad[2][:, frame, nid:nid + len(op["cols_h"])]).all()
        assert torch.equal(bad[2][:, frame, :nid], good[2][:, frame, :nid])   # the id block holds no distance
        assert torch.equal(bad[2][:, others], good[2][:, others])
        for a, b in zip(good[3:5], bad[3:5]):
            assert torch.isnan(b[frame]).all() and torch.equal(a[others], b[others])
        n_ch = op["n_ch"]
        assert (bad[5][:, :n_ch] == 0).all() and torch.isinf(bad[6][:, :n_ch]).all()
    # through gb_feat: a box that lives on the device is not read on the host
    U, forces, box, wrapped, moved = cases.dyadic_molecules(7, True, seed=3)
    dbox = torch.from_numpy(box).cuda()
    dbox[2, 0] = float("nan")
    cmap = LinearMap(orc.list_mapping_matrix(cases.BEADS, cases.N_ATOMS))
    res = gb_feat(moved.astype(np.float32), cmap, cases.CONS, outer=6.0, n_basis=4, lazy=False, box=dbox)
    ref = gb_feat(U.astype(np.float32), cmap, cases.CONS, outer=6.0, n_basis=4, lazy=False)
    keep = [0, 1, 3, 4, 5, 6]
    for c in range(4):
        assert np.isnan(res["divs"][c][2]).all() and np.array_equal(res["divs"][c][keep], ref["divs"][c][keep])
        assert np.array_equal(res["feats"][c][keep], ref["feats"][c][keep])


# ------------------------------------------------------------------ public level


def molecule_oracle(U, n_basis, outer=6.0):
    ids = orc.id_feat_ids(cases.N_ATOMS, cases.CONS)
    smear = orc.smear_matrix(orc.reduce_constraint_sets(cases.CONS), cases.N_ATOMS)
    cmat = orc.list_mapping_matrix(cases.BEADS, cases.N_ATOMS)
    cgs = orc.linearmap_apply(U, cmat)
    return [orc.gb_feat_site(U, cgs[:, c, :], ids, smear, outer=outer, inner=0.0, n_basis=n_basis, width=1.0,
                             dist_power=0.5, n_channels=int(ids.max())) for c in range(4)]


@pytest.mark.parametrize("per_frame", [False, True], ids=["box3", "boxT3"])
def test_gb_feat_with_a_box_matches_the_oracle_on_the_unwrapped_trajectory(per_frame):
    """Check 3: whole molecules moved by box vectors, constraint groups of one and two atoms, two-atom beads; with
    ``box=`` gb_feat gives what the oracle gives on the compact trajectory (2e-6 / 2e-5) -- and, the inputs being
    dyadic, exactly what gb_feat gives there without a box; without ``box=`` it does not."""
    U, forces, box, wrapped, moved = cases.dyadic_molecules(7, per_frame, seed=3)
    cmap = LinearMap(orc.list_mapping_matrix(cases.BEADS, cases.N_ATOMS))
    kw = dict(outer=6.0, inner=0.0, n_basis=5, width=1.0, dist_power=0.5, lazy=False)
    res = gb_feat(moved.astype(np.float32), cmap, cases.CONS, box=box, **kw)
    same = gb_feat(U.astype(np.float32), cmap, cases.CONS, **kw)
    openf = gb_feat(moved.astype(np.float32), cmap, cases.CONS, **kw)
    lazy = gb_feat(moved.astype(np.float32), cmap, cases.CONS, box=torch.from_numpy(box), **dict(kw, lazy=True))
    ref = molecule_oracle(U.astype(np.float32), 5)
    for c, (f_o, d_o) in enumerate(ref):
        f, d = res["feats"][c], res["divs"][c]
        assert f.dtype == np.float32 and f.shape == f_o.shape and d.shape == d_o.shape
        assert np.max(np.abs(f - f_o)) < TOL_FEAT and np.max(np.abs(d - d_o)) < TOL_DIV
        assert np.array_equal(f, same["feats"][c]) and np.array_equal(d, same["divs"][c])
        assert np.max(np.abs(openf["feats"][c] - f_o)) > 0.05
    assert np.array_equal(next(iter(lazy["feats"])), res["feats"][0])


def _fit_kwargs(T, n_basis=4, seed=3):
    rng = np.random.default_rng(seed)
    return dict(kbt=KBT, frame_indices=[rng.choice(T, size=6, replace=False) for _ in range(4)], l2_regularization=10.0)


@pytest.mark.parametrize("per_frame", [False, True], ids=["box3", "boxT3"])
def test_project_forces_on_a_wrapped_trajectory_matches_the_unwrapped_one(per_frame):
    """Check 3, through project_forces: atoms wrapped into the cell (molecules split over faces), ``box=`` and
    ``bonds=`` to make them whole, the box bound in the featuriser -- against the compact trajectory without any box:
    coefficients and mapped forces to 2e-4 (the fused/dense tolerance of the open path).  Without the box in the
    featuriser the fit is a different one.  This is the test that fails without the feature: ``gb_feat`` had no
    ``box``."""
    T = 48
    U, forces, box, wrapped, moved = cases.dyadic_molecules(T, per_frame, seed=3)
    U32, W32, F32h = U.astype(np.float32), wrapped.astype(np.float32), forces.astype(np.float32)
    cmap = LinearMap(orc.list_mapping_matrix(cases.BEADS, cases.N_ATOMS))
    gbkw = dict(outer=6.0, inner=0.0, n_basis=4, width=1.0)
    fit = _fit_kwargs(T)
    ref = project_forces(U32, F32h, cmap, constrained_inds=cases.CONS, method=qp_feat_linear_map,
                         featurizer=Multifeaturize([id_feat, Curry(gb_feat, **gbkw)]), **fit)
    got = project_forces(W32, F32h, cmap, constrained_inds=cases.CONS, method=qp_feat_linear_map, box=box,
                         bonds=cases.BONDS, featurizer=Multifeaturize([id_feat, Curry(gb_feat, box=box, **gbkw)]), **fit)
    blind = project_forces(W32, F32h, cmap, constrained_inds=cases.CONS, method=qp_feat_linear_map, box=box,
                           bonds=cases.BONDS, featurizer=Multifeaturize([id_feat, Curry(gb_feat, **gbkw)]), **fit)
    coef = lambda r: np.stack(r["tmap"].force_map.tags["coef_list"])
    assert rel(coef(got), coef(ref)) < 2e-4 and rel(got["mapped_forces"], ref["mapped_forces"]) < 2e-4
    assert rel(coef(blind), coef(ref)) > 1e-3 and rel(blind["mapped_forces"], ref["mapped_forces"]) > 1e-3
    # mapped coordinates: those of the whole molecules, i.e. the compact ones up to box vectors
    rows = box[:, None, :] if per_frame else box[None, None, :]
    shift = (got["mapped_coords"] - ref["mapped_coords"]) / rows
    assert np.array_equal(shift, np.rint(shift))
    assert got["tmap"].force_map.tags["fit_info"]["kept_columns"] == ref["tmap"].force_map.tags["fit_info"]["kept_columns"]


# ------------------------------------------------------------------ fused against dense, compaction, cross-validation


@pytest.mark.parametrize("per_frame", [False, True], ids=["box3", "boxT3"])
def test_fused_fit_matches_the_dense_path_with_a_box(per_frame):
    """Check 4: qp_feat_linear_map fused and dense with the same sampled frames and the same bound box (random
    coordinates over the whole cell, so most distances are through a face): coefficients and mapped forces to 2e-4,
    as the open test; the fitted map applies to other trajectories with a (3,) box and to trajectories of the fit's
    own length with a per-frame one, and refuses any other length."""
    T, N = 60, 16
    rng = np.random.default_rng(31)
    box = np.array([5.0, 6.5, 8.0]) if not per_frame else np.array([5.0, 6.5, 8.0]) + 1.5 * rng.random((T, 3))
    rows = box[:, None, :] if per_frame else box[None, None, :]
    # whole molecules of 4 atoms (bond length ~0.5) anywhere in the cell
    coords = (rng.random((T, 4, 1, 3)) * rows[:, :, None, :] + 0.5 * rng.random((T, 4, 4, 3))).reshape(T, N, 3).astype(np.float32)
    forces = (25 * rng.standard_normal((T, N, 3))).astype(np.float32)
    cmap = LinearMap(orc.list_mapping_matrix(cases.BEADS, N))
    smear = orc.smear_matrix(orc.reduce_constraint_sets(cases.CONS), N).astype(np.float64)
    _, share, _ = cases.image_statistics(np.einsum("tfd,cf->tcd", coords.astype(np.float64), smear),
                                         orc.linearmap_apply(coords.astype(np.float64), cmap.standard_matrix), box)
    assert share >= 0.25
    feat = Multifeaturize([id_feat, Curry(gb_feat, outer=3.0, inner=0.0, n_basis=4, width=0.5, box=box)])
    traj = Trajectory(coords=coords, forces=forces)
    fit = _fit_kwargs(T)
    kbt = fit.pop("kbt")
    fused = qp_feat_linear_map(traj, cmap, feat, kbt, constraints=cases.CONS, **fit)
    dense = qp_feat_linear_map(traj, cmap, feat, kbt, constraints=cases.CONS, fused=False, **fit)
    cf, cd = np.stack(fused.force_map.tags["coef_list"]), np.stack(dense.force_map.tags["coef_list"])
    assert rel(cf, cd) < 2e-4
    assert rel(fused(traj).forces, dense(traj).forces) < 2e-4
    info = fused.force_map.tags["fit_info"]
    assert max(info["kept_columns"]) < info["n_feat"]  # (outer 3.0 + reach is short of the cell: columns were dropped)
    # application to other frames
    other = Trajectory(coords=coords[:11], forces=forces[:11])
    if per_frame:
        for m in (fused, dense):
            with pytest.raises(ValueError, match="box"):
                m(other)
    else:
        assert rel(fused(other).forces, fused(traj).forces[:11]) < 1e-12
        assert rel(dense(other).forces, dense(traj).forces[:11]) < 1e-6


def open_test_system(T, N=14, seed=0):
    """tests/test_gpu_feat.py::system: the systems the open tests' tolerances were set on."""
    rng = np.random.default_rng(seed)
    coords = (6 * rng.random((T, N, 3)) + 1).astype(np.float32)
    forces = (25 * rng.standard_normal((T, N, 3))).astype(np.float32)
    cons = {frozenset([1, 2]), frozenset([4, 5]), frozenset([5, 6]), frozenset([10, 13])}
    cmat = orc.list_mapping_matrix([[0, 1], [4, 7], [8, 10], [12, 13]], N)
    return coords, forces, cons, cmat


@pytest.mark.parametrize("per_frame", [False, True], ids=["box3", "boxT3"])
def test_zero_column_compaction_is_exact_with_a_box(per_frame, monkeypatch):
    """Check 4: column compaction on and off give the same coefficients and mapped forces under a box, to the 1e-7 of
    test_zero_column_compaction_is_exact -- on that test's own system (two clusters 40 apart, one sampled frame per
    site), inside a cell whose nearest images keep the clusters 24 or more apart, with the second cluster moved by
    its own box vectors in every frame: the kept columns are decided by the range of MINIMUM-IMAGE distances (by open
    distances nothing of the far cluster could be dropped and everything of the near one would be)."""
    from aggforce_amd.qp import gbfeat

    rng = np.random.default_rng(21)
    T, N = 80, 24
    base = np.concatenate([3.0 * rng.random((N // 2, 3)), 3.0 * rng.random((N // 2, 3)) + 40.0])
    coords = base[None] + 0.2 * rng.standard_normal((T, N, 3))
    forces = (25 * rng.standard_normal((T, N, 3))).astype(np.float32)
    box = np.array([64.0, 72.0, 96.0]) if not per_frame else np.array([64.0, 72.0, 96.0]) + 4.0 * rng.random((T, 3))
    rows = box[:, None, :] if per_frame else box[None, None, :]
    coords[:, N // 2:] += rng.integers(-1, 2, size=(T, 1, 3)) * rows
    coords = coords.astype(np.float32)
    cons = {frozenset([1, 2]), frozenset([13, 14]), frozenset([14, 15]), frozenset([20, 23])}
    cmap = LinearMap(orc.list_mapping_matrix([[0, 1], [4, 7], [12, 13], [18, 22]], N))
    feat = Multifeaturize([id_feat, Curry(gb_feat, outer=6.0, inner=0.0, n_basis=5, width=1.0, box=box)])
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
    for c in range(4):  # dropped columns: exact zeros; the near cluster's columns are in use
        dead = np.setdiff1d(np.arange(info["n_feat"] - G), info["kept_gauss_columns"][c])
        assert len(dead) > 0 and np.all(cs[c, G + dead] == 0.0) and np.abs(cs[c, G:]).max() > 0


@pytest.mark.parametrize("with_id", [True, False])
def test_featurised_grid_cv_one_pass_matches_the_loop_with_a_box(with_id):
    """Check 4: project_forces_grid_cv with a (3,) box bound in the featuriser: the one-pass scores equal the
    loop's, to the tolerance of test_featurised_grid_cv_one_pass_matches_the_loop (1e-5; sds 1e-3) -- on that test's
    own system (240 frames, 4 folds, coordinates in [1, 7)), in a cell of (8, 9, 10): displacements beyond 4, 4.5 and 5
    have a nearer image, so the features are not the open ones (the scores without the box differ: asserted)."""
    from aggforce_amd import agg

    coords, forces, cons, cmat = open_test_system(T=240, seed=21)
    box = np.array([8.0, 9.0, 10.0])
    cmap = LinearMap(cmat)
    gb = Curry(gb_feat, outer=8.0, inner=0.0, n_basis=4, width=1.0, box=box)
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
        print(key, f"one-pass against loop: {abs(fast['scores'][key] - loop['scores'][key]) / abs(loop['scores'][key]):.2e}")
        assert abs(fast["scores"][key] - loop["scores"][key]) < 1e-5 * abs(loop["scores"][key]), key
        assert abs(fast["sds"][key] - loop["sds"][key]) < 1e-3 * abs(loop["sds"][key]) + 1e-6 * abs(loop["scores"][key]), key
    open_gb = Curry(gb_feat, outer=8.0, inner=0.0, n_basis=4, width=1.0)
    blind = go(True, Multifeaturize([id_feat, open_gb] if with_id else [open_gb]))
    assert any(abs(blind["scores"][k] - fast["scores"][k]) > 1e-4 * abs(fast["scores"][k]) for k in fast["scores"])


# ------------------------------------------------------------------ the array functions


@pytest.mark.parametrize("per_frame", [False, True], ids=["box3", "boxT3"])
@pytest.mark.parametrize("on_gpu", [True, False], ids=["kernels", "torch"])
def test_subfeat_jacobian_autograd_and_kernel_agree_under_a_box(per_frame, on_gpu):
    """Check 5, float64, 1e-10 relative: gb_subfeat_jac(box=) against torch.autograd of the collapsed
    gb_subfeat(box=, collapse=True) (per frame: the gradient summed over the atoms), and both against the ``grad``
    of K.gb_channels(box=) -- which carries the group size, as 'reorder' with the group-mean smear does."""
    from aggforce_amd.qp.jaxfeat import gb_subfeat, gb_subfeat_jac

    T, N, G, nb = 5, 7, 5, 6
    rng = np.random.default_rng(51)
    box = np.array([4.0, 5.0, 6.0]) if not per_frame else np.array([4.0, 5.0, 6.0]) + rng.random((T, 3))
    rows = box[:, None, :] if per_frame else box[None, None, :]
    ids = np.array([0, 0, 1, 2, 2, 3, 4])
    # atoms of a group stay together (whole groups), the groups are anywhere in the cell
    centre = rng.random((T, G, 3)) * rows
    pts_h = centre[:, ids, :] + 0.3 * rng.random((T, N, 3))
    cg_h = rng.random((T, 1, 3)) * rows
    smear_h = orc.smear_matrix([{0, 1}, {3, 4}], N).astype(np.float64)
    device = "cuda" if on_gpu else "cpu"
    pts = torch.tensor(pts_h, dtype=F64, device=device, requires_grad=True)
    cg = torch.tensor(cg_h, dtype=F64, device=device)
    smear = torch.tensor(smear_h, dtype=F64, device=device)
    kw = dict(outer=4.0, inner=0.0, n_basis=nb, width=1.0, dist_power=0.5)
    n_ch = G - 1
    if not on_gpu:  # (the smear step runs on the device: smear on the host for the plain-torch route)
        sm_pts = torch.einsum("tfd,cf->tcd", pts, smear)
        collapsed = gb_subfeat(sm_pts, cg, ids, n_ch, None, collapse=True, box=box, **kw)
    else:
        collapsed = gb_subfeat(pts, cg, ids, n_ch, smear, collapse=True, box=box, **kw)
    assert collapsed.shape == (n_ch * nb,)
    auto = torch.stack([torch.autograd.grad(collapsed[f], pts, retain_graph=True)[0].sum(dim=1) for f in range(n_ch * nb)],
                       dim=1)                                                   # (T, n_feat, 3)
    assert float(auto.abs().max()) > 0.1
    p_g, c_g, s_g = (x.detach().cuda() for x in (pts, cg, smear))
    jac = gb_subfeat_jac(p_g, c_g, ids, n_ch, smear_mat=s_g, box=box, **kw)
    assert rel(jac.cpu().numpy(), auto.cpu().numpy()) < 1e-10
    # the K4 kernel on the group means
    order = [0, 2, 3, 5, 6]  # one atom of each group
    Pg = torch.einsum("tfd,cf->tcd", p_g, s_g)[:, order, :].contiguous()
    sizes = torch.tensor([2, 1, 2, 1, 1], dtype=F32, device="cuda")
    centers = torch.from_numpy(gb_centers(4.0, 0.0, nb, 0.5, np.float64)).cuda()
    gauss, grad = K.gb_channels(Pg, c_g.contiguous(), 0, sizes, n_ch, centers, 1.0, CLIP, box=torch.from_numpy(box).cuda())
    assert rel(grad.reshape(T, n_ch * nb, 3).cpu().numpy(), auto.cpu().numpy()) < 1e-10
    per_site = gb_subfeat(p_g, c_g, ids, n_ch, s_g, box=box, **kw)               # (T, N, n_feat)
    assert rel(per_site[:, order[:n_ch], :].reshape(T, n_ch, n_ch, nb)[:, range(n_ch), range(n_ch), :].cpu().numpy(),
               gauss.cpu().numpy()) < 1e-12
    open_jac = gb_subfeat_jac(p_g, c_g, ids, n_ch, smear_mat=s_g, **kw)
    assert rel(open_jac.cpu().numpy(), auto.cpu().numpy()) > 1e-2                # the box matters on these inputs
