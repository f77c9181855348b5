"""Triclinic cells on the host: ``pbc.Cell`` (validation, refusals, ``from_lengths_angles``), the meaning raw arrays
keep, the reference of tests/cell_ref.py against a brute-force minimum image, and the host bodies of every function
that takes ``box=Cell`` -- ``pair_distances``, ``distances_in_box``, ``min_distances``, ``PairList.from_cutoff``,
``make_whole``, ``guess_pairwise_constraints`` -- against that reference and, for a diagonal cell, against their box
forms bit for bit.  No GPU."""
import numpy as np
import pytest
import torch

import aggforce_amd
import cell_ref as R
from aggforce_amd import Cell, guess_pairwise_constraints, make_whole, project_forces
from aggforce_amd import pbc
from aggforce_amd.agg import project_forces_grid_cv
from aggforce_amd.jaxutil import PairList, _as_box, distances_in_box, min_distances, pair_distances
from aggforce_amd.pbc import MoleculeTree
from pairlist_ref import lattice_sites, list_disp, random_list, triangle
from test_pbc_host import GC

KINDS = R.KINDS


# ------------------------------------------------------------------ 1. Cell
def test_cell_is_exported_and_holds_what_it_was_given():
    assert aggforce_amd.Cell is pbc.Cell and "Cell" in aggforce_amd.__all__
    c = Cell(R.SKEW)
    assert not c.is_per_frame and tuple(c.vectors.shape) == (3, 3) and c.vectors.dtype == torch.float64
    assert np.array_equal(c.vectors.numpy(), R.SKEW)
    assert isinstance(c.safe_radius, float) and c.safe_radius == 4.1 / 2
    f = Cell(R.frame_cells(5))
    assert f.is_per_frame and tuple(f.vectors.shape) == (5, 3, 3)
    assert f.safe_radius == float(R.frame_cells(5)[:, 0, 0].min()) / 2  # (over all frames)
    for given in (R.SKEW.tolist(), torch.tensor(R.SKEW), torch.tensor(R.SKEW, dtype=torch.float32), R.SKEW.astype(int)):
        assert tuple(Cell(given).vectors.shape) == (3, 3)
    assert tuple(Cell(R.SKEW).rows(4).shape) == (4, 9) and np.array_equal(Cell(R.SKEW).rows(4)[2].numpy(), R.SKEW.ravel())
    assert np.array_equal(f.rows(5).numpy(), R.frame_cells(5).reshape(5, 9))
    assert np.array_equal(f.take([3, 1]).vectors.numpy(), R.frame_cells(5)[[3, 1]]) and Cell(R.SKEW).take([0]).vectors.shape == (3, 3)


@pytest.mark.parametrize("bad,why", [
    (np.ones(3), "shape"), (np.ones((3, 2)), "shape"), (np.ones((2, 2, 3, 3)), "shape"), (np.ones((4, 9)), "shape"),
    ([["a", 0, 0], [0, 1, 0], [0, 0, 1]], "numbers"), (None, "numbers|shape"),
    ([[1, 0.1, 0], [0, 1, 0], [0, 0, 1]], "upper"), ([[1, 0, 0], [0, 1, -1e-300], [0, 0, 1]], "upper"),
    ([[0, 0, 0], [0, 1, 0], [0, 0, 1]], "diagonal"), ([[1, 0, 0], [0, -1, 0], [0, 0, 1]], "diagonal"),
    ([[1, 0, 0], [0, 1, 0], [0, 0, np.inf]], "finite"), ([[1, 0, 0], [np.nan, 1, 0], [0, 0, 1]], "finite"),
    ([[1, 0, 0], [0, 1, 0], [np.inf, 0, 1]], "finite"),
])
def test_a_bad_host_cell_is_refused(bad, why):
    with pytest.raises(ValueError, match=why):
        Cell(bad)
    if isinstance(bad, list) and why != "numbers":  # the same in one frame of a per-frame cell
        with pytest.raises(ValueError, match=why):
            Cell(np.stack([R.SKEW, np.array(bad, dtype=float)]))


def test_a_cell_that_requires_a_gradient_is_refused_and_a_wrong_frame_count_too():
    with pytest.raises(ValueError, match="gradient"):
        Cell(torch.tensor(R.SKEW, requires_grad=True))
    x = lattice_sites(4, 5, 1)
    with pytest.raises(ValueError, match="frames"):
        pair_distances(x, triangle(5), box=Cell(R.frame_cells(3)))
    with pytest.raises(ValueError, match="frames"):
        make_whole(x, Cell(R.frame_cells(5)), np.array([[0, 1]]))


def test_raw_arrays_keep_their_meaning():
    """A raw (3, 3) array is one orthorhombic box per frame for three frames and nothing else; (3, 3, 3), (n, 9) and
    (9,) are refused as before."""
    L = np.array([[4.1, 5.3, 6.7], [4.2, 5.2, 6.6], [4.0, 5.4, 6.8]])
    assert tuple(_as_box(L, 3).shape) == (3, 3)
    x = lattice_sites(3, 5, 2)
    got = pair_distances(x, triangle(5), box=L)
    per_frame = torch.stack([pair_distances(x[t:t + 1], triangle(5), box=L[t])[0] for t in range(3)])
    assert torch.equal(got, per_frame)
    lower = np.tril(L)  # (even a lower-triangular one: the rows are lengths, zeros are refused as lengths)
    with pytest.raises(ValueError, match="positive"):
        pair_distances(x, triangle(5), box=lower)
    for bad, T in ((L, 4), (np.ones((3, 3, 3)), 3), (np.ones((3, 9)), 3), (np.ones(9), 3), (np.ones((4, 3, 3)), 4)):
        with pytest.raises(ValueError, match="shape"):
            _as_box(bad, T)
        with pytest.raises(ValueError, match="shape"):
            pair_distances(lattice_sites(T, 5, 2), triangle(5), box=bad)


def test_from_lengths_angles():
    d = R.D
    rd = Cell.from_lengths_angles([d, d, d], [60, 60, 90])
    assert np.allclose(rd.vectors.numpy(), R.rhombic_dodecahedron(d), rtol=0, atol=4 * np.finfo(float).eps * d)
    assert rd.vectors[1, 0] == 0 and rd.vectors[0, 1] == 0  # (90 degrees: an exact zero)
    theta = np.degrees(np.arccos(1 / 3))
    to = Cell.from_lengths_angles([d, d, d], [theta, 180 - theta, theta])
    assert np.allclose(to.vectors.numpy(), R.truncated_octahedron(d), rtol=0, atol=8 * np.finfo(float).eps * d)
    diag = Cell.from_lengths_angles(R.DIAG_LENGTHS, [90, 90, 90])
    assert np.array_equal(diag.vectors.numpy(), R.DIAG)
    per = Cell.from_lengths_angles(np.stack([R.DIAG_LENGTHS, [d, d, d]]), np.array([[90, 90, 90], [60, 60, 90.0]]))
    assert per.is_per_frame and np.array_equal(per.vectors[0].numpy(), R.DIAG)
    assert np.array_equal(per.vectors[1].numpy(), rd.vectors.numpy())
    for lengths, angles in (([1, 2], [90, 90]), ([1, 2, 3], [[90, 90, 90]]), ([1, 2, 3], [90, 90, 200]),
                            ([1, -2, 3], [90, 90, 90]), (["a", 2, 3], [90, 90, 90])):
        with pytest.raises(ValueError):
            Cell.from_lengths_angles(lengths, angles)


# ------------------------------------------------------------------ 2. the reference against brute force
@pytest.mark.parametrize("kind", [k for k in KINDS if k != "frames"] + ["frames0", "frames3"])
def test_the_brick_image_is_the_minimum_image_below_the_safe_radius_and_never_shorter_beyond(kind):
    H = R.frame_cells(4)[int(kind[-1])] if kind.startswith("frames") else R.cell_of(kind, 1)
    rng = np.random.default_rng(len(kind))
    M = 6000
    d = rng.uniform(-3, 3, (M, 3)) @ H  # +-3 cell lengths along every lattice vector (uniform over 216 cells)
    image, counts, _ = R.brick(d[None], H)
    image, counts = image[0], counts[0]
    best, length = R.brute_min(d, H)
    got = np.linalg.norm(image, axis=-1)
    r_safe = R.safe_radius(H)
    inside = length < r_safe
    assert inside.mean() >= 0.25 and (~inside).mean() >= 0.25, f"{inside.mean():.2f} of the samples below r_safe"
    # a lattice translate, inside the brick
    assert np.allclose(d - counts @ H, image, rtol=0, atol=1e-12)
    assert (np.abs(image) <= np.diagonal(H) / 2 + 1e-12).all()
    # below r_safe: THE minimum image (the same vector, not only the same length)
    assert np.abs(image[inside] - best[inside]).max() < 1e-12
    # beyond: a periodic image, never shorter than the minimum
    assert (got[~inside] >= length[~inside] - 1e-12).all()
    if kind not in ("diag",):
        assert (got[~inside] > length[~inside] + 1e-6).any(), "the brick image is the minimum everywhere: a weak sample"
    assert np.abs(counts).max() >= 2 and np.abs(counts).max() <= 4  # (within the reach of the brute force)


def test_a_diagonal_cell_is_the_orthorhombic_wrap_in_the_reference_too():
    import pbc_ref

    d = np.random.default_rng(5).uniform(-15, 15, (3, 200, 3))
    assert np.array_equal(R.wrap(d, R.DIAG), pbc_ref.wrap(d, R.DIAG_LENGTHS))


# ------------------------------------------------------------------ 3. host bodies of the distances
def sites_for(kind, T, n, m, pairs, seed):
    H = R.cell_of(kind, T, seed)
    make = lambda k: (lattice_sites(T, n, seed + 100 * k), lattice_sites(T, m, seed + 100 * k + 1) + 0.4)  # noqa: E731
    (x, c), tie = R.tie_free_sites(make, lambda a, b: list_disp(a, b, pairs), H, torch.float64)
    return H, x, c, tie


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("as_tensor", [False, True], ids=["numpy", "cpu_tensor"])
def test_pair_distances_and_distances_in_box_match_the_reference(kind, as_tensor):
    T, n, m = 4, 9, 6
    pairs = random_list(40, m, n, 3, self_form=False)
    H, x, c, tie = sites_for(kind, T, n, m, pairs, 11)
    assert tie > 1e-11
    conv = torch.from_numpy if as_tensor else (lambda a: a)
    u = R.wrap(list_disp(x, c, pairs), H)
    assert (np.abs(R.brick(list_disp(x, c, pairs), H)[1]) >= 1).any()
    for square in (False, True):
        ref = (u * u).sum(-1) if square else np.linalg.norm(u, axis=-1)
        got = pair_distances(conv(x), pairs, cross_xyz=conv(c), square=square, box=Cell(H))
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-12, atol=1e-12)
    full = x[:, None, :, :] - c[:, :, None, :]
    if R.tie_distance(full, H) > 1e-11:
        mat = distances_in_box(conv(x), Cell(H), cross_xyz=conv(c))
        np.testing.assert_allclose(mat.numpy(), np.linalg.norm(R.wrap(full, H), axis=-1), rtol=1e-12, atol=1e-12)
        disp = distances_in_box(conv(x), Cell(H), cross_xyz=conv(c), return_displacements=True)
        np.testing.assert_allclose(disp.numpy(), R.wrap(full, H), rtol=0, atol=1e-12)
        mins = min_distances(conv(x), conv(c), box=Cell(H))
        np.testing.assert_allclose(mins.numpy(), np.linalg.norm(R.wrap(full, H), axis=-1).min(0), rtol=1e-12, atol=1e-12)
    # float32 inputs stay float32
    assert pair_distances(torch.from_numpy(x).float(), pairs, cross_xyz=torch.from_numpy(c).float(), box=Cell(H)).dtype == torch.float32


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_cell", "cell_per_frame"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_a_diagonal_cell_gives_the_bits_of_the_box_form_on_the_host(per_frame, dtype):
    import pbc_ref

    T, n, m = 5, 9, 6
    L = pbc_ref.frame_boxes(T, 3) if per_frame else R.DIAG_LENGTHS
    H = np.stack([np.diag(l) for l in L]) if per_frame else np.diag(L)
    x, c = torch.from_numpy(lattice_sites(T, n, 21)).to(dtype), torch.from_numpy(lattice_sites(T, m, 22) + 0.4).to(dtype)
    pairs = random_list(40, m, n, 3, self_form=False)
    for square in (False, True):
        assert torch.equal(pair_distances(x, pairs, cross_xyz=c, square=square, box=Cell(H)),
                           pair_distances(x, pairs, cross_xyz=c, square=square, box=L))
        assert torch.equal(distances_in_box(x, Cell(H), square=square), distances_in_box(x, L, square=square))
        assert torch.equal(min_distances(x, c, square=square, box=Cell(H)), min_distances(x, c, square=square, box=L))
    assert torch.equal(distances_in_box(x, Cell(H), return_displacements=True), distances_in_box(x, L, return_displacements=True))
    assert torch.equal(distances_in_box(x, Cell(H), return_matrix=False), distances_in_box(x, L, return_matrix=False))
    cut = 1.9
    assert np.array_equal(PairList.from_cutoff(x, cut, box=Cell(H)).pairs, PairList.from_cutoff(x, cut, box=L).pairs)
    # make_whole: coordinates and images
    tree = MoleculeTree(np.array([-1, 0, 1, 2, 3, -1, 5, 8, 5]))
    for arr in (x, x.numpy()):
        u, k = make_whole(arr, Cell(H), tree, return_images=True)
        u0, k0 = make_whole(arr, L, tree, return_images=True)
        same = torch.equal if isinstance(arr, torch.Tensor) else np.array_equal
        assert same(u, u0) and same(k, k0) and bool((k != 0).any())
    # the guess, host branch (cross_xyz)
    assert guess_pairwise_constraints(x.numpy(), cross_xyz=c.numpy(), box=Cell(H), threshold=0.35) == \
        guess_pairwise_constraints(x.numpy(), cross_xyz=c.numpy(), box=L, threshold=0.35)


@pytest.mark.parametrize("kind", KINDS)
def test_from_cutoff_on_the_host_is_the_brute_force_list_and_refuses_a_cutoff_beyond_the_safe_radius(kind):
    T, n = 3, 20
    H = R.cell_of(kind, T, 4)
    x = R.wrap_positions(lattice_sites(T, n, 31), H)
    i, j = np.triu_indices(n, 1)
    Hs = np.broadcast_to(H, (T, 3, 3))
    mins = np.min([R.brute_min(x[t][j] - x[t][i], Hs[t])[1] for t in range(T)], axis=0)
    r_safe = R.safe_radius(H)
    cut = 0.97 * r_safe
    assert np.min(np.abs(mins - cut)) > 1e-6 and 3 < (mins <= cut).sum() < len(mins)
    pl = PairList.from_cutoff(x, cut, box=Cell(H))
    assert [tuple(p) for p in pl.pairs] == [(a, b) for a, b, d in zip(i, j, mins) if d <= cut]
    assert PairList.from_cutoff(x, r_safe, box=Cell(H)).n_pairs >= pl.n_pairs  # (the radius itself is allowed)
    with pytest.raises(ValueError, match="safe radius"):
        PairList.from_cutoff(x, r_safe * 1.0001, box=Cell(H))


# ------------------------------------------------------------------ 4. make_whole on the host
TREES, molecule = R.TREES, R.molecule


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tree", sorted(TREES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_make_whole_on_the_host_matches_the_tree_walk(kind, tree, dtype):
    T, N = 4, 23
    H = torch.from_numpy(R.cell_of(kind, T, 6)).to(dtype).double().numpy()  # (as stored)
    w, par = molecule(tree, T, N, H, dtype, 41)
    u, k, tie, bound = R.whole_reference(w, H, par)
    assert tie > 2 * R.MARGIN[dtype] and np.abs(k).max() >= 1
    mt = MoleculeTree(par)
    assert mt.n_rounds >= (3 if tree != "forest" else 2)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    for arr in (w.astype(npdt), torch.from_numpy(w).to(dtype)):
        got, images = make_whole(arr, Cell(H), mt, return_images=True)
        g, im = (got.numpy(), images.numpy()) if isinstance(got, torch.Tensor) else (got, images)
        assert g.dtype == npdt and im.dtype == np.int32
        assert np.array_equal(im, k)
        R.assert_whole(g, u, bound, dtype, f"host {kind} {tree}")
        # every bonded pair's plain displacement is now its brick image
        has = par >= 0
        plain = g.astype(np.float64)[:, has] - g.astype(np.float64)[:, par[has]]
        assert np.abs(plain - R.wrap(plain, H)).max() == 0
    keep = w.astype(npdt).copy()
    out = make_whole(keep, Cell(H), mt, inplace=True)
    assert out is keep and np.array_equal(keep, g)
    xt = torch.from_numpy(w).to(dtype).requires_grad_(True)
    whole = make_whole(xt, Cell(H), mt)
    (grad,) = torch.autograd.grad(whole.sum(), xt)
    assert torch.equal(grad, torch.ones_like(xt))  # the identity backward


def test_make_whole_on_the_host_with_a_cell_from_the_gpu_conventions():
    """A bad frame (a cell that could only have come unchecked) and a non-finite coordinate in the NumPy body."""
    from aggforce_amd.pbc import _host_whole_cell

    T, N = 3, 6
    H = np.tile(R.SKEW, (T, 1, 1))
    w, par = molecule("chain", T, N, R.SKEW, torch.float64, 43)
    mt = MoleculeTree(par)
    good_u, good_k = _host_whole_cell(w, H.reshape(T, 9), mt)
    bad = H.copy()
    bad[1, 2, 1] = np.inf
    u, k = _host_whole_cell(w, bad.reshape(T, 9), mt)
    assert np.isnan(u[1]).all() and not k[1].any()
    assert np.array_equal(u[[0, 2]], good_u[[0, 2]]) and np.array_equal(k[[0, 2]], good_k[[0, 2]])
    w2 = w.copy()
    w2[0, 2, 1] = np.nan
    u, k = _host_whole_cell(w2, H.reshape(T, 9), mt)
    assert np.isnan(u[0, 2, 1]) and np.isfinite(np.delete(u[0].ravel(), 2 * 3 + 1)).all()
    assert np.array_equal(u[1:], good_u[1:])


# ------------------------------------------------------------------ 5. the guess, host branch
def test_the_host_guess_finds_a_rigid_pair_that_the_wrap_splits_across_a_skewed_face():
    T = 30
    H = R.rhombic_dodecahedron()
    rng = np.random.default_rng(51)
    centre = np.cumsum(0.4 * rng.standard_normal((T, 1, 3)), axis=0) + 0.3 * H[2]
    rigid = np.concatenate([centre, centre + np.array([0.5, 0.3, 0.7])], axis=1)
    loose = rng.uniform(0, 4, (T, 2, 3))
    whole = np.concatenate([rigid, loose], axis=1)
    x = R.wrap_positions(whole, H)
    k = R.brick(x[:, 1] - x[:, 0], H)[1]
    assert (k[:, 2] != 0).any() and (k[:, 2] == 0).any(), "the pair is never split across the c face"
    assert (0, 1) in guess_pairwise_constraints(x, cross_xyz=x, box=Cell(H))
    assert (0, 1) not in guess_pairwise_constraints(x, cross_xyz=x)
    assert (0, 1) not in guess_pairwise_constraints(x, cross_xyz=x, box=np.diagonal(H))


# ------------------------------------------------------------------ 6. gradcheck through the wrap
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
def test_gradcheck_through_the_wrap_on_the_cpu(kind, square):
    T, n = 2, 5
    pairs = triangle(n)
    H = R.cell_of(kind, T, 8)
    (xn, _), tie = R.tie_free_sites(lambda k: (lattice_sites(T, n, 61 + k) * 1.7, lattice_sites(T, n, 0)),
                                    lambda a, b: list_disp(a, a, pairs), H, torch.float64, margin=1e-3)
    assert tie > 1e-3  # (gradcheck steps by 1e-6)
    assert (R.brick(list_disp(xn, xn, pairs), H)[1] != 0).any()
    x = torch.tensor(xn, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a: pair_distances(a, pairs, square=square, box=Cell(H)), (x,), **GC)
    assert torch.autograd.gradcheck(lambda a: distances_in_box(a, Cell(H), square=True), (x,), **GC)


# ------------------------------------------------------------------ 7. refusals
def test_functions_without_a_triclinic_form_refuse_a_cell_by_name():
    from aggforce_amd import LinearMap
    from aggforce_amd.qp import gb_feat
    from aggforce_amd.qp.jaxfeat import gb_subfeat, gb_subfeat_jac

    cell = Cell(R.SKEW)
    x = lattice_sites(3, 6, 71)
    pts, cg = torch.from_numpy(x), torch.from_numpy(x[:, :1])
    with pytest.raises(ValueError, match="gb_subfeat.*triclinic"):
        gb_subfeat(pts, cg, np.zeros(6, dtype=int), 1, None, outer=6.0, box=cell)
    with pytest.raises(ValueError, match="gb_subfeat_jac.*triclinic"):
        gb_subfeat_jac(pts, cg, np.zeros(6, dtype=int), 1, outer=6.0, box=cell)
    cmap = LinearMap([[0, 1, 2], [3, 4, 5]], n_fg_sites=6)
    with pytest.raises(ValueError, match="gb_feat.*triclinic"):
        gb_feat(x, cmap, set(), outer=6.0, box=cell)
    comm = object()  # (refused before anything asks what it is)
    with pytest.raises(ValueError, match="guess_pairwise_constraints.*triclinic"):
        guess_pairwise_constraints(x, box=cell, comm=comm)
    with pytest.raises(ValueError, match="project_forces.*triclinic"):
        project_forces(x, x, cmap, constrained_inds=set(), box=cell, comm=comm)
    with pytest.raises(ValueError, match="project_forces_grid_cv.*triclinic"):
        project_forces_grid_cv({"l2_regularization": [1.0]}, x, x, coord_map=cmap, constrained_inds=set(), box=cell, comm=comm)
    with pytest.raises(ValueError, match="frames"):  # a per-frame cell of another length, with explicit constraints
        project_forces(x, x, cmap, constrained_inds=set(), box=Cell(R.frame_cells(4)))
