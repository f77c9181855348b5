"""The nearest image of a triclinic cell on the host (``Cell(vectors, images="nearest")``): the ``Cell`` surface, the
guarantee of the reference (tests/nearest_ref.py) against a brute force, its agreement with the brick and the box
references where they must agree, the conditions that the inputs of tests/test_gpu_nearest.py have to meet (checked on
the reference alone), and the host bodies of the pair-distance functions against the reference, gradients included."""
import numpy as np
import pytest
import torch

import cell_ref as R
import nearest_ref as N
from featpbc_cases import min_image
from pairlist_ref import random_list, triangle
from aggforce_amd import Cell
from aggforce_amd import jaxmapval as mv
from aggforce_amd import pbc
from aggforce_amd._cell import refuse_cell
from aggforce_amd.jaxutil import PairList, distances_in_box, min_distances, pair_distances

F32, F64 = torch.float32, torch.float64
GC = dict(eps=1e-6, atol=1e-6, rtol=1e-5)  # (tests/test_gpu_pairlist.py's gradcheck settings)


# ------------------------------------------------------------------ 1. the Cell
def test_images_is_validated_kept_and_shown():
    H = N.dodecahedron_square()
    brick, near = Cell(H), Cell(H, images="nearest")
    assert brick.images == "brick" and near.images == "nearest" and Cell(H, "brick").images == "brick"
    for bad in ("Nearest", "", None, 27, "minimum"):
        with pytest.raises(ValueError, match="images"):
            Cell(H, images=bad)
    assert "images" not in repr(brick) and repr(brick) == f"Cell(vectors={torch.as_tensor(H).tolist()})"
    assert repr(near).endswith(", images='nearest')") and repr(near).startswith(repr(brick)[:-1])
    per_frame = Cell(N.frame_cells("octahedron", 5), images="nearest")
    assert "per frame" in repr(per_frame) and "nearest" in repr(per_frame)
    taken = per_frame.take([3, 1])
    assert taken.images == "nearest" and torch.equal(taken.vectors, per_frame.vectors[[3, 1]])
    assert near.take([0, 1]) is near and Cell(N.frame_cells("octahedron", 5)).take([2]).images == "brick"
    assert near.safe_radius == brick.safe_radius == R.safe_radius(H)
    assert torch.equal(near.rows(4), brick.rows(4))


def test_from_lengths_angles_takes_images():
    d = N.D
    for images in ("brick", "nearest"):
        cell = Cell.from_lengths_angles([d, d, d], [60.0, 60.0, 90.0], images=images)  # the square dodecahedron
        assert cell.images == images
        np.testing.assert_allclose(cell.vectors.numpy(), N.dodecahedron_square(), atol=1e-12)
    assert Cell.from_lengths_angles([d, d, d], [60.0, 60.0, 90.0]).images == "brick"
    with pytest.raises(ValueError, match="images"):
        Cell.from_lengths_angles([d, d, d], [60.0, 60.0, 90.0], images="both")


@pytest.mark.parametrize("kind", sorted(N.STANDARD))
def test_image_radius_of_the_standard_cells_is_half_the_image_distance(kind):
    H = N.STANDARD[kind]()
    assert N.is_reduced(H)
    brick, near = Cell(H), Cell(H, images="nearest")
    assert brick.image_radius == brick.safe_radius
    assert isinstance(near.image_radius, float) and abs(near.image_radius - 0.5 * N.D) < 1e-12
    assert abs(near.image_radius - N.image_radius(H)) < 1e-12
    table = {"dodecahedron": 0.354, "dodecahedron_hex": 0.408, "octahedron": 0.408}  # safe_radius / d
    assert abs(near.safe_radius / N.D - table[kind]) < 5e-4
    frames = N.frame_cells(kind, 6)
    assert abs(Cell(frames, images="nearest").image_radius - N.image_radius(frames)) < 1e-12  # the smallest frame's
    assert Cell(np.zeros((0, 3, 3)), images="nearest").image_radius == float("inf")


def test_an_unreduced_host_cell_is_refused_and_equality_is_allowed():
    unreduced = np.array([[4.1, 0, 0], [-2.3, 4.7, 0], [1.7, -2.1, 5.0]])
    assert not N.is_reduced(unreduced) and N.is_reduced(R.SKEW)
    with pytest.raises(ValueError, match=r"\|bx\| <= ax/2.*\|cx\| <= ax/2.*\|cy\| <= by/2"):
        Cell(unreduced, images="nearest")
    Cell(unreduced)  # (the brick form has no such condition)
    Cell(R.SKEW, images="nearest")
    H = N.dodecahedron_square()
    assert H[2, 0] == H[0, 0] / 2 and H[2, 1] == H[1, 1] / 2  # equality in cx and cy
    Cell(H, images="nearest")
    for r, c in ((1, 0), (2, 0), (2, 1)):
        over = np.diag([4.0, 4.0, 4.0])
        over[r, c] = 2.0
        Cell(over, images="nearest")
        over[r, c] = -2.00001
        with pytest.raises(ValueError, match="reduced"):
            Cell(over, images="nearest")
    frames = N.frame_cells("octahedron", 4)
    frames[2, 1, 0] = 0.6 * frames[2, 0, 0]
    with pytest.raises(ValueError, match="reduced"):
        Cell(frames, images="nearest")
    with pytest.raises(ValueError, match="lower-triangular"):  # the other checks come first and stay
        Cell(np.array([[4.0, 1.0, 0], [0, 4.0, 0], [0, 0, 4.0]]), images="nearest")


# ------------------------------------------------------------------ 2. the guarantee of the reference
def check_guarantee(H, M, rng):
    d = rng.uniform(-3, 3, (M, 3)) @ H
    image, pick, _ = N.nearest(d[None], H)
    true, length = N.brute_from_brick(d, H, reach=3)
    below = length < N.image_radius(H)
    assert below.sum() > M // 20
    wrong = np.abs(image[0] - true).max(-1)[below] > 1e-9 * np.abs(H).max()
    assert not wrong.any(), f"{int(wrong.sum())} of {int(below.sum())} displacements below the image radius: {H.tolist()}"
    # beyond it: a periodic image, never longer than the brick image
    brick = R.wrap(d[None], H)[0]
    assert (np.linalg.norm(image[0], axis=-1) <= np.linalg.norm(brick, axis=-1)).all()
    frac = np.linalg.solve(H.T, (image[0] - d).T).T
    assert np.abs(frac - np.rint(frac)).max() < 1e-9
    return float((pick[0] != 0)[below].mean())


@pytest.mark.parametrize("kind", sorted(N.STANDARD))
def test_the_reference_is_the_true_minimum_image_below_the_image_radius_in_the_standard_cells(kind):
    differs = check_guarantee(N.STANDARD[kind](), 20000, np.random.default_rng(5))
    table = {"dodecahedron": 0.117, "dodecahedron_hex": 0.073, "octahedron": 0.051}  # where the brick image is not it
    print(f"{kind}: the brick image is not the minimum image for {differs:.3f} of the displacements below d / 2")
    assert abs(differs - table[kind]) < 0.01


def test_the_reference_is_the_true_minimum_image_below_the_image_radius_in_random_reduced_cells():
    rng = np.random.default_rng(6)
    for _ in range(40):
        H = N.random_reduced_cell(rng, ratio=4.0)
        assert N.is_reduced(H)
        check_guarantee(H, 3000, rng)


@pytest.mark.parametrize("kind", sorted(N.STANDARD) + ["dyadic"])
def test_pruned_and_unpruned_searches_agree_and_within_the_safe_radius_the_brick_image_stays(kind):
    H = N.DYADIC_NEAR if kind == "dyadic" else N.STANDARD[kind]()
    d = np.random.default_rng(7).uniform(-3, 3, (1, 30000, 3)) @ H
    if kind == "dyadic":
        d = np.rint(d * 16) / 16  # exact ties among them
    full, pruned = N.nearest(d, H), N.nearest(d, H, prune=True)
    assert np.array_equal(full[0], pruned[0]) and np.array_equal(full[1], pruned[1])
    brick = R.wrap(d, H)
    inside = np.linalg.norm(brick, axis=-1) <= R.safe_radius(H)
    assert inside.sum() > 1000 and np.array_equal(full[0][inside], brick[inside]) and not full[1][inside].any()
    assert (full[1] != 0).mean() > 0.05


def test_with_a_diagonal_cell_the_reference_is_the_orthorhombic_reference_exactly():
    d = np.random.default_rng(8).uniform(-14, 14, (3, 5000, 3))
    image, pick, _ = N.nearest(d, R.DIAG)
    assert np.array_equal(image, min_image(d, np.broadcast_to(R.DIAG_LENGTHS, d.shape), np.float64)) and not pick.any()
    assert N.image_radius(R.DIAG) == R.safe_radius(R.DIAG)


# ------------------------------------------------------------------ 3. the inputs of the GPU tests
LISTS = [("triangle19", triangle(19), None, 19), ("triangle70", triangle(70), None, 70),
         ("cross", random_list(300, 6, 11, 300, self_form=False), 6, 11)]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["one_cell", "cell_per_frame"])
@pytest.mark.parametrize("kind", N.GPU_KINDS)
def test_the_gpu_constructions_meet_their_conditions(kind, per_frame, dtype):
    H = N.gpu_cell(kind, per_frame, dtype)
    assert N.is_reduced(H) and (H.ndim == 3) == per_frame
    Cell(H, images="nearest")
    cases = [N.list_case(kind, per_frame, pairs, m, n, dtype)[3:] for _, pairs, m, n in LISTS]
    cases.append(N.matrix_case(kind, per_frame, 11, 70, dtype)[3:])
    for raw, tie in cases:
        differs, on_tie = N.input_conditions(raw, H)
        assert differs >= 0.05 and on_tie <= 0.02 and on_tie == tie.mean()
        assert R.tie_distance(raw, H) > 2 * R.MARGIN[dtype]
        # a fallback to the brick form is far outside every tolerance on these elements
        gap = np.abs(np.linalg.norm(N.wrap(raw, H), axis=-1) - np.linalg.norm(R.wrap(raw, H), axis=-1))
        assert (gap > 1e-3).mean() >= 0.05
        assert np.abs(R.brick(raw, H)[1]).max() >= 2  # raw displacements several cells long
    raw, tie = cases[-1]
    assert tie.any(axis=0).mean() <= 0.02  # pairs left out of the minimum over frames
    H, X, F, outer = N.mapval_case(kind, per_frame, dtype)
    off = ~np.eye(N.MV_N, dtype=bool)
    raw = (X[:, :, None, :] - X[:, None, :, :])[:, off]
    differs, on_tie = N.input_conditions(raw, H)
    assert differs >= 0.05 and on_tie == 0.0
    assert R.safe_radius(H) < outer < N.image_radius(H)
    x = (N.wrap(raw, H) ** 2).sum(-1)
    picked = N.nearest(raw, H)[1] != 0
    assert (picked & (x < outer**2)).sum() >= 10  # pairs the field reaches whose image the brick form gets wrong


@pytest.mark.parametrize("n,cross", [(19, None), (70, None), (11, 6)])
def test_the_dyadic_construction_is_exact_in_float32_and_free_of_ties(n, cross):
    x0, x1, c0, c1, H = N.dyadic_case(N.GPU_T, n, 3, cross)
    assert N.is_reduced(H) and np.array_equal(np.rint(H), H)
    for a in (x0, x1, c0, c1):
        assert np.array_equal(np.rint(a * 16), a * 16) and np.array_equal(a.astype(np.float32).astype(np.float64), a)
    d0, d1 = x0[:, None] - c0[:, :, None], x1[:, None] - c1[:, :, None]
    cand, q = N.candidates(R.wrap(d1, H), H)
    assert np.array_equal(q.astype(np.float32).astype(np.float64), q) and q.max() * 256 < 2**24  # exact squared lengths
    image, pick, gap = N.nearest(d1, H)
    assert np.array_equal(image, d0) and gap.min() > 0.1  # the unshifted displacement, and no tie
    assert np.linalg.norm(d0, axis=-1).max() < N.image_radius(H)
    assert (pick != 0).mean() >= 0.05 and np.abs(x1 - x0).max() >= 16


# ------------------------------------------------------------------ 4. the host bodies
def host_case(kind, per_frame, n=9, T=4, seed=0):
    H = N.frame_cells(kind, T, seed) if per_frame else N.STANDARD[kind]()
    x, c = N.spread_sites(T, n, H, 40 + seed), N.spread_sites(T, 5, H, 41 + seed)
    return H, x, c


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_cell", "cell_per_frame"])
@pytest.mark.parametrize("kind", N.GPU_KINDS)
def test_host_pair_distances_matrices_and_minima_match_the_reference(kind, per_frame):
    H, x, c = host_case(kind, per_frame)
    cell = Cell(H, images="nearest")
    pairs = random_list(40, 5, 9, 11, self_form=False)
    raw = x[:, pairs[:, 1]] - c[:, pairs[:, 0]]
    ref = np.linalg.norm(N.wrap(raw, H), axis=-1)
    assert (N.nearest(raw, H)[1] != 0).any() and N.nearest(raw, H)[2].min() > 1e-9
    for conv in (torch.from_numpy, lambda a: a):  # CPU tensors and NumPy arrays
        got = pair_distances(conv(x), pairs, cross_xyz=conv(c), box=cell)
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-13, atol=1e-13)
        sq = pair_distances(conv(x), pairs, cross_xyz=conv(c), square=True, box=cell)
        np.testing.assert_allclose(sq.numpy(), ref * ref, rtol=1e-13, atol=1e-13)
    full = N.wrap(x[:, None, :, :] - c[:, :, None, :], H)
    mat = distances_in_box(torch.from_numpy(x), cell, cross_xyz=torch.from_numpy(c))
    np.testing.assert_allclose(mat.numpy(), np.linalg.norm(full, axis=-1), rtol=1e-13, atol=1e-13)
    disp = distances_in_box(torch.from_numpy(x), cell, cross_xyz=torch.from_numpy(c), return_displacements=True)
    np.testing.assert_allclose(disp.numpy(), full, rtol=1e-13, atol=1e-13)
    own = N.wrap(x[:, None, :, :] - x[:, :, None, :], H)
    i, j = np.triu_indices(x.shape[1], 1)
    tri = distances_in_box(torch.from_numpy(x), cell, return_matrix=False)
    np.testing.assert_allclose(tri.numpy(), np.linalg.norm(own, axis=-1)[:, i, j], rtol=1e-13, atol=1e-13)
    mins = min_distances(torch.from_numpy(x), torch.from_numpy(c), box=cell)
    np.testing.assert_allclose(mins.numpy(), np.linalg.norm(full, axis=-1).min(0), rtol=1e-13, atol=1e-13)
    # and a brick cell behaves as before
    brick = pair_distances(torch.from_numpy(x), pairs, cross_xyz=torch.from_numpy(c), box=Cell(H))
    np.testing.assert_allclose(brick.numpy(), np.linalg.norm(R.wrap(raw, H), axis=-1), rtol=1e-13, atol=1e-13)
    assert (brick.numpy() > ref + 1e-3).any() and (brick.numpy() >= ref - 1e-12).all()


@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
@pytest.mark.parametrize("kind", N.GPU_KINDS)
def test_host_gradcheck_and_the_gradient_is_that_of_the_chosen_image(kind, square):
    H = N.STANDARD[kind]()
    pairs = np.array([[0, 1], [3, 2], [0, 4], [3, 2], [2, 0], [3, 4], [1, 3]])  # (no i == j: plain torch has no gradient at 0)
    for seed in range(2000):  # sites well away from every tie (gradcheck steps by 1e-6)
        x = N.spread_sites(2, 5, H, 70 + seed)
        raw = x[:, pairs[:, 1]] - x[:, pairs[:, 0]]
        if R.tie_distance(raw, H) > 1e-3 and N.nearest(raw, H)[2].min() > 1e-3 and (N.nearest(raw, H)[1] != 0).any():
            break
    else:
        raise AssertionError("no input away from the ties")
    cell = Cell(H, images="nearest")
    xt = torch.tensor(x, requires_grad=True)
    fn = lambda a: pair_distances(a, pairs, square=square, box=cell)  # noqa: E731
    assert torch.autograd.gradcheck(fn, (xt,), **GC) and torch.autograd.gradgradcheck(fn, (xt,), **GC)
    w = torch.randn(2, len(pairs), dtype=F64)
    (g,) = torch.autograd.grad((fn(xt) * w).sum(), xt)
    z = torch.tensor(x, requires_grad=True)
    u = N.torch_wrap(z[:, pairs[:, 1]] - z[:, pairs[:, 0]], H)
    d = (u * u).sum(-1) if square else torch.linalg.vector_norm(u, dim=-1)
    (g_ref,) = torch.autograd.grad((d * w).sum(), z)
    torch.testing.assert_close(g, g_ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", N.GPU_KINDS)
def test_from_cutoff_takes_the_image_radius_and_gives_the_reference_list(kind):
    H = N.STANDARD[kind]()
    T, n = 5, 30
    x = R.wrap_positions(N.spread_sites(T, n, H, 90), H)
    near, brick = Cell(H, images="nearest"), Cell(H)
    r = near.image_radius
    assert r > brick.safe_radius * 1.2
    i, j = np.triu_indices(n, 1)
    mins = np.min([R.brute_min(x[t][j] - x[t][i], H)[1] for t in range(T)], axis=0)  # the TRUE minimum image
    want = [(a, b) for a, b, d in zip(i, j, mins) if d <= r]
    assert np.min(np.abs(mins - r)) > 1e-9 and len(want) > len([d for d in mins if d <= brick.safe_radius]) + 10
    pl = PairList.from_cutoff(torch.from_numpy(x), r, box=near)
    assert [tuple(p) for p in pl.pairs] == want
    with pytest.raises(ValueError, match="image radius"):
        PairList.from_cutoff(torch.from_numpy(x), 1.0001 * r, box=near)
    # the refusals of a brick cell are unchanged
    with pytest.raises(ValueError, match="safe radius"):
        PairList.from_cutoff(torch.from_numpy(x), r, box=brick)
    with pytest.raises(ValueError, match="safe radius"):
        PairList.from_cutoff(torch.from_numpy(x), 1.0001 * brick.safe_radius, box=brick)
    PairList.from_cutoff(torch.from_numpy(x), brick.safe_radius, box=brick)


def test_map_validation_takes_outer_up_to_the_image_radius_and_refusals_stand():
    H = N.dodecahedron_square()
    near, brick = Cell(H, images="nearest"), Cell(H)
    x = np.random.default_rng(0).random((3, 6, 3)) @ H
    f = np.zeros_like(x)
    between = 0.5 * (near.image_radius + brick.safe_radius)
    for fn in (mv.random_force_proj, mv.random_residual_shift):
        with pytest.raises(ValueError, match="image radius"):  # (before any device work)
            fn(x, f, 3, np.random.default_rng(0), inner=0.5, outer=1.0001 * near.image_radius, width=0.5, box=near)
        with pytest.raises(ValueError, match="half the smallest box length"):
            fn(x, f, 3, np.random.default_rng(0), inner=0.5, outer=between, width=0.5, box=brick)
    with pytest.raises(ValueError, match="image radius"):
        pbc.rsqpg_forces(x, 0.5, 1.0001 * near.image_radius, 0.5, box=near)
    with pytest.raises(ValueError, match="image radius"):
        pbc.rsqpg_forces(x, 0.25, (1.0001 * near.image_radius) ** 2, 0.25, sq_args=False, box=near)
    with pytest.raises(ValueError, match="half the smallest box length"):
        pbc.rsqpg_forces(x, 0.5, between, 0.5, box=brick)


def test_the_brick_form_functions_accept_a_nearest_cell_and_the_refusals_of_any_cell_stand():
    x, H = N.spread_sites(12, 6, N.dodecahedron_square(), 3), N.dodecahedron_square()
    x = R.wrap_positions(x, H)
    near, brick = Cell(H, images="nearest"), Cell(H)
    par = np.array([-1, 0, 1, -1, 3, 4])
    tree = pbc.MoleculeTree(par)
    a, ka = pbc.make_whole(x, near, tree, return_images=True)
    b, kb = pbc.make_whole(x, brick, tree, return_images=True)
    assert np.array_equal(a, b) and np.array_equal(ka, kb)
    with pytest.raises(ValueError, match="triclinic cells are not built"):
        refuse_cell(near, "gb_feat")
