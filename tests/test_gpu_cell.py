"""Triclinic cells on the GPU: the triclinic forms of K9c / K9d (pairlist_pbc_kernel<.., 2>, pairlist_pull_pbc_kernel<..,
2>), K9e (pairmin_kernel<.., true, 2>), K6 (pair_stats_pbc_kernel<.., 2>, pair_var_pbc_kernel<.., 2>) and K11
(whole_lds_kernel / whole_edge_kernel / whole_shift_kernel<.., 2>) -- every instantiation launched and checked by name
-- against the float64 / long double restatement of tests/cell_ref.py, with the helpers, bounds and settings of the box
tests of the same kernels (tests/test_gpu_pairlist.py ``close``, ``TOL``, ``GC``; tests/test_gpu_guess_box.py's 1e-10
bound; tests/test_gpu_whole.py's end-to-end bound), then a diagonal cell against the box form bit for bit, bad cells,
the caller's stream, and ``project_forces`` / ``project_forces_grid_cv`` on a wrapped dodecahedron system.

Inputs are free of ties (``cell_ref.tie_free_sites``: no quotient of the three stages within the margin of a
half-integer, asserted), so no element is masked.  Cells: a rhombic dodecahedron, a truncated octahedron, a generic
skewed cell with negative off-diagonals, a cell whose skew changes from frame to frame, a diagonal cell."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cell_ref as R  # noqa: E402
import stream_gate as SG  # noqa: E402
import test_gpu_pairlist as base  # noqa: E402  (close, TOL, GC, launched, reset, dev, host, force_matching)
from aggforce_amd import Cell, LinearMap, MoleculeTree, guess_pairwise_constraints, make_whole, project_forces  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd import _lib  # noqa: E402
from aggforce_amd.agg import project_forces_grid_cv  # noqa: E402
from aggforce_amd.jaxutil import PairList, distances_in_box, min_distances, pair_distances  # noqa: E402
from pairlist_ref import lattice_sites, list_disp, pull_reference, random_list, triangle  # noqa: E402
from pbc_ref import frame_boxes  # noqa: E402

DEV = base.DEV
F32, F64 = torch.float32, torch.float64
TOL, NAME, LANE_DEG = base.TOL, base.NAME, base.LANE_DEG
dev, host, close, reset = base.dev, base.host, base.close, base.reset


def launched():
    """Names of the kernels launched since the last reset, without return type and namespace."""
    torch.cuda.synchronize()
    return sorted(p.split("(")[0].replace("void ", "").replace("aggf::", "")
                  for p, c in _lib.coverage(names=True).values() if c > 0)

KINDS = R.KINDS
FRAMES = (3, 9)

CROSS = random_list(70, 6, 11, 300, self_form=False)
CROSS[7] = (2, 2)  # an i == j entry beside the repeat
# (name, pairs, m or None for the self form, n): n from 5 to 70; triangle70 has 69 entries per site (the wave form of K9d)
CASES = [("triangle5", triangle(5), None, 5), ("triangle70", triangle(70), None, 70),
         ("random65", random_list(65, 9, 9, 265), None, 9), ("cross", CROSS, 6, 11)]
CASE_IDS = [c[0] for c in CASES]


def stored(a, dtype):
    """``a`` as float64 after a round trip through ``dtype``: what the device holds."""
    return torch.as_tensor(np.asarray(a)).to(dtype).double().numpy()


def rows(H, T, dtype):
    """The (T, 9) device rows of a cell H ((3, 3) or (T, 3, 3)) in ``dtype``: what the kernel wrappers take."""
    return dev(np.ascontiguousarray(np.broadcast_to(H, (T, 3, 3))).reshape(T, 9), dtype).contiguous()


def operands(kind, T, pairs, m, n, dtype, seed=0):
    """Tie-free operands of a list call: (H as stored, x, c, v, y, w on the device, the tie distance)."""
    H = stored(R.cell_of(kind, T, seed), dtype)
    base_seed = 1000 * T + 10 * len(pairs) + n + seed

    def make(k):
        x = lattice_sites(T, n, base_seed + 7919 * k)
        return (x, x if m is None else lattice_sites(T, m, base_seed + 7919 * k + 1) + 0.4)

    (xn, cn), tie = R.tie_free_sites(make, lambda a, b: list_disp(a, b, pairs), H, dtype)
    assert tie > 2 * R.MARGIN[dtype]
    rng = np.random.default_rng(base_seed + 2)
    x = dev(xn, dtype)
    c = x if m is None else dev(cn, dtype)
    v = dev(rng.standard_normal((T, n, 3)), dtype)
    y = v if m is None else dev(rng.standard_normal((T, m, 3)), dtype)
    w = dev(rng.standard_normal((T, len(pairs))), dtype)
    return H, x, c, v, y, w


def pull_names(pl, ind, outd, dv):
    forms = {int(deg > LANE_DEG) for _, _, deg in pl.tables()}
    return sorted(f"pairlist_pull_pbc_kernel<{NAME[ind]}, {NAME[outd]}, {'true' if dv else 'false'}, {f}, 2>" for f in forms)


def test_the_cases_reach_both_forms_of_the_pull_kernel_and_images_beyond_the_first():
    degs = {name: [deg for _, _, deg in PairList(pairs, n, m).tables()] for name, pairs, m, n in CASES}
    assert max(degs["triangle5"]) <= LANE_DEG < min(degs["triangle70"]) and max(degs["cross"]) <= LANE_DEG
    raw = list_disp(lattice_sites(3, 70, 1), lattice_sites(3, 70, 1), triangle(70))
    for kind in KINDS:
        assert np.abs(R.brick(raw, R.cell_of(kind, 3))[1]).max() >= 2, kind


# ------------------------------------------------------------------ 1. K9c / K9d against the reference
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_k9c_triclinic_form_every_mode_matches_the_reference(case, dtype, kind):
    _, pairs, m, n = case
    tab = PairList(pairs, n, m).on(DEV)
    for T in FRAMES:
        H, x, c, v, y, _ = operands(kind, T, pairs, m, n, dtype)
        raw = list_disp(host(x), host(c), pairs)
        u, b = R.wrap(raw, H), R.comp_bound(raw, H)
        g = list_disp(host(v), host(y), pairs)
        sq, bsq = (u * u).sum(-1), (b * b).sum(-1)
        cell = rows(H, T, dtype)
        reset()
        d = K.pair_list_dist(x, c, tab, K.PAIR_DIST, box=cell)
        s = K.pair_list_dist(x, c, tab, K.PAIR_SQDIST, box=cell)
        o = K.pair_list_dist(x, c, tab, K.PAIR_DOT, v, y, box=cell)
        assert launched() == [f"pairlist_pbc_kernel<{NAME[dtype]}, {mode}, 2>" for mode in (0, 1, 2)]
        for got in (d, s, o):
            assert got.dtype == dtype and tuple(got.shape) == (T, len(pairs))
        close(d, np.sqrt(sq), np.sqrt(bsq), TOL[dtype], "K9c cell DIST")
        close(s, sq, bsq, TOL[dtype], "K9c cell SQDIST")
        close(o, (g * u).sum(-1), (np.abs(g) * b).sum(-1), TOL[dtype], "K9c cell DOT")
        # the public function, from a Cell on the host (one cell, or one per frame)
        pub = pair_distances(x, PairList(pairs, n, m), None if m is None else c, box=Cell(H))
        assert torch.equal(pub, d)
        same = pairs[:, 0] == pairs[:, 1]
        if m is None and same.any():
            assert (d[:, torch.tensor(same, device=DEV)] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32)], ids=["f32", "f64", "f64-f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_k9d_triclinic_form_both_sums_match_the_reference_and_repeat_bit_for_bit(case, ind, outd, kind):
    _, pairs, m, n = case
    pl = PairList(pairs, n, m)
    tab = pl.on(DEV)
    nrows = n if m is None else m
    tol = max(TOL[ind], TOL[outd])
    for T in FRAMES:
        H, x, c, _, _, w = operands(kind, T, pairs, m, n, ind)
        raw = list_disp(host(x), host(c), pairs)
        u, b = R.wrap(raw, H), R.comp_bound(raw, H)
        wn = host(w)
        cell = rows(H, T, ind)

        def bounds(weights):
            ab, bb, _, _ = pull_reference(np.abs(weights), b, pairs, nrows, n)
            return ab, -bb

        a_ref, b_ref, _, _ = pull_reference(wn, u, pairs, nrows, n)
        a_bnd, b_bnd = bounds(wn)
        reset()
        a, bsum = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=cell)
        assert launched() == pull_names(pl, ind, outd, False)
        assert a.dtype == outd and bsum.dtype == outd and tuple(a.shape) == (T, n, 3) and tuple(bsum.shape) == (T, nrows, 3)
        close(a, a_ref, a_bnd, tol, "K9d cell A")
        close(bsum, b_ref, b_bnd, tol, "K9d cell B")
        a2, b2 = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=cell)
        assert torch.equal(a, a2) and torch.equal(bsum, b2)
        a1, none = K.pair_list_pull(w, x, c, tab, want_b=False, out_dtype=outd, box=cell)
        assert none is None and torch.equal(a1, a)
        # the distance form: w / dv where dv > 0, else 0
        dv = K.pair_list_dist(x, c, tab, K.PAIR_DIST, box=cell)
        dvn = host(dv)
        wq = np.where(dvn > 0, wn / np.where(dvn > 0, dvn, 1.0), 0.0)
        a_ref, b_ref, _, _ = pull_reference(wq, u, pairs, nrows, n)
        a_bnd, b_bnd = bounds(wq)
        reset()
        a, bsum = K.pair_list_pull(w, x, c, tab, dv=dv, out_dtype=outd, box=cell)
        assert launched() == pull_names(pl, ind, outd, True)
        assert torch.isfinite(a).all() and torch.isfinite(bsum).all()
        close(a, a_ref, a_bnd, tol, "K9d cell A (Dv)")
        close(bsum, b_ref, b_bnd, tol, "K9d cell B (Dv)")


def tie_free_x(kind, T, n, pairs, seed, scale=1.0):
    H = R.cell_of(kind, T, seed)
    (xn, _), tie = R.tie_free_sites(lambda k: (scale * lattice_sites(T, n, seed + 31 * k), np.zeros(1)),
                                    lambda a, _b: list_disp(a, a, pairs), H, F64)
    return H, xn, tie


@pytest.mark.parametrize("form", ["self", "cross"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
def test_gradcheck_and_gradgradcheck_under_a_cell(form, kind, square):
    T = 2
    H = R.cell_of(kind, T, 75)
    if form == "self":
        pairs = np.array(base.SELF7)
        (xn, cn), tie = R.tie_free_sites(lambda k: (1.7 * lattice_sites(T, 5, 71 + k), lattice_sites(T, 4, 73 + k)),
                                         lambda a, _b: list_disp(a, a, pairs), H, F64, margin=1e-3)
        raw = list_disp(xn, xn, pairs)
    else:
        pairs = np.array([[0, 1], [3, 2], [0, 4], [3, 2], [1, 1], [2, 0], [3, 4]])
        (xn, cn), tie = R.tie_free_sites(lambda k: (1.7 * lattice_sites(T, 5, 71 + k), 1.7 * lattice_sites(T, 4, 73 + k) + 0.4),
                                         lambda a, b: list_disp(a, b, pairs), H, F64, margin=1e-3)
        raw = list_disp(xn, cn, pairs)
    assert tie > 1e-3  # (gradcheck steps by 1e-6: stay well away from a tie)
    assert (R.brick(raw, H)[1] != 0).any()
    x, c = dev(xn, grad=True), dev(cn, grad=True)
    cell = Cell(dev(H))  # (a cell on the GPU)
    if form == "self":
        pl = PairList(pairs, 5)
        fn, args = (lambda a: pair_distances(a, pl, square=square, box=cell)), (x,)
    else:
        fn, args = (lambda a, b: pair_distances(a, pairs, cross_xyz=b, square=square, box=cell)), (x, c)
    reset()
    assert torch.autograd.gradcheck(fn, args, **base.GC)
    assert torch.autograd.gradgradcheck(fn, args, **base.GC)
    names = launched()
    assert any(k.startswith("pairlist_pull_pbc_kernel<double") and k.endswith(", 2>") for k in names)
    assert "pairlist_pbc_kernel<double, 2, 2>" in names


def cpu_force_matching(xn, H):
    x = torch.tensor(xn, requires_grad=True)
    n = x.shape[1]
    i0, i1 = (torch.tensor(a) for a in np.triu_indices(n, 1))
    return base.force_matching(lambda z: torch.linalg.vector_norm(R.torch_wrap(z[:, i1] - z[:, i0], H), dim=-1), x)


@pytest.mark.parametrize("T,n", [(3, 5), (9, 70)])
@pytest.mark.parametrize("kind", ["dodecahedron", "frames"])
def test_first_gradients_and_the_force_matching_double_backward_under_a_cell(T, n, kind):
    H, xn, tie = tie_free_x(kind, T, n, triangle(n), 600 + n)
    assert tie > 2 * R.MARGIN[F64]
    reset()
    g, gg = base.force_matching(lambda z: distances_in_box(z, Cell(H), return_matrix=False), dev(xn, grad=True))
    names = launched()
    assert "pairlist_pbc_kernel<double, 2, 2>" in names
    assert any(k.startswith("pairlist_pull_pbc_kernel") and k.endswith(", 2>") for k in names)
    assert not any(k.startswith(("pairdist_kernel", "pairpull_kernel")) for k in names)
    assert torch.isfinite(gg).all(), "non-finite double backward"
    g_ref, gg_ref = cpu_force_matching(xn, H)
    torch.testing.assert_close(g.cpu(), g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg.cpu(), gg_ref, rtol=1e-10, atol=1e-9)


BAD = [("zero", (1, 1), 0.0), ("negative", (0, 0), -4.1), ("nan", (2, 2), float("nan")), ("inf", (1, 1), float("inf")),
       ("skew_nan", (2, 1), float("nan")), ("skew_inf", (1, 0), float("-inf"))]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("bad", BAD, ids=[b[0] for b in BAD])
def test_a_bad_cell_in_one_frame_makes_that_frame_nan_and_leaves_the_others_exact(dtype, bad):
    T = 3
    _, (r, cidx), value = bad
    for pairs, n in ((triangle(70), 70), (triangle(5), 9)):  # (the second leaves sites without entries)
        tab = PairList(pairs, n).on(DEV)
        H, x, c, v, y, w = operands("frames", T, pairs, None, n, dtype, seed=91)
        broken = np.array(np.broadcast_to(H, (T, 3, 3)))
        broken[1, r, cidx] = value
        good, bcell = rows(H, T, dtype), rows(broken, T, dtype)
        for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
            ref = K.pair_list_dist(x, c, tab, mode, v, y, box=good)
            got = K.pair_list_dist(x, c, tab, mode, v, y, box=bcell)
            assert torch.isnan(got[1]).all() and torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
        for kw in ({}, {"dv": K.pair_list_dist(x, c, tab, box=good)}):
            ra, rb = K.pair_list_pull(w, x, c, tab, box=good, **kw)
            ga, gb = K.pair_list_pull(w, x, c, tab, box=bcell, **kw)
            for got, ref in ((ga, ra), (gb, rb)):
                assert torch.isnan(got[1]).all() and torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
                assert torch.isfinite(ref).all()
        assert torch.isnan(K.pair_min(x, x, box=bcell)).all() and torch.isfinite(K.pair_min(x, x, box=good)).all()
    # an upper-triangular entry is not read
    upper = np.array(np.broadcast_to(H, (T, 3, 3)))
    upper[:, 0, 1], upper[:, 0, 2], upper[:, 1, 2] = float("nan"), 7.0, float("inf")
    assert torch.equal(K.pair_list_dist(x, c, tab, box=rows(upper, T, dtype)), K.pair_list_dist(x, c, tab, box=good))
    # a cell on the host is refused before any launch; a raw (T, 9) array is no box
    with pytest.raises(ValueError):
        Cell(broken)
    with pytest.raises(ValueError, match="shape"):
        pair_distances(x, pairs, box=good)


# ------------------------------------------------------------------ 2. K9e
def pairmin_names(dtype, split):
    return sorted([f"pairmin_kernel<{NAME[dtype]}, true, 2>"] + ([f"pairmin_reduce_kernel<{NAME[dtype]}>"] if split else []))


@pytest.mark.parametrize("T,m,n,split", [(5, 3, 7, False), (9, 11, 70, False), (200, 3, 7, True)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_min_distances_under_a_cell_match_the_reference_and_the_list_kernels(T, m, n, split, dtype, kind):
    pairs = PairList.all_pairs(n, m).pairs
    H, x, c, _, _, _ = operands(kind, T, pairs, m, n, dtype, seed=51)
    raw = host(x)[:, None, :, :] - host(c)[:, :, None, :]
    u, b = R.wrap(raw, H), R.comp_bound(raw, H)
    dist = np.linalg.norm(u, axis=-1)
    arg = dist.argmin(0)
    ref = np.take_along_axis(dist, arg[None], 0)[0]
    bnd = np.take_along_axis(np.linalg.norm(b, axis=-1), arg[None], 0)[0]
    if split:
        assert _lib.load().aggf_pair_min_workspace_bytes(T, m, n, K.dtype_code(dtype)) // (m * n * x.element_size()) == 4
    for square in (False, True):
        reset()
        got = min_distances(x, c, square=square, box=Cell(H))
        assert launched() == pairmin_names(dtype, split)
        assert tuple(got.shape) == (m, n) and got.dtype == dtype and not got.requires_grad
        close(got, ref * ref if square else ref, bnd * bnd if square else bnd, TOL[dtype], f"K9e cell square={square}")
        assert torch.equal(got, pair_distances(x, PairList.all_pairs(n, m), c, square=square, box=Cell(H)).amin(0).reshape(m, n))
    own = min_distances(x, box=Cell(dev(H)))  # (a cell on the GPU)
    assert (own.diagonal() == 0).all()
    assert torch.equal(own, pair_distances(x, PairList.all_pairs(n), box=Cell(H)).amin(0).reshape(n, n))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_from_cutoff_within_the_safe_radius_is_the_brute_force_list(dtype, kind):
    T, n = 6, 30
    H = stored(R.cell_of(kind, T, 63), dtype)
    xn = stored(R.wrap_positions(lattice_sites(T, n, 61), H), dtype)
    i, j = np.triu_indices(n, 1)
    Hs = np.broadcast_to(H, (T, 3, 3))
    mins = np.min([R.brute_min(xn[t][j] - xn[t][i], Hs[t])[1] for t in range(T)], axis=0)  # the TRUE minimum image
    r_safe = R.safe_radius(H)
    v = np.sort(mins[(mins >= 0.6 * r_safe) & (mins <= r_safe)])
    k = int(np.argmax(np.diff(v)))
    cut = float(0.5 * (v[k] + v[k + 1]))
    assert cut <= r_safe and np.min(np.abs(mins - cut)) > 1e-4 * cut  # no reference minimum within 1e-4 of the cutoff
    want = [(a, b) for a, b, d in zip(i, j, mins) if d <= cut]
    assert 20 < len(want) < len(i)
    x = dev(xn, dtype)
    reset()
    pl = PairList.from_cutoff(x, cut, box=Cell(H))
    assert launched() == pairmin_names(dtype, False)
    assert [tuple(p) for p in pl.pairs] == want
    assert [tuple(p) for p in PairList.from_cutoff(x, cut, box=Cell(dev(H))).pairs] == want  # a cell on the GPU
    ex = [want[1], want[5][::-1]]
    assert [tuple(p) for p in PairList.from_cutoff(x, cut, box=Cell(H), exclude=ex).pairs] == [p for p in want if p not in (want[1], want[5])]
    with pytest.raises(ValueError, match="safe radius"):
        PairList.from_cutoff(x, r_safe * 1.01, box=Cell(H))
    PairList.from_cutoff(x, r_safe * 1.01, box=Cell(dev(H)))  # (on the GPU the condition is the caller's part)
    assert tuple(pair_distances(x, pl, box=Cell(H)).shape) == (T, len(want))  # the list feeds the list kernels


# ------------------------------------------------------------------ 3. a diagonal cell gives the bits of the box form
def diagonal(L, T):
    """The (T, 3, 3) diagonal cells of box lengths L ((3,) or (T, 3))."""
    return np.stack([np.diag(l) for l in np.broadcast_to(L, (T, 3))])


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_box", "box_per_frame"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_diagonal_cell_gives_the_box_forms_bits_in_k9c_k9d_k9e(dtype, per_frame):
    for (_, pairs, m, n), T in ((CASES[1], 9), (CASES[3], 3), (CASES[2], 67)):
        pl = PairList(pairs, n, m)
        tab = pl.on(DEV)
        x, c, v, y, w = base.list_operands(T, pairs, m, n, dtype)
        L = frame_boxes(T, 900) if per_frame else R.DIAG_LENGTHS
        box, cell = dev(L, dtype), rows(diagonal(L, T), T, dtype)
        reset()
        for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
            assert torch.equal(K.pair_list_dist(x, c, tab, mode, v, y, box=cell), K.pair_list_dist(x, c, tab, mode, v, y, box=box))
        dvs = K.pair_list_dist(x, c, tab, box=box)
        outs = (F32,) if dtype == F32 else (F64, F32)
        for outd in outs:
            for kw in ({}, {"dv": dvs}):
                a, b = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=cell, **kw)
                a0, b0 = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=box, **kw)
                assert torch.equal(a, a0) and torch.equal(b, b0)
        for square in (False, True):
            assert torch.equal(K.pair_min(x, c, square, box=cell), K.pair_min(x, c, square, box=box))
        names = launched()
        assert any(k.endswith(", 2>") for k in names) and any(not k.endswith(", 2>") for k in names)
        assert (np.abs(np.rint(list_disp(host(x), host(c), pairs) / R.DIAG_LENGTHS)) >= 1).any()
    # K9e over split frames
    T, m, n = 200, 3, 7
    x, c = dev(lattice_sites(T, n, 54), dtype), dev(lattice_sites(T, m, 55) + 0.4, dtype)
    L = frame_boxes(T, 56) if per_frame else R.DIAG_LENGTHS
    reset()
    assert torch.equal(K.pair_min(x, c, box=rows(diagonal(L, T), T, dtype)), K.pair_min(x, c, box=dev(L, dtype)))
    assert f"pairmin_reduce_kernel<{NAME[dtype]}>" in launched()
    # the public functions, from a Cell
    assert torch.equal(min_distances(x, c, box=Cell(diagonal(L, T) if per_frame else np.diag(L))), min_distances(x, c, box=L))


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_box", "box_per_frame"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_diagonal_cell_gives_the_box_forms_bits_in_k6_and_k11(dtype, per_frame):
    T, N = 17, 70
    x = dev(lattice_sites(T, N, 57), dtype)
    L = frame_boxes(T, 58) if per_frame else R.DIAG_LENGTHS
    box, cell = dev(L, dtype), rows(diagonal(L, T), T, dtype)
    assert torch.equal(K.pair_dist_var(x, box=cell), K.pair_dist_var(x, box=box))
    for got, ref in zip(K.pair_dist_moments(x, box=cell), K.pair_dist_moments(x, box=box)):
        assert torch.equal(got, ref) and torch.isfinite(ref).all()
    # K11, both forms, images included: a chain that is several cells long
    par = R.TREES["forest"](N)
    tab = MoleculeTree(par).on(DEV)
    for form in (K.WHOLE_LDS, K.WHOLE_GLOBAL):
        im, im0 = (torch.zeros((T, N, 3), dtype=torch.int32, device=DEV) for _ in range(2))
        got = K.make_whole(x, cell, tab, images=im, _form=form)
        ref = K.make_whole(x, box, tab, images=im0, _form=form)
        assert torch.equal(got, ref) and torch.equal(im, im0) and int(im.abs().max()) >= 1
    whole, images = make_whole(x, Cell(diagonal(L, T) if per_frame else np.diag(L)), MoleculeTree(par), return_images=True)
    whole0, images0 = make_whole(x, L, MoleculeTree(par), return_images=True)
    assert torch.equal(whole, whole0) and torch.equal(images, images0)


# ------------------------------------------------------------------ 4. K6
K6_N, K6_T = 70, 17  # two 64-tiles (a ragged one and a diagonal one), a ragged 8-frame stage, three frame splits


def k6_system(kind, dtype):
    """(x as stored, H as stored): K6_N sites wrapped into the cell, no displacement within 1e-9 of a tie."""
    H = stored(R.cell_of(kind, K6_T, 65), dtype)
    i, j = np.triu_indices(K6_N, 1)
    (xn, _), tie = R.tie_free_sites(lambda k: (R.wrap_positions(lattice_sites(K6_T, K6_N, 66 + k), H), np.zeros(1)),
                                    lambda a, _b: a[:, j] - a[:, i], H, dtype)
    assert R.tie_distance(xn[:, j] - xn[:, i], H) > 1e-9  # (float64 arithmetic on the stored values: tests/test_gpu_guess_box.py)
    return xn, H


def k6_reference(xn, H):
    d = np.linalg.norm(R.wrap(xn[:, None, :, :] - xn[:, :, None, :], H), axis=-1)
    return d.mean(0), d.var(0)


def k6_close(got, ref, what):
    err, bound = float(np.max(np.abs(got - ref))), 1e-10 * max(1.0, float(ref.max()))
    print(f"{what}: max |got - ref| = {err:.3e}, bound {bound:.3e}")
    assert err < bound, f"{what}: {err:.3e} >= {bound:.3e}"


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_k6_variances_and_moments_under_a_cell_match_the_reference(dtype, kind):
    xn, H = k6_system(kind, dtype)
    ksplit = (_lib.load().aggf_pair_dist_var_workspace_bytes(K6_T, K6_N) - 256) // (3 * 2 * 64 * 64 * 8)
    assert ksplit == 3  # more than one frame split
    x, cell = dev(xn, dtype), rows(H, K6_T, dtype)
    ref_mean, ref_var = k6_reference(xn, H)
    reset()
    var = K.pair_dist_var(x, box=cell).cpu().numpy()
    assert launched() == sorted(f"{k}<{NAME[dtype]}, 2>" for k in ("pair_stats_pbc_kernel", "pair_var_pbc_kernel"))
    k6_close(var, ref_var, f"var {kind}")
    mean, var2 = (a.cpu().numpy() for a in K.pair_dist_moments(x, box=cell))
    k6_close(mean, ref_mean, f"mean {kind}")
    k6_close(var2, ref_var, f"var (moments) {kind}")
    for a in (var, var2, mean):
        assert np.array_equal(a, a.T) and not np.diagonal(a).any()
    # a bad cell in the last frame (the single frame of the last split): NaN off the diagonal, 0 on it
    broken = np.array(np.broadcast_to(H, (K6_T, 3, 3)))
    broken[-1, 2, 0] = np.inf
    bad = K.pair_dist_var(x, box=rows(broken, K6_T, dtype)).cpu().numpy()
    off = ~np.eye(K6_N, dtype=bool)
    assert np.isnan(bad[off]).all() and not np.diagonal(bad).any()
    with pytest.raises(ValueError, match="cell"):
        guess_pairwise_constraints(x, box=Cell(rows(broken, K6_T, dtype).reshape(K6_T, 3, 3)))


def split_pair(T=40, seed=51):
    """Four atoms in a rhombic dodecahedron: 0 and 1 a rigid pair drifting across the skewed c face, 2 and 3 loose."""
    H = R.rhombic_dodecahedron()
    rng = np.random.default_rng(seed)
    centre = np.cumsum(0.4 * rng.standard_normal((T, 1, 3)), axis=0) + 0.3 * H[2]
    rigid = np.concatenate([centre, centre + np.array([0.5, 0.3, 0.7])], axis=1)
    whole = np.concatenate([rigid, rng.uniform(0, 4, (T, 2, 3))], axis=1)
    x = R.wrap_positions(whole, H)
    k = R.brick(x[:, 1] - x[:, 0], H)[1]
    assert (k[:, 2] != 0).any() and (k[:, 2] == 0).any(), "the pair is never split across the c face"
    return x, H


@pytest.mark.parametrize("on_gpu", [False, True], ids=["numpy", "gpu_tensors"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_the_guess_finds_a_pair_split_across_a_skewed_face_only_with_the_cell(dtype, on_gpu):
    x, H = split_pair()
    npdt = np.float32 if dtype == F32 else np.float64
    xs = dev(x, dtype) if on_gpu else x.astype(npdt)
    cell = Cell(dev(H)) if on_gpu else Cell(H)
    rigid = frozenset((0, 1))
    assert rigid in guess_pairwise_constraints(xs, box=cell, threshold=1e-3)
    assert rigid not in guess_pairwise_constraints(xs, threshold=1e-3)
    assert rigid not in guess_pairwise_constraints(xs, box=np.diagonal(H), threshold=1e-3)


# ------------------------------------------------------------------ 5. K11
def whole_names(dtype, form, rounds):
    if form == K.WHOLE_LDS:
        return [f"whole_lds_kernel<{NAME[dtype]}, 2>"]
    return sorted([f"whole_edge_kernel<{NAME[dtype]}, 2>", f"whole_shift_kernel<{NAME[dtype]}, 2>"]
                  + (["whole_jump_kernel"] if rounds else []))


@pytest.mark.parametrize("tree", sorted(R.TREES))
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_make_whole_under_a_cell_counts_exact_and_coordinates_within_three_roundings(tree, dtype, kind):
    for T, N in ((3, 23), (9, 70)):
        H = stored(R.cell_of(kind, T, 6), dtype)
        w, par = R.molecule(tree, T, N, H, dtype, 41 + N)
        u, k, tie, bound = R.whole_reference(w, H, par)
        assert tie > 2 * R.MARGIN[dtype] and np.abs(k).max() >= 1
        mt = MoleculeTree(par)
        assert mt.n_rounds >= (2 if tree == "forest" else 3) and (tree != "backward" or (par[:-1] > np.arange(N - 1)).all())
        assert tree != "forest" or (par < 0).sum() >= 3
        x, cell = dev(w, dtype), rows(H, T, dtype)
        tab = mt.on(DEV)
        outs = []
        for form in (K.WHOLE_LDS, K.WHOLE_GLOBAL):
            images = torch.zeros((T, N, 3), dtype=torch.int32, device=DEV)
            reset()
            got = K.make_whole(x, cell, tab, images=images, _form=form)
            assert launched() == whole_names(dtype, form, mt.n_rounds)
            assert got.dtype == dtype and torch.equal(x, dev(w, dtype))  # the input untouched
            assert np.array_equal(images.cpu().numpy(), k), f"image counts {kind} {tree} N={N} T={T} form {form}"
            R.assert_whole(host(got), u, bound, dtype, f"{kind} {tree} N={N} T={T} form {form}")
            y = x.clone()  # in place
            assert K.make_whole(y, cell, tab, out=y, _form=form) is y and torch.equal(y, got)
            outs.append(got)
        assert torch.equal(outs[0], outs[1]), "LDS form != global form"
        # the public function: a Cell on the host, return_images, inplace, whole already
        whole, images = make_whole(x, Cell(H), mt, return_images=True)
        assert torch.equal(whole, outs[0]) and np.array_equal(images.cpu().numpy(), k)
        y = x.clone()
        assert make_whole(y, Cell(H), mt, inplace=True) is y and torch.equal(y, whole)
        again, zero = make_whole(whole, Cell(H), mt, return_images=True)
        assert torch.equal(again, whole) and not zero.any()
        assert torch.equal(whole[:, dev(par < 0, torch.bool)], x[:, dev(par < 0, torch.bool)])  # a root never moves
        # every bonded pair's plain displacement is its brick image
        g = host(whole)
        has = par >= 0
        plain = g[:, has] - g[:, par[has]]
        assert np.array_equal(plain, R.wrap(plain, H))
        assert np.abs(R.brick(plain, H)[1]).max() == 0


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_on_either_side_of_the_lds_bound_of_the_triclinic_form(dtype):
    """The triclinic form stages nine numbers per frame where the box form stages six: its LDS bound is one atom lower."""
    bound = K.whole_lds_max_sites() - 1
    assert bound == 6823
    T = 2
    H = stored(R.frame_cells(T, 9), dtype)
    for N, form in ((bound, K.WHOLE_LDS), (bound + 1, K.WHOLE_GLOBAL)):
        w, par = R.molecule("forest", T, N, H, dtype, 47)
        u, k, tie, bnd = R.whole_reference(w, H, par)
        assert tie > 2 * R.MARGIN[dtype]
        mt = MoleculeTree(par)
        x = dev(w, dtype)
        reset()
        got, images = make_whole(x, Cell(H), mt, return_images=True)  # the library's choice
        assert launched() == whole_names(dtype, form, mt.n_rounds) and mt.n_rounds > 0
        assert np.array_equal(images.cpu().numpy(), k)
        R.assert_whole(host(got), u, bnd, dtype, f"N={N} {NAME[dtype]}")
        if form == K.WHOLE_LDS:
            assert torch.equal(K.make_whole(x, rows(H, T, dtype), mt.on(DEV), _form=K.WHOLE_GLOBAL), got)
        else:
            with pytest.raises(_lib.AggfError, match="LDS form"):
                K.make_whole(x, rows(H, T, dtype), mt.on(DEV), _form=K.WHOLE_LDS)


@pytest.mark.parametrize("form", [K.WHOLE_LDS, K.WHOLE_GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_make_whole_under_a_cell_bad_frames_and_non_finite_coordinates(dtype, form):
    T, N = 3, 23
    H = stored(R.frame_cells(T, 12), dtype)
    w, par = R.molecule("chain", T, N, H, dtype, 43)
    tab = MoleculeTree(par).on(DEV)
    x = dev(w, dtype)

    def run(xs, cell):
        images = torch.full((T, N, 3), 7, dtype=torch.int32, device=DEV)
        return K.make_whole(xs, cell, tab, images=images, _form=form), images

    good, good_k = run(x, rows(H, T, dtype))
    for _, (r, cidx), value in BAD:
        broken = H.copy()
        broken[1, r, cidx] = value
        got, k = run(x, rows(broken, T, dtype))
        assert torch.isnan(got[1]).all() and not k[1].any()  # every component NaN, the counts 0
        assert torch.equal(got[[0, 2]], good[[0, 2]]) and torch.equal(k[[0, 2]], good_k[[0, 2]])
    # a non-finite coordinate stays where it is; the atoms beyond it are placed from their own parents
    for value in (float("nan"), float("inf")):
        w2 = w.copy()
        w2[0, 5, 1] = value
        got, k = run(dev(w2, dtype), rows(H, T, dtype))
        g = host(got)
        assert (np.isnan(g[0, 5, 1]) if np.isnan(value) else g[0, 5, 1] == value)
        assert np.isfinite(np.delete(g[0].ravel(), 5 * 3 + 1)).all()
        assert torch.equal(got[1:], good[1:]) and torch.equal(k[1:], good_k[1:])
        assert torch.equal(got[0, :5], good[0, :5])  # the atoms before it on the chain are not touched by it


def test_make_whole_under_a_cell_has_the_identity_backward():
    T, N = 3, 23
    H = R.SKEW
    w, par = R.molecule("chain", T, N, H, F64, 44)
    mt = MoleculeTree(par)
    x = dev(w, grad=True)
    out = make_whole(x, Cell(H), mt)
    h = torch.randn_like(out)
    (g,) = torch.autograd.grad((out * h).sum(), x)
    assert torch.equal(g, h) and not torch.equal(out.detach(), x.detach())
    with pytest.raises(ValueError, match="inplace"):
        make_whole(x, Cell(H), mt, inplace=True)
    assert torch.autograd.gradcheck(lambda a: make_whole(a, Cell(H), mt), (x,), eps=1e-6, atol=1e-6, rtol=1e-6)


# ------------------------------------------------------------------ 6. the caller's stream
class GateCase:
    def __init__(self, name, families, build):
        self.name, self.group, self.entries, self.families = name, "cell", (), tuple(families)
        self.build, self.synchronises, self.env, self.cleanup = build, None, None, None


def gate_cases():
    from pairlist_ref import lattice_sites as sites

    T, m, n, P = 9, 6, 11, 70
    cell = np.broadcast_to(R.SKEW, (T, 3, 3)).reshape(T, 9)

    def lists(pull):
        def build():
            tab = PairList(random_list(P, m, n, 300, self_form=False), n, m).on(DEV)
            floats = [dev(sites(T, n, 58)), dev(sites(T, m, 59) + 0.4)]
            floats += [dev(np.random.default_rng(60).standard_normal((T, P)))] if pull else []
            floats += [dev(cell)]

            def call(x_, c_, *rest):
                if pull:
                    return K.pair_list_pull(rest[0], x_, c_, tab, box=rest[1])
                return K.pair_list_dist(x_, c_, tab, box=rest[0])
            return floats, call
        return build

    def pair_min():
        return [dev(sites(T, n, 51)), dev(sites(T, m, 52) + 0.4), dev(cell)], lambda x_, c_, b: K.pair_min(x_, c_, box=b)

    def pair_var():
        xn, H = k6_system("skew", F64)
        return [dev(xn), rows(H, K6_T, F64)], lambda x_, b: K.pair_dist_moments(x_, box=b)

    def whole(form):
        def build():
            w, par = R.molecule("forest", T, 131, R.SKEW, F64, 45)
            tab = MoleculeTree(par).on(DEV)

            def call(x, b):
                images = torch.zeros(tuple(x.shape), dtype=torch.int32, device=DEV)
                return K.make_whole(x, b, tab, images=images, _form=form), images
            return [dev(w), dev(cell)], call
        return build

    return [GateCase("cell_pair_list_dist", ["pairlist_pbc_kernel<double, 0, 2>"], lists(False)),
            GateCase("cell_pair_list_pull", ["pairlist_pull_pbc_kernel<double, double, false, 0, 2>"], lists(True)),
            GateCase("cell_pair_min", ["pairmin_kernel<double, true, 2>"], pair_min),
            GateCase("cell_pair_dist_moments", ["pair_stats_pbc_kernel<double, 2>", "pair_var_pbc_kernel<double, 2>"], pair_var),
            GateCase("cell_make_whole_lds", ["whole_lds_kernel<double, 2>"], whole(K.WHOLE_LDS)),
            GateCase("cell_make_whole_global", ["whole_edge_kernel<double, 2>", "whole_jump_kernel", "whole_shift_kernel<double, 2>"],
                     whole(K.WHOLE_GLOBAL))]


def test_the_triclinic_forms_run_on_the_callers_stream_and_never_wait(monkeypatch):
    """The method of tests/test_gpu_streams.py (tests/stream_gate.py) on the new launches: behind a gate that holds the
    caller's stream the calls return at once, and their results are those of the true data, not of the poison."""
    SG.run_behind_gate(gate_cases(), monkeypatch)


# ------------------------------------------------------------------ 7. end to end
N_BEADS, BEAD, E2E_T = 10, 4, 50
E2E_H = R.rhombic_dodecahedron(4.3)
COORD_TOL = 64 * np.finfo(np.float64).eps * float(np.abs(E2E_H).sum(0).max())  # tests/test_gpu_whole.py's 64 eps max(L)


def bead_trajectory(T=E2E_T):
    """40 atoms in 10 four-atom beads in a rhombic dodecahedron: (wrapped, forces, bonds).  A bead is a rigid triangle
    plus a fourth atom on a fluctuating bond, diffusing; every atom is wrapped into the cell."""
    rng = np.random.default_rng(20261019)
    n = N_BEADS * BEAD
    centre = rng.uniform(0, 1, (1, N_BEADS, 3)) @ E2E_H + np.cumsum(0.2 * rng.standard_normal((T, N_BEADS, 3)), axis=0)
    shape = rng.uniform(-0.45, 0.45, (1, N_BEADS, BEAD, 3))
    shape[:, :, 0] = 0.0
    x = centre[:, :, None, :] + shape
    x[:, :, 3] += 0.1 * rng.standard_normal((T, N_BEADS, 3))
    wrapped = R.wrap_positions(x.reshape(T, n, 3), E2E_H)
    forces = 30 * rng.standard_normal(wrapped.shape)
    first = np.arange(N_BEADS) * BEAD
    bonds = np.concatenate([np.stack([first, first + 1], 1), np.stack([first + 1, first + 2], 1),
                            np.stack([first + 2, first], 1), np.stack([first + 2, first + 3], 1)])
    return wrapped, forces, bonds


RIGID = {frozenset((BEAD * c + i, BEAD * c + j)) for c in range(N_BEADS) for i, j in ((0, 1), (0, 2), (1, 2))}


def reference_unwrap(wrapped, bonds):
    """(coordinates made whole by the reference, its constraint set): the tree walk of cell_ref on the forest that
    ``MoleculeTree.from_bonds`` builds, and the pairs whose brick-image distance has a standard deviation below 1e-3."""
    mt = MoleculeTree.from_bonds(wrapped.shape[1], bonds)
    u, k, tie, _ = R.whole_reference(wrapped, E2E_H, mt.parent)
    assert tie > 1e-9 and np.abs(k).max() >= 1
    whole = u.astype(np.float64)
    d = np.linalg.norm(R.wrap(whole[:, None, :, :] - whole[:, :, None, :], E2E_H), axis=-1)
    i, j = np.nonzero(np.triu(d.std(0) < 1e-3, 1))
    return whole, {frozenset((int(a), int(b))) for a, b in zip(i, j)}


def bead_map():
    return LinearMap([list(range(BEAD * c, BEAD * c + BEAD)) for c in range(N_BEADS)], n_fg_sites=N_BEADS * BEAD)


@pytest.mark.parametrize("on_gpu", [False, True], ids=["numpy", "gpu_tensors"])
def test_project_forces_on_a_wrapped_dodecahedron_system(on_gpu):
    wrapped, forces, bonds = bead_trajectory()
    whole, constraints = reference_unwrap(wrapped, bonds)
    assert constraints == RIGID
    spread = whole.reshape(E2E_T, N_BEADS, BEAD, 3) - wrapped.reshape(E2E_T, N_BEADS, BEAD, 3)
    split = np.abs(spread - spread[:, :, :1]).max(axis=(2, 3)) > 1e-9  # (frame, bead): the wrap splits the bead
    assert split.any(axis=1).sum() >= 10 and not split.all()
    cmap = bead_map()
    conv = dev if on_gpu else (lambda a: a)
    out = (lambda a: a.cpu().numpy()) if on_gpu else (lambda a: a)
    kw = dict(l2_regularization=1.0)
    ref = project_forces(conv(whole), conv(forces), cmap, constrained_inds=set(constraints), **kw)
    given = conv(wrapped)
    keep = given.clone() if on_gpu else given.copy()
    cell = Cell(dev(E2E_H)) if on_gpu else Cell(E2E_H)
    got = project_forces(given, conv(forces), cmap, box=cell, bonds=bonds, **kw)
    assert (torch.equal(given, keep) if on_gpu else np.array_equal(given, keep)), "the caller's array was written"
    assert got["constraints"] == constraints
    assert np.array_equal(got["tmap"].force_map.standard_matrix, ref["tmap"].force_map.standard_matrix)
    assert np.array_equal(out(got["mapped_forces"]), out(ref["mapped_forces"]))
    err = np.abs(out(got["mapped_coords"]) - out(ref["mapped_coords"])).max()
    print(f"mapped_coords: max |wrapped + cell + bonds - reference| = {err:.3e}, bound {COORD_TOL:.3e}")
    assert err <= COORD_TOL
    # the defect without bonds=: the cell alone finds the constraints but leaves the split beads' averages off
    alone = project_forces(given, conv(forces), cmap, box=cell, **kw)
    assert alone["constraints"] == constraints
    off = np.abs(out(alone["mapped_coords"]) - out(ref["mapped_coords"])).max(axis=2)
    assert (off[split] > 0.2 * R.safe_radius(E2E_H)).all() and (off[~split] <= COORD_TOL).all()
    # and without the cell the guess misses rigid pairs
    assert not RIGID <= project_forces(given, conv(forces), cmap, **kw)["constraints"]


def test_grid_cv_under_a_cell_hands_each_training_subset_its_frames():
    wrapped, forces, bonds = bead_trajectory()
    whole, constraints = reference_unwrap(wrapped, bonds)
    cmap = bead_map()
    grid = {"l2_regularization": [1.0, 1e3]}
    per_frame = Cell(np.broadcast_to(E2E_H, (E2E_T, 3, 3)).copy())  # (one cell per frame: the folds index it)
    # (the loop over project_forces on both sides: the one-pass forms take explicit constraints only)
    plain = project_forces_grid_cv(grid, whole, forces, n_folds=2, rng=np.random.default_rng(0), coord_map=cmap,
                                   constrained_inds=set(constraints), reuse_gram=False)
    for cell in (Cell(E2E_H), per_frame):
        boxed = project_forces_grid_cv(grid, wrapped, forces, n_folds=2, rng=np.random.default_rng(0), coord_map=cmap,
                                       box=cell, bonds=bonds, reuse_gram=False)
        assert set(boxed["scores"]) == set(plain["scores"]) and len(boxed["scores"]) == 2
        for key, want in plain["scores"].items():
            got = boxed["scores"][key]
            print(f"{key}: {got!r} with the cell and bonds, {want!r} on the reference's coordinates")
            assert boxed["n_runs"][key] == plain["n_runs"][key] == 2
            assert abs(got - want) <= 1e-10 * abs(want)
