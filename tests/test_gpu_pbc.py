"""Periodic boxes on the GPU: the box forms of K9c / K9d (pairlist_pbc_kernel, pairlist_pull_pbc_kernel) and K9e
(pairmin_kernel, pairmin_reduce_kernel) -- every instantiation launched and checked by name -- against the float64
NumPy restatement of tests/pbc_ref.py, with the helpers, bounds and settings of tests/test_gpu_pairlist.py (``close``,
``TOL``, ``GC``) applied to bounds built from b = |d| + |rint(d / L)| L; then whole-box shifts, a box far larger than
the system (the open kernels bit for bit), the matrix form of ``distances`` over ``PairList.all_pairs``,
``min_distances`` against ``pair_distances(...).amin(0)`` bit for bit, ``PairList.from_cutoff`` against the reference
list, gradcheck / gradgradcheck, the force-matching double backward under a box, and bad boxes.

Inputs: ``lattice_sites``, unwrapped (displacements span up to three box lengths), the box (4.1, 5.3, 6.7), constant
or varying by a few percent per frame.  Elements near a tie of the wrap are masked as tests/pbc_ref.py describes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_pairlist as base  # noqa: E402  (close, TOL, GC, launched, reset, dev, host, list_operands, force_matching)
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd.jaxutil import PairList, distances_in_box, min_distances, pair_distances  # noqa: E402
from pairlist_ref import chain, lattice_sites, list_disp, pull_reference, random_list, triangle  # noqa: E402
from pbc_ref import BOX, MARGIN, MAX_MASKED, comp_bound, frame_boxes, over, tie_distance, tie_mask, torch_wrap, wrap  # noqa: E402

DEV = base.DEV
F32, F64 = torch.float32, torch.float64
TOL, NAME, LANE_DEG, FRAMES = base.TOL, base.NAME, base.LANE_DEG, base.FRAMES
dev, host, close, launched, reset = base.dev, base.host, base.close, base.launched, base.reset
BOX_KINDS = ["const", "frames"]

# (name, pairs, m or None for the self form, n)
CASES = ([(f"triangle{n}", triangle(n), None, n) for n in (2, 5, 65)]       # 65: 64 entries per site, the wave form
         + [("chain130", chain(130), None, 130)]                             # the lane form, more than one block
         + [(f"random{P}", random_list(P, 9, 9, 200 + P), None, 9) for P in (1, 63, 64, 65)]
         + [("cross", random_list(70, 6, 11, 300, self_form=False), 6, 11)])
CASE_IDS = [c[0] for c in CASES]


def box_for(kind, T, dtype, seed=0):
    return dev(frame_boxes(T, 900 + seed) if kind == "frames" else BOX, dtype)


def masked(got, ref, tie):
    """``got`` on the host in float64 with the reference's value wherever the element is near a tie."""
    g = got.detach().cpu().double()
    g[torch.from_numpy(tie)] = torch.from_numpy(ref)[torch.from_numpy(tie)]
    return g


def reference(x, c, pairs, box, dtype):
    """(raw displacements, wrapped, per-component bound b, tie mask) from the operands as stored."""
    raw = list_disp(host(x), host(c), pairs)
    L = host(box)
    tie = tie_mask(raw, L, MARGIN[dtype])
    assert tie.mean() <= MAX_MASKED, f"{tie.mean():.3g} of the elements are near a tie"
    return raw, wrap(raw, L), comp_bound(raw, L), tie


def pull_names(pl, ind, outd, dv):
    forms = {int(deg > LANE_DEG) for _, _, deg in pl.tables()}
    return sorted(f"pairlist_pull_pbc_kernel<{NAME[ind]}, {NAME[outd]}, {'true' if dv else 'false'}, {f}>" for f in forms)


def test_the_inputs_span_several_box_lengths_and_both_forms_of_the_pull_kernel():
    raw = list_disp(lattice_sites(3, 130, 1), lattice_sites(3, 130, 1), triangle(130))
    assert np.abs(np.rint(raw / BOX)).max() >= 2
    degs = {name: [deg for _, _, deg in PairList(pairs, n, m).tables()] for name, pairs, m, n in CASES}
    assert max(degs["chain130"]) <= 2 and max(degs["triangle5"]) <= LANE_DEG < min(degs["triangle65"])


# ------------------------------------------------------------------ 1. K9c / K9d box forms vs NumPy float64
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", BOX_KINDS)
def test_k9c_box_form_every_mode_matches_numpy(case, dtype, kind):
    _, pairs, m, n = case
    tab = PairList(pairs, n, m).on(DEV)
    for T in FRAMES:
        x, c, v, y, _ = base.list_operands(T, pairs, m, n, dtype)
        box = box_for(kind, T, dtype, T)
        raw, u, b, tie = reference(x, c, pairs, box, dtype)
        g = list_disp(host(v), host(y), pairs)
        sq, bsq = (u * u).sum(-1), (b * b).sum(-1)
        reset()
        d = K.pair_list_dist(x, c, tab, K.PAIR_DIST, box=box)
        s = K.pair_list_dist(x, c, tab, K.PAIR_SQDIST, box=box)
        o = K.pair_list_dist(x, c, tab, K.PAIR_DOT, v, y, box=box)
        assert launched() == [f"pairlist_pbc_kernel<{NAME[dtype]}, {mode}>" for mode in (0, 1, 2)]
        for got in (d, s, o):
            assert got.dtype == dtype and tuple(got.shape) == (T, len(pairs))
        close(masked(d, np.sqrt(sq), tie), np.sqrt(sq), np.sqrt(bsq), TOL[dtype], "K9c box DIST")
        close(masked(s, sq, tie), sq, bsq, TOL[dtype], "K9c box SQDIST")
        close(masked(o, (g * u).sum(-1), tie), (g * u).sum(-1), (np.abs(g) * b).sum(-1), TOL[dtype], "K9c box DOT")
        assert (host(d)[~tie] <= 0.5 * np.linalg.norm(over(host(box), u) + 0 * u, axis=-1)[~tie] * (1 + 1e-6)).all()
        same = pairs[:, 0] == pairs[:, 1]
        if m is None and same.any():
            assert (d[:, torch.tensor(same, device=DEV)] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32)], ids=["f32", "f64", "f64-f32"])
@pytest.mark.parametrize("kind", BOX_KINDS)
def test_k9d_box_form_both_sums_match_numpy_and_repeat_bit_for_bit(case, ind, outd, kind):
    _, pairs, m, n = case
    pl = PairList(pairs, n, m)
    tab = pl.on(DEV)
    rows = n if m is None else m
    tol = max(TOL[ind], TOL[outd])
    for T in FRAMES:
        x, c, _, _, w = base.list_operands(T, pairs, m, n, ind)
        box = box_for(kind, T, ind, T)
        raw, u, b, tie = reference(x, c, pairs, box, ind)
        wn = host(w)
        wn[tie] = 0  # (a site's sum must not depend on which image a tie took)
        w = dev(wn, ind)
        wn = host(w)

        def bounds(weights):
            ab, bb, _, _ = pull_reference(np.abs(weights), b, pairs, rows, n)
            return ab, -bb

        a_ref, b_ref, _, _ = pull_reference(wn, u, pairs, rows, n)
        a_bnd, b_bnd = bounds(wn)
        reset()
        a, bsum = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=box)
        assert launched() == pull_names(pl, ind, outd, False)
        assert a.dtype == outd and bsum.dtype == outd and tuple(a.shape) == (T, n, 3) and tuple(bsum.shape) == (T, rows, 3)
        close(a, a_ref, a_bnd, tol, "K9d box A")
        close(bsum, b_ref, b_bnd, tol, "K9d box B")
        a2, b2 = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=box)
        assert torch.equal(a, a2) and torch.equal(bsum, b2)
        a1, none = K.pair_list_pull(w, x, c, tab, want_b=False, out_dtype=outd, box=box)
        assert none is None and torch.equal(a1, a)
        none, b1 = K.pair_list_pull(w, x, c, tab, want_a=False, out_dtype=outd, box=box)
        assert none is None and torch.equal(b1, bsum)
        # the distance form: w / dv where dv > 0, else 0
        dv = K.pair_list_dist(x, c, tab, K.PAIR_DIST, box=box)
        dvn = host(dv)
        wq = np.where(dvn > 0, wn / np.where(dvn > 0, dvn, 1.0), 0.0)
        a_ref, b_ref, _, _ = pull_reference(wq, u, pairs, rows, n)
        a_bnd, b_bnd = bounds(wq)
        reset()
        a, bsum = K.pair_list_pull(w, x, c, tab, dv=dv, out_dtype=outd, box=box)
        assert launched() == pull_names(pl, ind, outd, True)
        assert torch.isfinite(a).all() and torch.isfinite(bsum).all()
        close(a, a_ref, a_bnd, tol, "K9d box A (Dv)")
        close(bsum, b_ref, b_bnd, tol, "K9d box B (Dv)")
        a2, b2 = K.pair_list_pull(w, x, c, tab, dv=dv, out_dtype=outd, box=box)
        assert torch.equal(a, a2) and torch.equal(bsum, b2)


# ------------------------------------------------------------------ 2. whole-box shifts; a box far larger than the system
GRID = 2.0**16
EXACT_BOX = np.array([4.125, 5.25, 6.75])  # with sites on the 2^-16 grid, x + k L is exact in float32 for |k| <= 3


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_shift_by_whole_box_lengths_gives_the_unshifted_result(dtype):
    T, n = 3, 65
    pairs = triangle(n)
    tab = PairList(pairs, n).on(DEV)
    xn = np.round(lattice_sites(T, n, 21) * GRID) / GRID
    k = np.random.default_rng(22).integers(-3, 4, (T, n, 3))
    sn = xn + k * EXACT_BOX
    x, s, box = dev(xn, dtype), dev(sn, dtype), dev(EXACT_BOX, dtype)
    assert np.array_equal(host(x), xn) and np.array_equal(host(s), sn) and np.abs(k).max() == 3
    raw, u, _, tie0 = reference(x, x, pairs, box, dtype)
    _, us, b, tie1 = reference(s, s, pairs, box, dtype)
    tie = tie0 | tie1
    assert np.allclose(u[~tie], us[~tie], rtol=0, atol=1e-12)
    sq, bsq = (u * u).sum(-1), (b * b).sum(-1)
    close(masked(K.pair_list_dist(s, s, tab, K.PAIR_DIST, box=box), np.sqrt(sq), tie), np.sqrt(sq), np.sqrt(bsq),
          TOL[dtype], "shifted DIST")
    close(masked(K.pair_list_dist(s, s, tab, K.PAIR_SQDIST, box=box), sq, tie), sq, bsq, TOL[dtype], "shifted SQDIST")
    wn = np.random.default_rng(23).standard_normal((T, len(pairs)))
    wn[tie] = 0
    w = dev(wn, dtype)
    a_ref, b_ref, _, _ = pull_reference(host(w), u, pairs, n, n)
    a_bnd, b_bnd, _, _ = pull_reference(np.abs(host(w)), b, pairs, n, n)
    a, bsum = K.pair_list_pull(w, s, s, tab, box=box)
    close(a, a_ref, a_bnd, TOL[dtype], "shifted A")
    close(bsum, b_ref, -b_bnd, TOL[dtype], "shifted B")


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", BOX_KINDS)
def test_a_box_far_larger_than_the_system_gives_the_open_kernels_bits(dtype, kind):
    for pairs, m, n in ((triangle(65), None, 65), (chain(130), None, 130), (random_list(70, 6, 11, 300, self_form=False), 6, 11)):
        tab = PairList(pairs, n, m).on(DEV)
        T = 67
        x, c, v, y, w = base.list_operands(T, pairs, m, n, dtype)
        box = dev(1e6 * (frame_boxes(T, 31) if kind == "frames" else BOX), dtype)
        for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
            assert torch.equal(K.pair_list_dist(x, c, tab, mode, v, y, box=box), K.pair_list_dist(x, c, tab, mode, v, y))
        dv = K.pair_list_dist(x, c, tab)
        for kw in ({}, {"dv": dv}):
            a, b = K.pair_list_pull(w, x, c, tab, box=box, **kw)
            a0, b0 = K.pair_list_pull(w, x, c, tab, **kw)
            assert torch.equal(a, a0) and torch.equal(b, b0)
        assert torch.equal(min_distances(x, None if m is None else c, box=box), min_distances(x, None if m is None else c))


# ------------------------------------------------------------------ 3. the matrix form; min_distances
@pytest.mark.parametrize("T,m,n", [(3, 3, 7), (2, 70, 130)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_the_matrix_form_under_a_box_is_the_list_over_all_pairs_reshaped(T, m, n, dtype):
    x, c = dev(lattice_sites(T, n, 41), dtype), dev(lattice_sites(T, m, 42) + 0.4, dtype)
    box = frame_boxes(T, 43)
    reset()
    for square in (False, True):
        got = distances_in_box(x, box, c, square=square)
        assert tuple(got.shape) == (T, m, n)
        assert torch.equal(got, pair_distances(x, PairList.all_pairs(n, m), c, square=square, box=box).reshape(T, m, n))
        own = distances_in_box(x, box, square=square)
        assert tuple(own.shape) == (T, n, n) and (own.diagonal(dim1=1, dim2=2) == 0).all()
        assert torch.equal(own, pair_distances(x, PairList.all_pairs(n), square=square, box=box).reshape(T, n, n))
        assert torch.equal(own, own.transpose(1, 2))  # (the wrap is odd)
    names = launched()
    assert names and all(k.startswith("pairlist_pbc_kernel") for k in names), names  # K9a launches nothing
    raw = host(x)[:, None, :, :] - host(c)[:, :, None, :]
    tie = tie_mask(raw, host(dev(box, dtype)), MARGIN[dtype])
    assert tie.mean() <= MAX_MASKED
    ref = np.linalg.norm(wrap(raw, host(dev(box, dtype))), axis=-1)
    bnd = np.linalg.norm(comp_bound(raw, host(dev(box, dtype))), axis=-1)
    close(masked(distances_in_box(x, box, c), ref, tie), ref, bnd, TOL[dtype], "matrix form")


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.isnan(a), torch.isnan(b)) and \
        torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def pairmin_names(dtype, pbc, split):
    names = [f"pairmin_kernel<{NAME[dtype]}, {'true' if pbc else 'false'}>"]
    return sorted(names + ([f"pairmin_reduce_kernel<{NAME[dtype]}>"] if split else []))


@pytest.mark.parametrize("T,m,n,split", [(1, 1, 1, False), (5, 3, 7, False), (67, 70, 257, True)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["open"] + BOX_KINDS)
def test_min_distances_is_the_amin_of_pair_distances_bit_for_bit(T, m, n, split, dtype, kind):
    x, c = dev(lattice_sites(T, n, 51), dtype), dev(lattice_sites(T, m, 52) + 0.4, dtype)
    box = None if kind == "open" else frame_boxes(T, 53) if kind == "frames" else BOX
    for square in (False, True):
        reset()
        got = min_distances(x, c, square=square, box=box)
        own = min_distances(x, square=square, box=box)
        assert launched() == pairmin_names(dtype, box is not None, split)
        assert tuple(got.shape) == (m, n) and got.dtype == dtype and not got.requires_grad
        assert torch.equal(got, pair_distances(x, PairList.all_pairs(n, m), c, square=square, box=box).amin(0).reshape(m, n))
        assert torch.equal(own, pair_distances(x, PairList.all_pairs(n), square=square, box=box).amin(0).reshape(n, n))
        assert (own.diagonal() == 0).all()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["open", "frames"])
def test_min_distances_over_split_frames_with_a_nan_site_and_an_empty_side(dtype, kind):
    T, m, n = 300, 3, 7  # one tile: the plan splits the frames five ways
    xn = lattice_sites(T, n, 54)
    xn[100, 2, 1] = np.nan
    x, c = dev(xn, dtype), dev(lattice_sites(T, m, 55) + 0.4, dtype)
    box = None if kind == "open" else frame_boxes(T, 56)
    reset()
    got, own = min_distances(x, c, box=box), min_distances(x, box=box)
    assert launched() == pairmin_names(dtype, box is not None, True)
    touched = np.zeros((n, n), dtype=bool)
    touched[2, :] = touched[:, 2] = True
    assert np.array_equal(np.isnan(host(got)), np.tile(np.arange(n) == 2, (m, 1)))
    assert np.array_equal(np.isnan(host(own)), touched)
    assert same_bits(got, pair_distances(x, PairList.all_pairs(n, m), c, box=box).amin(0).reshape(m, n))
    assert same_bits(own, pair_distances(x, PairList.all_pairs(n), box=box).amin(0).reshape(n, n))
    reset()
    assert tuple(min_distances(x, c[:, :0], box=box).shape) == (0, n)
    assert tuple(min_distances(x[:, :0], c, box=box).shape) == (m, 0)
    none = min_distances(x[:0], c[:0], box=None if box is None else box[:0])
    assert tuple(none.shape) == (m, n) and torch.isinf(none).all()
    assert launched() == []


# ------------------------------------------------------------------ 4. from_cutoff
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["open"] + BOX_KINDS)
def test_from_cutoff_is_the_reference_list(dtype, kind):
    T, m, n = 20, 9, 40
    x, c = dev(lattice_sites(T, n, 61), dtype), dev(lattice_sites(T, m, 62) + 0.4, dtype)
    box = None if kind == "open" else dev(frame_boxes(T, 63, 0.01) if kind == "frames" else BOX, dtype)
    half = np.inf if box is None else 0.5 * host(box).min()

    def minima(a, b):
        raw = host(a)[:, None, :, :] - host(b)[:, :, None, :]
        return np.linalg.norm(raw if box is None else wrap(raw, host(box)), axis=-1).min(0)

    def cutoff(vals):
        v = np.sort(vals[(vals >= 1.4) & (vals <= min(half, 2.0))])
        k = int(np.argmax(np.diff(v)))
        cut = 0.5 * (v[k] + v[k + 1])
        assert np.min(np.abs(vals - cut)) > 1e-4 * cut  # no reference minimum within 1e-4 relative of the cutoff
        return float(cut)

    ref = minima(x, x)
    i, j = np.triu_indices(n, 1)
    cut = cutoff(ref[i, j])
    want = [(a, b) for a, b in zip(i, j) if ref[a, b] <= cut]
    assert 20 < len(want) < len(i)
    reset()
    pl = PairList.from_cutoff(x, cut, box=box)
    assert launched() == pairmin_names(dtype, box is not None, False)
    assert [tuple(p) for p in pl.pairs] == want
    ex = [want[1], want[5][::-1]]
    assert [tuple(p) for p in PairList.from_cutoff(x, cut, box=box, exclude=ex).pairs] == [p for p in want if p not in (want[1], want[5])]
    refc = minima(x, c)
    cutc = cutoff(refc.ravel())
    plc = PairList.from_cutoff(x, cutc, cross_xyz=c, box=box)
    assert (plc.n_sites, plc.n_cross) == (n, m)
    assert [tuple(p) for p in plc.pairs] == [(a, b) for a in range(m) for b in range(n) if refc[a, b] <= cutc]
    if box is not None:
        with pytest.raises(ValueError):
            PairList.from_cutoff(x, half * 1.01, box=box)
    # the list feeds the list kernels
    assert tuple(pair_distances(x, pl, box=box).shape) == (T, len(want))


# ------------------------------------------------------------------ 5. gradcheck / gradgradcheck (float64)
def imaged(xn, seed):
    return xn + np.random.default_rng(seed).integers(-2, 3, (1,) + xn.shape[1:]) * BOX


@pytest.mark.parametrize("form", ["self", "cross"])
@pytest.mark.parametrize("kind", BOX_KINDS)
@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
def test_gradcheck_and_gradgradcheck_under_a_box(form, kind, square):
    xn, cn = imaged(lattice_sites(2, 5, 71), 72), imaged(lattice_sites(2, 4, 73) + 0.4, 74)
    boxn = frame_boxes(2, 75) if kind == "frames" else BOX
    if form == "self":
        pairs = np.array(base.SELF7)
        raw = list_disp(xn, xn, pairs)
    else:
        pairs = np.array([[0, 1], [3, 2], [0, 4], [3, 2], [1, 1], [2, 0], [3, 4]])
        raw = list_disp(xn, cn, pairs)
    assert tie_distance(raw, boxn) > 1e-3 and (np.rint(raw / over(boxn, raw)) != 0).any()
    x, c, box = dev(xn, grad=True), dev(cn, grad=True), dev(boxn)
    if form == "self":
        pl = PairList(pairs, 5)
        fn, args = (lambda a: pair_distances(a, pl, square=square, box=box)), (x,)
    else:
        fn, args = (lambda a, b: pair_distances(a, pairs, cross_xyz=b, square=square, box=box)), (x, c)
    reset()
    assert torch.autograd.gradcheck(fn, args, **base.GC)
    assert torch.autograd.gradgradcheck(fn, args, **base.GC)
    names = launched()
    assert any(k.startswith("pairlist_pull_pbc_kernel<double") for k in names)
    assert any(k.startswith("pairlist_pbc_kernel<double, 2>") for k in names)


# ------------------------------------------------------------------ 6. force-matching double backward under a box
def cpu_force_matching(xn, boxn, skip=()):
    x = torch.tensor(xn, requires_grad=True)
    n = x.shape[1]
    i0, i1 = (torch.tensor(a) for a in zip(*[(i, j) for i in range(n) for j in range(i + 1, n) if (i, j) not in skip]))
    box = torch.tensor(boxn)
    return base.force_matching(lambda z: torch.linalg.vector_norm(torch_wrap(z[:, i1] - z[:, i0], box), dim=-1), x)


@pytest.mark.parametrize("T,n", [(3, 5), (5, 65)])
def test_force_matching_double_backward_under_a_box(T, n):
    xn = lattice_sites(T, n, 600 + n)
    boxn = frame_boxes(T, 81)
    reset()
    g, gg = base.force_matching(lambda z: distances_in_box(z, boxn, return_matrix=False), dev(xn, grad=True))
    names = launched()
    assert "pairlist_pbc_kernel<double, 2>" in names and any(k.startswith("pairlist_pull_pbc_kernel") for k in names)
    assert not any(k.startswith(("pairdist_kernel", "pairpull_kernel")) for k in names)
    assert torch.isfinite(gg).all(), "non-finite double backward"
    g_ref, gg_ref = cpu_force_matching(xn, boxn)
    torch.testing.assert_close(g.cpu(), g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg.cpu(), gg_ref, rtol=1e-10, atol=1e-9)


def test_force_matching_is_finite_with_two_sites_that_are_images_of_each_other():
    xn = np.round(lattice_sites(3, 5, 605) * GRID) / GRID
    xn[:, 3] = xn[:, 1] + EXACT_BOX * [1, 0, -1]  # (exact: the wrapped displacement is 0)
    x = dev(xn, grad=True)
    d = distances_in_box(x, EXACT_BOX, return_matrix=False)
    assert (d == 0).sum() == 3
    g, gg = base.force_matching(lambda z: distances_in_box(z, EXACT_BOX, return_matrix=False), x)
    assert torch.isfinite(g).all() and torch.isfinite(gg).all()
    g_ref, gg_ref = cpu_force_matching(xn, EXACT_BOX, skip={(1, 3)})
    torch.testing.assert_close(g.cpu(), g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg.cpu(), gg_ref, rtol=1e-10, atol=1e-9)


# ------------------------------------------------------------------ 7. a bad box in one frame
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("bad", [0.0, -4.1, float("nan"), float("inf")], ids=["zero", "negative", "nan", "inf"])
def test_a_bad_length_in_one_frame_makes_that_frame_nan_and_leaves_the_others_exact(dtype, bad):
    T = 3
    for pairs, n in ((triangle(65), 65), (chain(130)[:100], 130)):  # (the chain leaves sites without entries)
        tab = PairList(pairs, n).on(DEV)
        x, c, v, y, w = base.list_operands(T, pairs, None, n, dtype)
        good = frame_boxes(T, 91)
        broken = good.copy()
        broken[1, 1] = bad
        gbox, bbox = dev(good, dtype), dev(broken, dtype)
        for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
            ref = K.pair_list_dist(x, c, tab, mode, v, y, box=gbox)
            got = K.pair_list_dist(x, c, tab, mode, v, y, box=bbox)
            assert torch.isnan(got[1]).all() and torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
        for kw in ({}, {"dv": K.pair_list_dist(x, c, tab, box=gbox)}):
            ra, rb = K.pair_list_pull(w, x, c, tab, box=gbox, **kw)
            ga, gb = K.pair_list_pull(w, x, c, tab, box=bbox, **kw)
            for got, ref in ((ga, ra), (gb, rb)):
                assert torch.isnan(got[1]).all() and torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
                assert torch.isfinite(ref).all()
        assert torch.isnan(min_distances(x, box=bbox)).all() and torch.isfinite(min_distances(x, box=gbox)).all()
    # a box on the host is refused before any launch
    with pytest.raises(ValueError):
        pair_distances(x, pairs, box=broken)
