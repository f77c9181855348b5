"""Periodic boxes and cutoff lists, host side (no GPU): ``distances`` / ``pair_distances`` / ``min_distances`` with a
``box`` on CPU tensors and NumPy inputs against tests/pbc_ref.py, the three pair-list Functions over kernels restated
in torch (where the box goes at first and second order, and that an open call carries none), ``PairList.from_cutoff``
and ``PairList.all_pairs``, and the boxes that are refused."""
import numpy as np
import pytest
import torch

import aggforce_amd._kernels as K
import aggforce_amd.jaxutil as jaxutil
import pairlist_ref
import pbc_ref
from aggforce_amd._autograd import PairListDist, PairListDot, PairListPull
from aggforce_amd.jaxutil import PairList, distances, distances_in_box, min_distances, pair_distances
from pairlist_ref import lattice_sites, random_list, triangle
from pbc_ref import BOX, frame_boxes, wrap

GC = dict(eps=1e-6, atol=1e-5, rtol=1e-5)


def imaged(xn, seed):
    """``xn`` with some sites moved by whole box lengths (an unwrapped trajectory)."""
    k = np.random.default_rng(seed).integers(-2, 3, (1,) + xn.shape[1:])
    return xn + k * BOX


def test_the_new_names_are_exported():
    for name in ("min_distances", "pair_distances", "distances", "PairList"):
        assert hasattr(jaxutil, name)
    assert callable(PairList.from_cutoff) and callable(PairList.all_pairs) and callable(K.pair_min)


# ------------------------------------------------------------------ plain torch routes against the reference
@pytest.mark.parametrize("make", [np.asarray, torch.tensor], ids=["numpy", "cpu"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["const", "frames"])
def test_cpu_and_numpy_inputs_wrap_as_the_reference(make, per_frame):
    T, n, m = 4, 7, 3
    xn, cn = imaged(lattice_sites(T, n, 1), 2), imaged(lattice_sites(T, m, 3) + 0.4, 4)
    L = frame_boxes(T, 5) if per_frame else BOX
    u = wrap(xn[:, None, :, :] - cn[:, :, None, :], L)
    assert (np.abs(u) <= 0.5 * pbc_ref.over(L, u) + 1e-12).all()
    assert (np.rint((xn[:, None] - cn[:, :, None]) / pbc_ref.over(L, u)) != 0).any()  # something is wrapped
    x, c = make(xn), make(cn)
    for box in (L, L.tolist(), torch.tensor(L)):
        np.testing.assert_allclose(distances_in_box(x, box, c, return_displacements=True).numpy(), u, rtol=0, atol=1e-12)
        np.testing.assert_allclose(distances_in_box(x, box, c).numpy(), np.sqrt((u * u).sum(-1)), rtol=1e-13)
        np.testing.assert_allclose(distances_in_box(x, box, c, square=True).numpy(), (u * u).sum(-1), rtol=1e-13)
    us = wrap(xn[:, None, :, :] - xn[:, :, None, :], L)
    ds = np.sqrt((us * us).sum(-1))
    np.testing.assert_allclose(distances_in_box(x, L).numpy(), ds, rtol=1e-13, atol=1e-14)
    i, j = np.triu_indices(n, 1)
    np.testing.assert_allclose(distances_in_box(x, L, return_matrix=False).numpy(), ds[:, i, j], rtol=1e-13)
    pairs = random_list(9, m, n, 6, self_form=False)
    np.testing.assert_allclose(pair_distances(x, pairs, c, box=L).numpy(),
                               np.sqrt((u * u).sum(-1))[:, pairs[:, 0], pairs[:, 1]], rtol=1e-13)
    np.testing.assert_allclose(min_distances(x, c, box=L).numpy(), np.sqrt((u * u).sum(-1)).min(0), rtol=1e-13)
    np.testing.assert_allclose(min_distances(x, square=True, box=L).numpy(), (us * us).sum(-1).min(0), rtol=1e-13,
                               atol=1e-14)
    assert tuple(min_distances(x, c).shape) == (m, n) and not min_distances(x, c).requires_grad
    np.testing.assert_allclose(min_distances(x, c).numpy(),
                               np.linalg.norm(xn[:, None] - cn[:, :, None], axis=-1).min(0), rtol=1e-13)


def test_one_box_for_all_frames_is_the_same_box_repeated():
    T, n = 5, 6
    x = torch.tensor(imaged(lattice_sites(T, n, 7), 8))
    rep = np.tile(BOX, (T, 1))
    for fn in (lambda b: distances_in_box(x, b), lambda b: distances_in_box(x, b, return_displacements=True),
               lambda b: pair_distances(x, triangle(n), box=b), lambda b: min_distances(x, box=b)):
        assert torch.equal(fn(BOX), fn(rep))


def test_gradients_flow_through_the_wrap_on_the_cpu():
    x = torch.tensor(imaged(lattice_sites(2, 5, 9), 10), requires_grad=True)
    assert pbc_ref.tie_distance(pairlist_ref.list_disp(x.detach().numpy(), x.detach().numpy(), triangle(5)), BOX) > 1e-3
    assert torch.autograd.gradcheck(lambda a: pair_distances(a, triangle(5), box=BOX), (x,), **GC)
    assert not min_distances(x, box=BOX).requires_grad


# ------------------------------------------------------------------ rejected boxes
@pytest.mark.parametrize("box", [[4.0, 5.0], [[4.0, 5.0, 6.0]] * 2, np.ones((3, 3, 3)), [4.0, 0.0, 6.0],
                                 [4.0, -5.0, 6.0], [4.0, float("nan"), 6.0], [4.0, float("inf"), 6.0], "abc"],
                         ids=["short", "frames", "rank", "zero", "negative", "nan", "inf", "text"])
def test_bad_boxes_are_refused(box):
    x = torch.tensor(lattice_sites(3, 4, 11))
    for call in (lambda: distances_in_box(x, box), lambda: pair_distances(x, [[0, 1]], box=box),
                 lambda: min_distances(x, box=box), lambda: PairList.from_cutoff(x, 1.0, box=box)):
        with pytest.raises(ValueError):
            call()


def test_a_box_that_requires_grad_is_refused():
    x = torch.tensor(lattice_sites(3, 4, 12))
    box = torch.tensor(BOX, requires_grad=True)
    for call in (lambda: distances_in_box(x, box), lambda: pair_distances(x, [[0, 1]], box=box),
                 lambda: min_distances(x, box=box)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        PairListDist.apply(x, x, PairList([[0, 1]], 4), False, box)


# ------------------------------------------------------------------ the Functions over kernels restated in torch
@pytest.fixture
def kernels_in_torch(monkeypatch):
    monkeypatch.setattr(K, "pair_list_dist", pbc_ref.fake_pair_list_dist)
    monkeypatch.setattr(K, "pair_list_pull", pbc_ref.fake_pair_list_pull)


def sites(T, n, seed, shift=0.0):
    return torch.tensor(imaged(lattice_sites(T, n, seed) + shift, seed + 100), requires_grad=True)


def box_of(per_frame, T=2):
    return torch.tensor(frame_boxes(T, 13) if per_frame else BOX)


@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
@pytest.mark.parametrize("self_form", [False, True], ids=["cross", "self"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["const", "frames"])
def test_pairlistdist_under_a_box_gradcheck_and_gradgradcheck(kernels_in_torch, square, self_form, per_frame):
    x, c, box = sites(2, 5, 14), sites(2, 4, 15, 0.4), box_of(per_frame)
    if self_form:
        pl = PairList([[0, 1], [1, 2], [0, 4], [3, 2], [0, 1], [4, 1], [2, 0]], 5)
        fn, args = (lambda a: PairListDist.apply(a, a, pl, square, box)), (x,)
        u = pairlist_ref.list_disp(x.detach().numpy(), x.detach().numpy(), pl.pairs)
    else:
        pl = PairList(random_list(7, 4, 5, 16, self_form=False), 5, 4)
        fn, args = (lambda a, b: PairListDist.apply(a, b, pl, square, box)), (x, c)
        u = pairlist_ref.list_disp(x.detach().numpy(), c.detach().numpy(), pl.pairs)
    assert pbc_ref.tie_distance(u, box.numpy()) > 1e-3 and (np.rint(u / pbc_ref.over(box.numpy(), u)) != 0).any()
    assert torch.autograd.gradcheck(fn, args, **GC)
    assert torch.autograd.gradgradcheck(fn, args, **GC)


def test_pairlistpull_and_pairlistdot_under_a_box_gradcheck_and_gradgradcheck(kernels_in_torch):
    x, c, v, y = sites(2, 5, 17), sites(2, 4, 18, 0.4), sites(2, 5, 19), sites(2, 4, 20)
    pl = PairList(random_list(7, 4, 5, 21, self_form=False), 5, 4)
    box = box_of(True)
    assert pbc_ref.tie_distance(pairlist_ref.list_disp(x.detach().numpy(), c.detach().numpy(), pl.pairs), box.numpy()) > 1e-3
    w = torch.tensor(np.random.default_rng(22).standard_normal((2, 7)), requires_grad=True)
    for fn, args in ((lambda *a: PairListPull.apply(*a, pl, True, True, None, box), (w, x, c)),
                     (lambda *a: PairListDot.apply(*a, pl, box), (v, y, x, c))):
        assert torch.autograd.gradcheck(fn, args, **GC)
        assert torch.autograd.gradgradcheck(fn, args, **GC)


def force_matching(dist, x):
    u = torch.exp(-(dist(x) - 1) ** 2).sum()
    (g,) = torch.autograd.grad(u, x, create_graph=True)
    (gg,) = torch.autograd.grad((g * g).sum(), x)
    return g.detach(), gg


class Recorder:
    """Stand-ins that note, per kernel call, whether it carried a box and whether its sites were the coordinates."""

    def __init__(self, monkeypatch, coords):
        self.calls, self.coords = [], {t.data_ptr() for t in coords}
        monkeypatch.setattr(K, "pair_list_dist", lambda *a, **k: self.note("dist", a[0], k) or pbc_ref.fake_pair_list_dist(*a, **k))
        monkeypatch.setattr(K, "pair_list_pull", lambda *a, **k: self.note("pull", a[1], k) or pbc_ref.fake_pair_list_pull(*a, **k))

    def note(self, kind, x, kwargs):
        self.calls.append((kind, "box" in kwargs, x.data_ptr() in self.coords))


@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
def test_the_box_reaches_every_call_that_forms_a_displacement_of_coordinates(monkeypatch, square):
    """First and second order.  Every K9c call, and every K9d call whose sites are the coordinates, gets the box; the
    K9d calls whose "sites" are tangents (the derivative of a pull with respect to its coordinates) sum W (G_j - G_i),
    which is no displacement: wrapping it would be wrong, so they stay open."""
    x = sites(3, 5, 23)
    box = torch.tensor(BOX)
    rec = Recorder(monkeypatch, [x])
    g, gg = force_matching(lambda z: PairListDist.apply(z, z, PairList.upper_triangle(5), square, box), x)
    kinds = {c[0] for c in rec.calls}
    assert kinds == {"dist", "pull"} and len(rec.calls) >= 4
    for kind, has_box, on_coords in rec.calls:
        assert has_box == on_coords, rec.calls
    assert all(has_box for kind, has_box, _ in rec.calls if kind == "dist")
    assert any(kind == "pull" and not has_box for kind, has_box, _ in rec.calls)  # a second-order tangent pull ran
    # and the result is the derivative of the wrapped potential
    xr = x.detach().clone().requires_grad_(True)
    i, j = triangle(5).T

    def plain(z):
        u = pbc_ref.torch_wrap(z[:, j] - z[:, i], box)
        return (u * u).sum(-1) if square else torch.linalg.vector_norm(u, dim=-1)

    g_ref, gg_ref = force_matching(plain, xr)
    torch.testing.assert_close(g, g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg, gg_ref, rtol=1e-10, atol=1e-9)


def test_without_a_box_no_call_carries_a_box_argument(monkeypatch):
    x = sites(3, 5, 24)
    rec = Recorder(monkeypatch, [x])
    force_matching(lambda z: PairListDist.apply(z, z, PairList.upper_triangle(5), False), x)
    force_matching(lambda z: pair_distances(z, triangle(5), square=True), x)
    assert rec.calls and not any(has_box for _, has_box, _ in rec.calls)
    # the stand-ins of tests/test_pairlist_host.py, which accept no `box`, still serve
    monkeypatch.setattr(K, "pair_list_dist", pairlist_ref.fake_pair_list_dist)
    monkeypatch.setattr(K, "pair_list_pull", pairlist_ref.fake_pair_list_pull)
    g, gg = force_matching(lambda z: PairListDist.apply(z, z, PairList.upper_triangle(5), False), x)
    assert torch.isfinite(gg).all()


def test_the_box_is_cast_to_the_dtype_of_each_call(kernels_in_torch):
    x = torch.tensor(imaged(lattice_sites(2, 5, 25), 26), dtype=torch.float32, requires_grad=True)
    c = torch.tensor(lattice_sites(2, 4, 27), requires_grad=True)
    pl = PairList(random_list(7, 4, 5, 28, self_form=False), 5, 4)
    d = PairListDist.apply(x, c, pl, False, torch.tensor(BOX, dtype=torch.float32))  # (the stand-ins assert the dtype)
    gx, gc = torch.autograd.grad(d.sum(), (x, c))
    assert d.dtype == torch.float64 and gx.dtype == torch.float32 and gc.dtype == torch.float64


# ------------------------------------------------------------------ all_pairs and from_cutoff
def test_all_pairs_is_the_matrix_in_row_major_order_and_is_cached():
    pl = PairList.all_pairs(4)
    assert pl.n_cross is None and pl.n_sites == 4 and pl.n_pairs == 16
    assert np.array_equal(pl.pairs, [[i, j] for i in range(4) for j in range(4)])
    cross = PairList.all_pairs(5, 3)
    assert (cross.n_sites, cross.n_cross, cross.n_pairs) == (5, 3, 15)
    assert np.array_equal(cross.pairs, [[i, j] for i in range(3) for j in range(5)])
    assert PairList.all_pairs(5, 3) is cross and PairList.all_pairs(4) is pl and PairList.all_pairs(4, 4) is not pl
    assert PairList.all_pairs(0).n_pairs == 0 and PairList.all_pairs(3, 0).n_pairs == 0
    x, c = torch.tensor(lattice_sites(3, 5, 29)), torch.tensor(lattice_sites(3, 3, 30))
    assert torch.equal(pair_distances(x, cross, c, box=BOX).reshape(3, 3, 5), distances_in_box(x, BOX, c))


def cutoff_in_a_gap(vals, lo, hi):
    """The middle of the widest gap between consecutive sorted values inside [lo, hi]."""
    v = np.sort(vals[(vals >= lo) & (vals <= hi)])
    k = int(np.argmax(np.diff(v)))
    cut = 0.5 * (v[k] + v[k + 1])
    assert np.min(np.abs(vals - cut)) > 1e-4 * cut
    return float(cut)


@pytest.mark.parametrize("box", [None, BOX], ids=["open", "box"])
def test_from_cutoff_keeps_the_upper_triangle_in_order_and_drops_exclusions(box):
    T, n = 4, 12
    xn = imaged(lattice_sites(T, n, 31), 32) if box is not None else lattice_sites(T, n, 31)
    u = xn[:, None, :, :] - xn[:, :, None, :]
    dmin = np.linalg.norm(u if box is None else wrap(u, box), axis=-1).min(0)
    i, j = np.triu_indices(n, 1)
    cut = cutoff_in_a_gap(dmin[i, j], 1.2, 2.0)
    want = [(a, b) for a, b in zip(i, j) if dmin[a, b] <= cut]
    assert 5 < len(want) < len(i)
    for x in (xn, torch.tensor(xn)):
        pl = PairList.from_cutoff(x, cut, box=box)
        assert (pl.n_sites, pl.n_cross) == (n, None) and [tuple(p) for p in pl.pairs] == want
    far = next((a, b) for a, b in zip(i, j) if (a, b) not in want)
    ex = [want[0], want[3][::-1], far]  # either orientation; a pair that is not in the list anyway
    kept = [p for p in want if p not in (want[0], want[3])]
    for exclude in (np.array(ex), PairList(ex, n)):
        assert [tuple(p) for p in PairList.from_cutoff(xn, cut, box=box, exclude=exclude).pairs] == kept
    assert PairList.from_cutoff(xn, 0.0, box=box).n_pairs == 0


def test_from_cutoff_cross_form_nan_sites_and_refusals():
    T, n, m = 4, 9, 5
    xn, cn = imaged(lattice_sites(T, n, 33), 34), imaged(lattice_sites(T, m, 35) + 0.4, 36)
    dmin = np.linalg.norm(wrap(xn[:, None, :, :] - cn[:, :, None, :], BOX), axis=-1).min(0)
    cut = cutoff_in_a_gap(dmin.ravel(), 1.0, 2.0)
    want = [(a, b) for a in range(m) for b in range(n) if dmin[a, b] <= cut]
    pl = PairList.from_cutoff(xn, cut, cross_xyz=cn, box=BOX)
    assert (pl.n_sites, pl.n_cross) == (n, m) and [tuple(p) for p in pl.pairs] == want
    # in the cross form (i, j) and (j, i) are different pairs
    a, b = next(p for p in want if p[0] != p[1] and p[1] < m and (p[1], p[0]) not in want)
    assert [tuple(p) for p in PairList.from_cutoff(xn, cut, cn, BOX, exclude=[[b, a]]).pairs] == want
    assert [tuple(p) for p in PairList.from_cutoff(xn, cut, cn, BOX, exclude=[[a, b]]).pairs] == [p for p in want if p != (a, b)]
    # a NaN coordinate in one frame: the pairs of its site are never kept
    bad = xn.copy()
    site = want[0][1]
    bad[2, site, 1] = np.nan
    assert np.isnan(min_distances(bad, cn, box=BOX).numpy()[:, site]).all()
    assert [tuple(p) for p in PairList.from_cutoff(bad, cut, cn, BOX).pairs] == [p for p in want if p[1] != site]
    for call in (lambda: PairList.from_cutoff(xn, 0.5 * BOX.min() + 1e-9, box=BOX),       # beyond half the box
                 lambda: PairList.from_cutoff(xn, 2.0, box=np.tile(BOX, (T, 1)) * np.linspace(1, 0.9, T)[:, None]),
                 lambda: PairList.from_cutoff(xn, -1.0), lambda: PairList.from_cutoff(xn, float("nan")),
                 lambda: PairList.from_cutoff(xn, 1.0, exclude=[[0, n]]),
                 lambda: PairList.from_cutoff(xn, 1.0, cross_xyz=cn, exclude=[[m, 0]])):
        with pytest.raises(ValueError):
            call()
    assert PairList.from_cutoff(xn, 0.5 * BOX.min(), box=BOX).n_pairs > 0  # half the box itself is allowed
