"""jaxutil.PairList and jaxutil.pair_distances on the host: validation, the upper-triangle list, the incidence tables
against a brute-force build, the plain-torch body for inputs that never reach a kernel, and the three list Functions of
aggforce_amd/_autograd.py (PairListDist / PairListPull / PairListDot) with the K9c / K9d kernels restated in torch:
their backward formulas and closure under differentiation.  CPU only."""
import numpy as np
import pytest
import torch

import aggforce_amd._kernels as K
import aggforce_amd.jaxutil as jaxutil
from aggforce_amd._autograd import PairListDist, PairListDot, PairListPull
from aggforce_amd.jaxutil import PairList, pair_distances
from pairlist_ref import (brute_tables, chain, fake_pair_list_dist, fake_pair_list_pull, lattice_sites, random_list)


def sites(T, n, seed, dtype=torch.float64, grad=True):
    return torch.tensor(lattice_sites(T, n, seed), dtype=dtype, requires_grad=grad)


def plain(x, pairs, c=None, square=False):
    pairs = torch.as_tensor(np.array(pairs))
    disp = x[:, pairs[:, 1]] - (x if c is None else c)[:, pairs[:, 0]]
    return (disp**2).sum(-1) if square else torch.linalg.vector_norm(disp, dim=-1)


# ------------------------------------------------------------------ PairList
def test_the_new_names_are_exported():
    assert jaxutil.PairList is PairList and jaxutil.pair_distances is pair_distances
    if hasattr(jaxutil, "__all__"):
        assert {"PairList", "pair_distances"} <= set(jaxutil.__all__)


@pytest.mark.parametrize("make", [lambda a: a.tolist(), lambda a: a.copy(), lambda a: a.astype(np.int32),
                                  lambda a: torch.tensor(a), lambda a: torch.tensor(a, dtype=torch.int32)],
                         ids=["list", "int64", "int32", "tensor", "tensor32"])
def test_pairlist_takes_any_integer_array_and_keeps_a_host_copy(make):
    src = np.array([[0, 1], [2, 4], [2, 4], [3, 3]])
    given = make(src)
    pl = PairList(given, 5)
    assert pl.pairs.dtype == np.int64 and np.array_equal(pl.pairs, src)
    assert (pl.n_pairs, pl.n_sites, pl.n_cross) == (4, 5, None)
    if isinstance(given, np.ndarray):
        given[0, 0] = 4
        assert pl.pairs[0, 0] == 0  # a copy
    cross = PairList(src, 5, n_cross=4)
    assert (cross.n_sites, cross.n_cross) == (5, 4)


def test_pairlist_accepts_an_empty_list():
    for empty in ([], np.zeros((0, 2), dtype=np.int64), torch.zeros((0, 2), dtype=torch.int64)):
        pl = PairList(empty, 3)
        assert pl.n_pairs == 0 and pl.pairs.shape == (0, 2)
        (a_ptr, a_idx, a_deg), (b_ptr, b_idx, b_deg) = pl.tables()
        assert not a_ptr.any() and a_ptr.shape == (4,) and a_idx.shape == (0,) and a_deg == 0 and b_deg == 0


def test_pairlist_names_the_first_bad_row():
    with pytest.raises(ValueError, match=r"row 2 = \(1, 5\)"):
        PairList([[0, 1], [1, 2], [1, 5], [9, 9]], 5)
    with pytest.raises(ValueError, match=r"row 1 = \(-1, 2\)"):
        PairList([[0, 1], [-1, 2]], 5)
    with pytest.raises(ValueError, match=r"row 0 = \(3, 0\).*\[0, 3\).*\[0, 5\)"):
        PairList([[3, 0]], 5, n_cross=3)  # i runs over the cross sites
    PairList([[2, 4]], 5, n_cross=3)
    with pytest.raises(ValueError, match=r"row 0 = \(2, 4\)"):
        PairList([[2, 4]], 4, n_cross=3)


def test_pairlist_refuses_other_dtypes_and_shapes():
    for bad in (np.array([[0.0, 1.0]]), torch.tensor([[0.0, 1.0]]), np.array([[True, False]]),
                torch.tensor([[True, False]])):
        with pytest.raises(ValueError, match="integers"):
            PairList(bad, 3)
    for bad in (np.zeros((3,), dtype=np.int64), np.zeros((3, 3), dtype=np.int64), np.zeros((2, 2, 2), dtype=np.int64)):
        with pytest.raises(ValueError, match="shape"):
            PairList(bad, 3)
    with pytest.raises(ValueError, match="negative"):
        PairList([], -1)


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_upper_triangle_is_triu_indices_and_is_cached(n):
    pl = PairList.upper_triangle(n)
    i, j = np.triu_indices(n, 1)
    assert np.array_equal(pl.pairs[:, 0], i) and np.array_equal(pl.pairs[:, 1], j)
    assert np.array_equal(pl.pairs.T, torch.triu_indices(n, n, offset=1).numpy())
    assert (pl.n_sites, pl.n_cross, pl.n_pairs) == (n, None, n * (n - 1) // 2)
    assert PairList.upper_triangle(n) is pl


@pytest.mark.parametrize("P,m,n,self_form", [(1, 4, 4, True), (40, 7, 7, True), (257, 9, 9, True), (64, 5, 11, False),
                                             (0, 3, 3, True)])
def test_incidence_tables_match_a_brute_force_build(P, m, n, self_form):
    pairs = random_list(P, m, n, 100 + P, self_form)
    pl = PairList(pairs, n, None if self_form else m)
    if P >= 3:
        assert (pairs[P // 2] == pairs[0]).all() and (not self_form or pairs[-1, 0] == pairs[-1, 1])
    got = pl.tables()
    for (ptr, idx, deg), (rptr, ridx) in zip(got, brute_tables(pairs, m, n)):
        assert ptr.dtype == np.int32 and idx.dtype == np.int32
        assert np.array_equal(ptr, rptr) and np.array_equal(idx, ridx)
        assert deg == (np.diff(rptr).max() if len(rptr) > 1 else 0)
    assert got[0][0][-1] == P and (P == 0 or got[0][0][n] - got[0][0][n - 1] == 0)  # the last site has no pair
    tab = pl.on("cpu")
    assert tab.pairs.dtype == torch.int32 and tuple(tab.pairs.shape) == (P, 2) and (tab.m, tab.n) == (m, n)
    assert np.array_equal(tab.a_ptr.numpy(), got[0][0]) and np.array_equal(tab.b_idx.numpy(), got[1][1])
    assert pl.on("cpu") is tab


# ------------------------------------------------------------------ pair_distances off the kernels
def no_kernel(*a, **k):
    raise AssertionError("a kernel call for an input that stays on torch")


@pytest.fixture
def kernels_off(monkeypatch):
    monkeypatch.setattr(K, "pair_list_dist", no_kernel)
    monkeypatch.setattr(K, "pair_list_pull", no_kernel)


@pytest.mark.parametrize("square", [False, True])
def test_pair_distances_on_cpu_tensors_and_numpy_is_the_plain_expression(kernels_off, square):
    x, c = sites(3, 6, 1), sites(3, 4, 2)
    pairs = random_list(9, 6, 6, 3)
    for given in (pairs, pairs.tolist(), torch.tensor(pairs), PairList(pairs, 6)):
        out = pair_distances(x, given, square=square)
        assert torch.equal(out, plain(x, pairs, square=square)) and out.requires_grad
    from_numpy = pair_distances(x.detach().numpy(), pairs, square=square)
    assert isinstance(from_numpy, torch.Tensor) and torch.equal(from_numpy, plain(x, pairs, square=square).detach())
    cpairs = random_list(7, 4, 6, 4, self_form=False)
    assert torch.equal(pair_distances(x, cpairs, cross_xyz=c, square=square), plain(x, cpairs, c, square))
    mixed = pair_distances(x, PairList(cpairs, 6, 4), c.detach().numpy(), square)  # a tensor and a NumPy array
    assert mixed.requires_grad and torch.equal(mixed.detach(), plain(x, cpairs, c, square).detach())
    half = pair_distances(x.detach().half(), pairs)
    assert half.dtype == torch.float16 and tuple(half.shape) == (3, 9)
    assert tuple(pair_distances(x, []).shape) == (3, 0)


@pytest.mark.parametrize("square", [False, True])
def test_the_triangle_list_gives_distances_upper_triangles(kernels_off, square):
    x = sites(3, 7, 5)
    ref = jaxutil.distances(x, return_matrix=False, square=square)
    assert torch.equal(pair_distances(x, PairList.upper_triangle(7), square=square), ref)
    i, j = torch.triu_indices(7, 7, offset=1)
    assert torch.equal(ref, jaxutil.distances(x, square=square)[:, i, j])


def test_gradients_flow_on_the_cpu(kernels_off):
    x, c = sites(2, 5, 6), sites(2, 3, 7)
    pairs = random_list(6, 3, 5, 8, self_form=False)
    gx, gc = torch.autograd.grad(pair_distances(x, pairs, c).sum(), (x, c))
    rx, rc = torch.autograd.grad(plain(x, pairs, c).sum(), (x, c))
    assert torch.equal(gx, rx) and torch.equal(gc, rc) and gx.abs().sum() > 0 and gc.abs().sum() > 0
    assert torch.autograd.gradcheck(lambda a, b: pair_distances(a, pairs, b), (x, c), eps=1e-6, atol=1e-5, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda a: pair_distances(a, chain(5), square=True), (x,), eps=1e-6, atol=1e-5,
                                    rtol=1e-5)


def test_pair_distances_refuses_lists_and_arrays_that_do_not_fit():
    x, c = sites(3, 6, 9, grad=False), sites(3, 4, 10, grad=False)
    with pytest.raises(ValueError, match="row 0"):
        pair_distances(x, [[0, 6]])
    with pytest.raises(ValueError, match="row 0"):
        pair_distances(x, [[4, 0]], cross_xyz=c)
    with pytest.raises(ValueError, match="pair list for n_sites 5"):
        pair_distances(x, PairList([[0, 1]], 5))
    with pytest.raises(ValueError, match="pair list for n_sites 6, n_cross None"):
        pair_distances(x, PairList([[0, 1]], 6), cross_xyz=c)
    with pytest.raises(ValueError, match="n_cross 4"):
        pair_distances(x, PairList([[0, 1]], 6, 4))
    with pytest.raises(ValueError, match="number of frames"):
        pair_distances(x, [[0, 1]], cross_xyz=c[:2])
    with pytest.raises(ValueError, match="n_steps, n_sites, 3"):
        pair_distances(x[0], [[0, 1]])
    with pytest.raises(ValueError, match="n_steps, n_sites, 3"):
        pair_distances(x[:, :, :2], [[0, 1]])


# ------------------------------------------------------------------ the list Functions over kernels restated in torch
@pytest.fixture
def kernels_in_torch(monkeypatch):
    monkeypatch.setattr(K, "pair_list_dist", fake_pair_list_dist)
    monkeypatch.setattr(K, "pair_list_pull", fake_pair_list_pull)


GC = dict(eps=1e-6, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("square", [False, True])
@pytest.mark.parametrize("self_form", [False, True])
def test_pairlistdist_gradcheck_and_gradgradcheck(kernels_in_torch, square, self_form):
    x, c = sites(2, 5, 11), sites(2, 4, 12)
    if self_form:
        pl = PairList([[0, 1], [1, 2], [0, 4], [3, 2], [0, 1], [4, 1], [2, 0]], 5)  # (a repeat, both orders)
        fn, args = (lambda a: PairListDist.apply(a, a, pl, square)), (x,)
    else:
        pl = PairList(random_list(7, 4, 5, 13, self_form=False), 5, 4)
        fn, args = (lambda a, b: PairListDist.apply(a, b, pl, square)), (x, c)
    assert torch.autograd.gradcheck(fn, args, **GC)
    assert torch.autograd.gradgradcheck(fn, args, **GC)


def test_pairlistpull_and_pairlistdot_gradcheck_and_gradgradcheck(kernels_in_torch):
    x, c, v, y = sites(2, 5, 14), sites(2, 4, 15), sites(2, 5, 16), sites(2, 4, 17)
    pl = PairList(random_list(7, 4, 5, 18, self_form=False), 5, 4)
    w = torch.tensor(np.random.default_rng(19).standard_normal((2, 7)), requires_grad=True)
    for fn, args in ((lambda *a: PairListPull.apply(*a, pl), (w, x, c)), (lambda *a: PairListDot.apply(*a, pl), (v, y, x, c))):
        assert torch.autograd.gradcheck(fn, args, **GC)
        assert torch.autograd.gradgradcheck(fn, args, **GC)


def force_matching(dist, x):
    u = torch.exp(-(dist(x) - 1) ** 2).sum()
    (g,) = torch.autograd.grad(u, x, create_graph=True)
    (gg,) = torch.autograd.grad((g * g).sum(), x)
    return g.detach(), gg


def test_force_matching_double_backward_on_the_triangle_list(kernels_in_torch):
    x = sites(3, 5, 20, grad=False)
    x[:, 3] = x[:, 1]  # two coincident sites: non-finite through plain torch, weight 0 here
    x.requires_grad_(True)
    pl = PairList.upper_triangle(5)
    g, gg = force_matching(lambda z: PairListDist.apply(z, z, pl, False), x)
    assert torch.isfinite(g).all() and torch.isfinite(gg).all()
    _, gg_plain = force_matching(lambda z: plain(z, pl.pairs), x)
    assert not torch.isfinite(gg_plain).all()
    keep = torch.tensor([p for p in range(pl.n_pairs) if tuple(pl.pairs[p]) != (1, 3)])
    g_ref, gg_ref = force_matching(lambda z: plain(z, pl.pairs[keep.numpy()]), x)  # (the zero pair is a constant)
    torch.testing.assert_close(g, g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg, gg_ref, rtol=1e-10, atol=1e-9)


def test_first_order_backward_hands_h_and_d_to_the_kernel_and_skips_unasked_sums(monkeypatch, kernels_in_torch):
    calls = []
    monkeypatch.setattr(K, "pair_list_pull", lambda *a, **k: calls.append((k.get("dv") is not None, k["want_a"], k["want_b"]))
                        or fake_pair_list_pull(*a, **k))
    x, c = sites(2, 5, 21), sites(2, 4, 22, grad=False)
    pl = PairList(random_list(7, 4, 5, 23, self_form=False), 5, 4)
    PairListDist.apply(x, c, pl, False).sum().backward()
    assert calls == [(True, True, False)]  # the quotient form, A only
    calls.clear()
    torch.autograd.grad(PairListDist.apply(x, c, pl, False).sum(), x, create_graph=True)
    assert calls == [(False, True, False)]


@pytest.mark.parametrize("xd,cd", [(torch.float32, torch.float32), (torch.float32, torch.float64),
                                   (torch.float64, torch.float32)])
def test_gradients_come_back_in_their_inputs_dtype(kernels_in_torch, xd, cd):
    x, c = sites(2, 5, 24, xd), sites(2, 4, 25, cd)
    pl = PairList(random_list(7, 4, 5, 26, self_form=False), 5, 4)
    for square in (False, True):
        d = PairListDist.apply(x, c, pl, square)
        assert d.dtype == torch.promote_types(xd, cd)
        gx, gc = torch.autograd.grad((d * d).sum(), (x, c), create_graph=True)
        assert gx.dtype == xd and gc.dtype == cd
        hx, hc = torch.autograd.grad((gx.double() ** 2).sum() + (gc.double() ** 2).sum(), (x, c))
        assert hx.dtype == xd and hc.dtype == cd
