"""The pair-distance Functions of aggforce_amd/_autograd.py (PairDist, PairPull, PairDot) with the two K9 kernels
restated in torch on the CPU: the backward formulas and their closure under differentiation, the zero-distance rule,
the dtype and cost rules, and the routing of jaxutil.distances for inputs that never reach a kernel.  CPU only."""
import numpy as np
import pytest
import torch

import aggforce_amd._kernels as K
import aggforce_amd.jaxutil as jaxutil
from aggforce_amd._autograd import PairDist, PairDot, PairPull

CALLS = []


def _u(x, c):
    return x[:, None, :, :] - c[:, :, None, :]


def fake_pair_dist(x, c, mode=K.PAIR_DIST, v=None, y=None):
    CALLS.append(("dist", mode))
    assert x.dtype == c.dtype and x.is_contiguous() and c.is_contiguous()
    u = _u(x, c)
    if mode == K.PAIR_DOT:
        assert v.dtype == x.dtype == y.dtype
        return (_u(v, y) * u).sum(-1)
    s = (u * u).sum(-1)
    return s if mode == K.PAIR_SQDIST else s.sqrt()


def fake_pair_pull(w, x, c, dv=None, want_a=True, want_b=True, out_dtype=None):
    CALLS.append(("pull", dv is not None, want_a, want_b))
    assert w.dtype == x.dtype == c.dtype and (dv is None or dv.dtype == w.dtype)
    out_dtype = out_dtype or x.dtype
    assert not (x.dtype == torch.float32 and out_dtype == torch.float64)
    if dv is not None:
        w = torch.where(dv > 0, w / dv, torch.zeros_like(w))
    q = w[..., None] * _u(x, c)
    return (q.sum(1).to(out_dtype) if want_a else None), ((-q.sum(2)).to(out_dtype) if want_b else None)


@pytest.fixture(autouse=True)
def kernels_in_torch(monkeypatch):
    monkeypatch.setattr(K, "pair_dist", fake_pair_dist)
    monkeypatch.setattr(K, "pair_pull", fake_pair_pull)
    CALLS.clear()


def sites(T, n, seed, dtype=torch.float64, grad=True):
    """Sites on a 1.5-spaced lattice with 0.3 of noise per frame."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1 / 3)))
    a = np.arange(n)
    lat = 1.5 * np.stack([a % side, (a // side) % side, a // side**2], axis=1)
    return torch.tensor(lat[None] + 0.3 * rng.standard_normal((T, n, 3)), dtype=dtype, requires_grad=grad)


def plain(x, c=None, square=False):
    disp = _u(x, x if c is None else c)
    return (disp**2).sum(-1) if square else torch.linalg.vector_norm(disp, dim=-1)


@pytest.mark.parametrize("square", [False, True])
@pytest.mark.parametrize("self_form", [False, True])
def test_pairdist_gradcheck_and_gradgradcheck(square, self_form):
    x = sites(2, 4, 1)
    c = sites(2, 3, 2)
    fn = (lambda a: PairDist.apply(a, a, square)) if self_form else (lambda a, b: PairDist.apply(a, b, square))
    args = (x,) if self_form else (x, c)
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-5)
    assert torch.autograd.gradgradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-5)


def test_pairpull_and_pairdot_gradcheck_and_gradgradcheck():
    x, c, v, y = sites(2, 4, 3), sites(2, 3, 4), sites(2, 4, 5), sites(2, 3, 6)
    w = torch.tensor(np.random.default_rng(7).standard_normal((2, 3, 4)), requires_grad=True)
    for fn, args in ((lambda *a: PairPull.apply(*a), (w, x, c)), (lambda *a: PairDot.apply(*a), (v, y, x, c))):
        assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-5)
        assert torch.autograd.gradgradcheck(fn, args, eps=1e-6, atol=1e-5, rtol=1e-5)


def test_third_order_chain_matches_plain_torch():
    x, c = sites(3, 5, 8), sites(3, 4, 9)

    def chain(dist):
        u = torch.exp(-(dist(x, c) - 1) ** 2).sum()
        g1 = torch.autograd.grad(u, (x, c), create_graph=True)
        s2 = sum((g**2).sum() for g in g1)
        g2 = torch.autograd.grad(s2, (x, c), create_graph=True)
        s3 = sum((g * torch.sin(g)).sum() for g in g2)
        return g1, g2, torch.autograd.grad(s3, (x, c))

    got = chain(lambda a, b: PairDist.apply(a, b, False))
    ref = chain(lambda a, b: plain(a, b))
    for gs, rs in zip(got, ref):
        for g, r in zip(gs, rs):
            torch.testing.assert_close(g, r, rtol=1e-9, atol=1e-10)


def force_matching(dist, x):
    u = torch.exp(-(dist(x) - 1) ** 2).sum()
    (g,) = torch.autograd.grad(u, x, create_graph=True)
    (gg,) = torch.autograd.grad((g * g).sum(), x)
    return g.detach(), gg


def upper_triangle_reference(x):
    """The same double backward from the off-diagonal pairs only: U = 2 sum_{i<j} f(d_ij) + n T f(0)."""
    n = x.shape[1]
    i0, i1 = torch.triu_indices(n, n, offset=1)

    def dist(z):
        return torch.linalg.vector_norm(z[:, i1] - z[:, i0], dim=-1)

    u = 2 * torch.exp(-(dist(x) - 1) ** 2).sum() + x.shape[0] * n * float(np.exp(-1.0))
    (g,) = torch.autograd.grad(u, x, create_graph=True)
    (gg,) = torch.autograd.grad((g * g).sum(), x)
    return g.detach(), gg


def test_force_matching_double_backward_on_the_self_matrix_is_finite():
    x = sites(3, 5, 10)
    g_plain, gg_plain = force_matching(lambda z: plain(z), x)
    assert torch.isfinite(g_plain).all() and not torch.isfinite(gg_plain).all()  # what the Functions replace
    g, gg = force_matching(lambda z: PairDist.apply(z, z, False), x)
    g_ref, gg_ref = upper_triangle_reference(x)
    assert torch.isfinite(gg).all()
    torch.testing.assert_close(g, g_plain, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(g, g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg, gg_ref, rtol=1e-10, atol=1e-9)


def test_coincident_sites_have_zero_weight_at_every_order():
    x = sites(2, 4, 11, grad=False)
    x[:, 2] = x[:, 0]
    c = torch.cat([x[:, 1:2], sites(2, 2, 12, grad=False)], dim=1)  # c[:, 0] coincides with x[:, 1]
    x.requires_grad_(True)
    c.requires_grad_(True)
    for fn, ref, args in ((lambda a: PairDist.apply(a, a, False), lambda a: plain(a), (x,)),
                          (lambda a, b: PairDist.apply(a, b, False), lambda a, b: plain(a, b), (x, c))):
        g = torch.autograd.grad(torch.exp(-fn(*args)).sum(), args, create_graph=True)
        r = torch.autograd.grad(torch.exp(-ref(*args)).sum(), args)
        for a, b in zip(g, r):
            torch.testing.assert_close(a.detach(), b, rtol=1e-12, atol=1e-12)
        gg = torch.autograd.grad(sum((a * a).sum() for a in g), args)
        assert all(torch.isfinite(a).all() for a in gg)


def test_first_order_backward_hands_h_and_d_to_the_kernel_and_skips_unasked_sums():
    x, c = sites(2, 4, 13), sites(2, 3, 14, grad=False)
    d = PairDist.apply(x, c, False)
    CALLS.clear()
    d.sum().backward()
    assert CALLS == [("pull", True, True, False)]  # Dv form, A only: no W array, no B
    CALLS.clear()
    torch.autograd.grad(PairDist.apply(x, c, False).sum(), x, create_graph=True)
    assert CALLS == [("dist", K.PAIR_DIST), ("pull", False, True, False)]


@pytest.mark.parametrize("xd,cd", [(torch.float32, torch.float32), (torch.float32, torch.float64),
                                   (torch.float64, torch.float32)])
def test_gradients_come_back_in_their_inputs_dtype(xd, cd):
    x, c = sites(2, 4, 15, xd), sites(2, 3, 16, cd)
    for square in (False, True):
        d = PairDist.apply(x, c, square)
        assert d.dtype == torch.promote_types(xd, cd)
        gx, gc = torch.autograd.grad((d * d).sum(), (x, c), create_graph=True)
        assert gx.dtype == xd and gc.dtype == cd
        hx, hc = torch.autograd.grad((gx.double() ** 2).sum() + (gc.double() ** 2).sum(), (x, c))
        assert hx.dtype == xd and hc.dtype == cd


def test_distances_keeps_cpu_numpy_and_displacement_inputs_off_the_kernels(monkeypatch):
    def no_kernel(*a, **k):
        raise AssertionError("a kernel call for an input that stays on torch")

    monkeypatch.setattr(K, "pair_dist", no_kernel)
    monkeypatch.setattr(K, "pair_pull", no_kernel)
    x, c = sites(3, 5, 17), sites(3, 4, 18)
    for kw in ({}, {"square": True}, {"return_matrix": False}):
        torch.testing.assert_close(jaxutil.distances(x, **kw).detach(),
                                   jaxutil.distances(x.detach().numpy(), **kw), rtol=0, atol=0)
    torch.testing.assert_close(jaxutil.distances(x, c), plain(x, c), rtol=0, atol=0)
    assert jaxutil.distances(x, c, return_displacements=True).shape == (3, 4, 5, 3)
    jaxutil.distances(x).sum().backward()
    assert torch.isfinite(x.grad).all()
