"""Differentiable pair distances on the GPU (K9, aggforce_amd/_autograd.py: PairDist / PairPull / PairDot): every
kernel instantiation against a float64 NumPy restatement of the values as stored, gradcheck / gradgradcheck of
jaxutil.distances, the force-matching double backward on the self-distance matrix (non-finite through plain torch),
coincident sites, routing, inputs anywhere in memory, IEEE special values and offsets beyond 2^31.

Sites sit on a 1.5-spaced lattice with 0.3 of seeded noise per frame (bench.py's synthetic recipe), so distances stay
away from zero except where a test wants a zero."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd import _lib  # noqa: E402
from aggforce_amd import jaxutil  # noqa: E402

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
TOL = {F32: 2e-5, F64: 1e-12}  # (the K8 bounds of tests/test_gpu_autograd.py)
SHAPES = [(1, 1, 1), (3, 5, 4), (67, 17, 33), (5, 65, 257), (2, 257, 65), (3, 1, 300), (3, 300, 1)]  # (T, m, n)
SELF_SHAPES = [(T, n) for T, _, n in SHAPES]


def lattice_sites(T, n, seed):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1 / 3)))
    while side**3 < n:
        side += 1
    a = np.arange(n)
    lat = 1.5 * np.stack([a % side, (a // side) % side, a // side**2], axis=1)
    return lat[None] + 0.3 * rng.standard_normal((T, n, 3))


def dev(a, dtype=F64, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV, requires_grad=grad)


def host(t):
    return t.detach().cpu().double().numpy()


def close(got, ref, bound, tol, what=""):
    """|got - ref| <= tol * bound elementwise (bound: the sum of |terms| of each entry, float64)."""
    got = host(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    lim = tol * bound + 1e-300
    worst = float(np.max(err / lim)) if err.size else 0.0
    print(f"{what}: error {worst:.3g} x the {tol:g} bound")
    assert worst <= 1.0, f"{what}: error {worst:.3g} x the {tol:g} bound"


def launched():
    """Demangled names of the kernels launched since the last reset."""
    torch.cuda.synchronize()
    return sorted(p.split("(")[0].replace("void aggf::", "") for p, c in _lib.coverage(names=True).values() if c > 0)


def reset():
    torch.cuda.synchronize()
    _lib.load().aggf_coverage_reset()


def disp(x, c):
    """u[t,i,j] = x[t,j] - c[t,i] in NumPy."""
    return x[:, None, :, :] - c[:, :, None, :]


def plain_distances(xyz, cross_xyz=None, square=False):
    """jaxutil.distances as plain torch ops: the (T, m, n, 3) displacements, then a norm."""
    d = xyz[:, None, :, :] - (xyz if cross_xyz is None else cross_xyz)[:, :, None, :]
    return (d**2).sum(dim=-1) if square else torch.linalg.vector_norm(d, dim=-1)


# ------------------------------------------------------------------ 1. every K9 instantiation vs NumPy float64
def pair_operands(T, m, n, dtype, self_form):
    seed = 1000 * T + 10 * m + n
    x = dev(lattice_sites(T, n, seed), dtype)
    c = x if self_form else dev(lattice_sites(T, m, seed + 1) + 0.4, dtype)
    rng = np.random.default_rng(seed + 2)
    v = dev(rng.standard_normal((T, n, 3)), dtype)
    y = dev(rng.standard_normal((T, m, 3)), dtype)
    w = dev(rng.standard_normal((T, m, n)), dtype)
    return x, c, v, y, w


def pull_reference(w, u):
    q = w[..., None] * u
    bound = np.abs(w)[..., None] * np.abs(u)
    return q.sum(1), -q.sum(2), bound.sum(1), bound.sum(2)


# (3, 9, 200): one panel of float32 columns, two of float64
ALL_SHAPES = [(s, False) for s in SHAPES + [(3, 9, 200)]] + [((T, n, n), True) for T, n in SELF_SHAPES]


@pytest.mark.parametrize("shape,self_form", ALL_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("self" if v else "cross"))
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_k9a_every_mode_matches_numpy(shape, self_form, dtype):
    T, m, n = shape
    x, c, v, y, _ = pair_operands(T, m, n, dtype, self_form)
    u, g = disp(host(x), host(c)), disp(host(v), host(y))
    sq = (u * u).sum(-1)
    reset()
    d = K.pair_dist(x, c, K.PAIR_DIST)
    s = K.pair_dist(x, c, K.PAIR_SQDIST)
    o = K.pair_dist(x, c, K.PAIR_DOT, v, y)
    k = "float" if dtype == F32 else "double"
    assert launched() == [f"pairdist_kernel<{k}, {mode}>" for mode in (0, 1, 2)]
    for got in (d, s, o):
        assert got.dtype == dtype and tuple(got.shape) == (T, m, n)
    close(d, np.sqrt(sq), np.sqrt(sq), TOL[dtype], "K9a DIST")
    close(s, sq, sq, TOL[dtype], "K9a SQDIST")
    close(o, (g * u).sum(-1), (np.abs(g) * np.abs(u)).sum(-1), TOL[dtype], "K9a DOT")
    if self_form:
        idx = torch.arange(n, device=DEV)
        assert (d[:, idx, idx] == 0).all() and (s[:, idx, idx] == 0).all()


@pytest.mark.parametrize("shape,self_form", ALL_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("self" if v else "cross"))
@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32)], ids=["f32", "f64", "f64-f32"])
def test_k9b_both_sums_match_numpy_and_repeat_bit_for_bit(shape, self_form, ind, outd):
    T, m, n = shape
    x, c, _, _, w = pair_operands(T, m, n, ind, self_form)
    u = disp(host(x), host(c))
    tol = max(TOL[ind], TOL[outd])
    k = {F32: "float", F64: "double"}
    panels = n > (256 if ind == F32 else 128)  # more than one 1 KiB panel of columns: B goes through partial sums
    # the weights as given
    a_ref, b_ref, a_bnd, b_bnd = pull_reference(host(w), u)
    reset()
    a, b = K.pair_pull(w, x, c, out_dtype=outd)
    names = [f"pairpull_kernel<{k[ind]}, {k[outd]}, false>"] + ([f"pairpull_reduce_kernel<{k[outd]}>"] if panels else [])
    assert launched() == names
    assert a.dtype == outd and b.dtype == outd and tuple(a.shape) == (T, n, 3) and tuple(b.shape) == (T, m, 3)
    close(a, a_ref, a_bnd, tol, "K9b A")
    close(b, b_ref, b_bnd, tol, "K9b B")
    a2, b2 = K.pair_pull(w, x, c, out_dtype=outd)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    # either output alone: the same bits, and no partial-sum pass without B
    reset()
    a1, none = K.pair_pull(w, x, c, want_b=False, out_dtype=outd)
    assert none is None and torch.equal(a1, a) and launched() == names[:1]
    none, b1 = K.pair_pull(w, x, c, want_a=False, out_dtype=outd)
    assert none is None and torch.equal(b1, b)
    # the distance form: w / dv where dv > 0, else 0 (the self form's diagonal is zero)
    dv = K.pair_dist(x, c, K.PAIR_DIST)
    dvn = host(dv)
    assert self_form == bool((dvn == 0).any())
    wn = np.where(dvn > 0, host(w) / np.where(dvn > 0, dvn, 1.0), 0.0)
    a_ref, b_ref, a_bnd, b_bnd = pull_reference(wn, u)
    reset()
    a, b = K.pair_pull(w, x, c, dv=dv, out_dtype=outd)
    assert launched()[0] == f"pairpull_kernel<{k[ind]}, {k[outd]}, true>"
    close(a, a_ref, a_bnd, tol, "K9b A (Dv)")
    close(b, b_ref, b_bnd, tol, "K9b B (Dv)")
    a2, b2 = K.pair_pull(w, x, c, dv=dv, out_dtype=outd)
    assert torch.equal(a, a2) and torch.equal(b, b2)
    a1, _ = K.pair_pull(w, x, c, dv=dv, want_b=False, out_dtype=outd)
    _, b1 = K.pair_pull(w, x, c, dv=dv, want_a=False, out_dtype=outd)
    assert torch.equal(a1, a) and torch.equal(b1, b)


def test_k9_wrappers_refuse_mixed_operands_and_return_empty_shapes_without_a_launch():
    x, c = dev(lattice_sites(3, 4, 1), F32), dev(lattice_sites(3, 5, 2), F64)
    with pytest.raises(ValueError):
        K.pair_dist(x, c)
    with pytest.raises(ValueError):
        K.pair_pull(torch.zeros((3, 5, 4), dtype=F32, device=DEV), x, x.clone())
    with pytest.raises(ValueError):
        K.pair_pull(torch.zeros((3, 4, 4), dtype=F32, device=DEV), x, x, out_dtype=F64)
    reset()
    e = torch.empty((3, 0, 3), dtype=F32, device=DEV)
    assert tuple(K.pair_dist(x, e).shape) == (3, 0, 4) and tuple(K.pair_dist(e, x).shape) == (3, 4, 0)
    a, b = K.pair_pull(torch.empty((3, 0, 4), dtype=F32, device=DEV), x, e)
    assert tuple(a.shape) == (3, 4, 3) and not a.any() and tuple(b.shape) == (3, 0, 3)
    assert tuple(jaxutil.distances(x[:0]).shape) == (0, 4, 4)
    assert launched() == []


# ------------------------------------------------------------------ 2. gradcheck / gradgradcheck (float64)
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("T,m,n", SHAPES)
@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
def test_cross_distances_gradcheck_and_gradgradcheck(T, m, n, square):
    x = dev(lattice_sites(T, n, 3 * T + n), grad=True)
    c = dev(lattice_sites(T, m, 5 * T + m) + 0.4, grad=True)
    fast = x.numel() + c.numel() > 400

    def fn(a, b):
        return jaxutil.distances(a, b, square=square)

    assert torch.autograd.gradcheck(fn, (x, c), fast_mode=fast, **GC)
    assert torch.autograd.gradgradcheck(fn, (x, c), fast_mode=fast, **GC)


@pytest.mark.parametrize("T,n", SELF_SHAPES)
@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
@pytest.mark.parametrize("matrix", [True, False], ids=["matrix", "triu"])
def test_self_distances_gradcheck_and_gradgradcheck(T, n, square, matrix):
    x = dev(lattice_sites(T, n, 7 * T + n), grad=True)
    fast = x.numel() > 400

    def fn(a):
        return jaxutil.distances(a, square=square, return_matrix=matrix)

    assert tuple(fn(x).shape) == ((T, n, n) if matrix else (T, n * (n - 1) // 2))
    if n == 1 and not matrix:
        return  # (no pair: the result is empty)
    assert torch.autograd.gradcheck(fn, (x,), fast_mode=fast, **GC)
    assert torch.autograd.gradgradcheck(fn, (x,), fast_mode=fast, **GC)


def test_third_order_chain_matches_plain_torch():
    xn, cn = lattice_sites(3, 5, 21), lattice_sites(3, 4, 22) + 0.4

    def chain(dist, device):
        x = torch.tensor(xn, device=device, requires_grad=True)
        c = torch.tensor(cn, device=device, requires_grad=True)
        u = torch.exp(-(dist(x, c) - 1) ** 2).sum()
        g1 = torch.autograd.grad(u, (x, c), create_graph=True)
        g2 = torch.autograd.grad(sum((g**2).sum() for g in g1), (x, c), create_graph=True)
        g3 = torch.autograd.grad(sum((g * torch.sin(g)).sum() for g in g2), (x, c))
        return [g.detach().cpu() for g in (*g1, *g2, *g3)]

    reset()
    got = chain(jaxutil.distances, DEV)
    assert any("pairdist_kernel<double, 2>" in k for k in launched())  # PairDot ran
    ref = chain(plain_distances, "cpu")
    for g, r in zip(got, ref):
        torch.testing.assert_close(g, r, rtol=1e-10, atol=1e-9)


# ------------------------------------------------------------------ 3. force-matching double backward, self matrix
def force_matching(dist, x):
    u = torch.exp(-(dist(x) - 1) ** 2).sum()
    (g,) = torch.autograd.grad(u, x, create_graph=True)
    (gg,) = torch.autograd.grad((g * g).sum(), x)
    return g.detach(), gg


def upper_triangle_force_matching(xn):
    """The same two quantities in float64 on the CPU from the pairs i < j only: U = 2 sum_{i<j} f(d_ij) + T n f(0)."""
    x = torch.tensor(xn, requires_grad=True)
    T, n, _ = x.shape
    i0, i1 = torch.triu_indices(n, n, offset=1)
    d = torch.linalg.vector_norm(x[:, i1] - x[:, i0], dim=-1)
    u = 2 * torch.exp(-(d - 1) ** 2).sum() + T * n * float(np.exp(-1.0))
    (g,) = torch.autograd.grad(u, x, create_graph=True)
    (gg,) = torch.autograd.grad((g * g).sum(), x)
    return g.detach(), gg


@pytest.mark.parametrize("T,n", [(3, 5), (20, 65)])
def test_force_matching_double_backward_on_the_self_matrix(T, n):
    xn = lattice_sites(T, n, 31 + n)
    g, gg = force_matching(jaxutil.distances, dev(xn, grad=True))
    assert torch.isfinite(gg).all(), "non-finite double backward"
    g_ref, gg_ref = upper_triangle_force_matching(xn)
    torch.testing.assert_close(gg.cpu(), gg_ref, rtol=1e-10, atol=1e-9)
    g_plain, _ = force_matching(plain_distances, dev(xn, grad=True))
    torch.testing.assert_close(g, g_plain, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(g.cpu(), g_ref, rtol=1e-10, atol=1e-9)


# ------------------------------------------------------------------ 4. coincident sites
@pytest.mark.parametrize("self_form", [False, True], ids=["cross", "self"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_coincident_sites_have_finite_gradients(self_form, dtype):
    xn = lattice_sites(4, 9, 41)
    xn[:, 6] = xn[:, 2]
    cn = lattice_sites(4, 7, 42) + 0.4
    cn[:, 3] = xn[:, 5]
    x, c = dev(xn, dtype, grad=True), dev(cn, dtype, grad=True)
    args = (x,) if self_form else (x, c)
    assert (jaxutil.distances(*args) == 0).sum() == (4 * (9 + 2) if self_form else 4)
    g = torch.autograd.grad(torch.exp(-jaxutil.distances(*args)).sum(), args, create_graph=True)
    r = torch.autograd.grad(torch.exp(-plain_distances(*args)).sum(), args)
    for a, b in zip(g, r):
        assert torch.isfinite(a).all()
        # (a gradient sums at most 9 terms of size <= 1: a few units of the dtype's rounding)
        torch.testing.assert_close(a.detach(), b, rtol=0, atol=TOL[dtype])
    gg = torch.autograd.grad(sum((a * a).sum() for a in g), args)
    assert all(torch.isfinite(a).all() for a in gg)


# ------------------------------------------------------------------ 5. routing
def test_gpu_tensors_run_on_k9_and_an_unasked_gradient_costs_nothing(monkeypatch):
    x = dev(lattice_sites(3, 300, 51), F32, grad=True)
    c = dev(lattice_sites(3, 2, 52) + 0.4, F32)
    reset()
    d = jaxutil.distances(x, c)
    d.sum().backward()
    assert launched() == ["pairdist_kernel<float, 0>", "pairpull_kernel<float, float, true>"]  # no B: no partial sums
    assert x.grad.dtype == F32 and c.grad is None
    calls = []
    real = K.pair_pull
    monkeypatch.setattr(K, "pair_pull", lambda *a, **k: calls.append((k, real(*a, **k))) or calls[-1][1])
    c.requires_grad_(True)
    reset()
    jaxutil.distances(x).sum().backward()                      # self: both sums, one call
    jaxutil.distances(x, c.detach(), square=True).sum().backward()  # x alone
    jaxutil.distances(x.detach(), c).sum().backward()          # cross_xyz alone
    jaxutil.distances(x, c.double()).sum().backward()          # promoted
    assert [(k["want_a"], k["want_b"], a is None, b is None) for k, (a, b) in calls] == [
        (True, True, False, False), (True, False, False, True), (False, True, True, False), (True, True, False, False)]
    assert "pairpull_reduce_kernel<float>" in launched() and "pairdist_kernel<double, 0>" in launched()
    assert x.grad.dtype == F32 and c.grad.dtype == F32
    assert jaxutil.distances(x, c.double()).dtype == F64


def test_cpu_numpy_and_displacement_inputs_launch_nothing():
    xn, cn = lattice_sites(3, 5, 53), lattice_sites(3, 4, 54)
    x, c = torch.tensor(xn, requires_grad=True), torch.tensor(cn)
    xg = dev(xn, grad=True)
    reset()
    out = jaxutil.distances(x, c)
    assert out.device.type == "cpu" and torch.equal(out, plain_distances(x, c))
    out.sum().backward()
    i0, i1 = np.triu_indices(5, k=1)
    assert torch.equal(jaxutil.distances(x, return_matrix=False, square=True), plain_distances(x, square=True)[:, i0, i1])
    from_numpy = jaxutil.distances(xn, cn)
    assert from_numpy.device.type == "cpu" and torch.equal(from_numpy, out.detach())
    d4 = jaxutil.distances(xg, dev(cn), return_displacements=True)
    assert d4.is_cuda and tuple(d4.shape) == (3, 4, 5, 3) and d4.requires_grad
    assert torch.equal(d4.detach().cpu(), torch.tensor(disp(xn, cn)))
    half = jaxutil.distances(xg.detach().half())
    assert half.dtype == torch.float16
    assert launched() == []
    with pytest.raises(ValueError, match="Cross distances"):
        jaxutil.distances(xg, xg, return_matrix=False)
    with pytest.raises(ValueError, match="Displacements"):
        jaxutil.distances(xg, return_matrix=False, return_displacements=True)


# ------------------------------------------------------------------ 6. layouts and special values
PAD = 64


def placed(arr, k):
    """Device copy of `arr` that starts k elements into a larger allocation whose rest is NaN."""
    buf = torch.full((k + arr.numel() + PAD,), float("nan"), dtype=arr.dtype, device=DEV)
    view = buf[k:k + arr.numel()].view(arr.shape)
    view.copy_(arr)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def bits(t):
    return t.detach().view(torch.int32 if t.dtype == F32 else torch.int64)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_operands_at_element_offsets_give_the_aligned_results(dtype, k):
    if dtype == F64 and k == 2:
        k = 5  # (two float64 elements are 16 bytes)
    T, m, n = 5, 65, 257
    x, c, v, y, w = pair_operands(T, m, n, dtype, False)
    dv = K.pair_dist(x, c)
    px, pc, pv, py, pw, pdv = (placed(t, k) for t in (x, c, v, y, w, dv))
    for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
        assert torch.equal(K.pair_dist(px, pc, mode, pv, py), K.pair_dist(x, c, mode, v, y))
    for kw, pkw in (({}, {}), ({"dv": dv}, {"dv": pdv})):
        a, b = K.pair_pull(w, x, c, **kw)
        pa, pb = K.pair_pull(pw, px, pc, **pkw)
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert torch.equal(pa, a) and torch.equal(pb, b)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_non_contiguous_inputs(dtype):
    big = dev(lattice_sites(6, 66, 61), dtype)
    x = big[::2, 1::2]           # (3, 33, 3), strided in frames and sites
    c = big[1::2, :12:2]         # (3, 6, 3)
    assert not x.is_contiguous() and not c.is_contiguous()
    xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    xs, cs = x.detach().requires_grad_(True), c.detach().requires_grad_(True)
    d = jaxutil.distances(xs, cs)
    dr = jaxutil.distances(xr.contiguous(), cr.contiguous())
    assert torch.equal(d, dr)
    h = dev(np.random.default_rng(62).standard_normal(tuple(d.shape)), dtype)
    got = torch.autograd.grad(d, (xs, cs), h.transpose(1, 2).contiguous().transpose(1, 2))  # a strided upstream gradient
    ref = torch.autograd.grad(dr, (xr, cr), h)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_nan_and_infinite_coordinates_propagate_as_numpys_do(dtype):
    T, m, n = 3, 17, 70
    x, c, v, y, w = pair_operands(T, m, n, dtype, False)
    x, c = x.clone(), c.clone()
    x[0, 3, 1] = float("nan")
    x[1, 64, 0] = float("inf")
    x[1, 69, 2] = float("-inf")
    c[1, 4, 0] = float("inf")
    c[2, 16, 2] = float("nan")
    c[0, 0, 1] = float("-inf")
    nd = np.float32 if dtype == F32 else np.float64
    xn, cn, vn, yn, wn = (t.cpu().numpy().astype(nd) for t in (x, c, v, y, w))
    rt = dict(rtol=TOL[dtype], atol=0, equal_nan=True)
    with np.errstate(all="ignore"):
        u = disp(xn, cn)
        sq = (u * u).sum(-1)
        np.testing.assert_allclose(K.pair_dist(x, c, K.PAIR_SQDIST).cpu().numpy(), sq, **rt)
        np.testing.assert_allclose(K.pair_dist(x, c, K.PAIR_DIST).cpu().numpy(), np.sqrt(sq), **rt)
        dot = K.pair_dist(x, c, K.PAIR_DOT, v, y).cpu().numpy()
        ref = (disp(vn, yn).astype(np.float64) * u).sum(-1)
        assert np.array_equal(np.isnan(dot), np.isnan(ref)) and np.array_equal(np.isinf(dot), np.isinf(ref))
        assert np.array_equal(np.sign(dot[np.isinf(dot)]), np.sign(ref[np.isinf(ref)]))
        a, b = K.pair_pull(w, x, c)
        q = wn.astype(np.float64)[..., None] * u
        for got, full in ((a.cpu().numpy(), q.sum(1)), (b.cpu().numpy(), -q.sum(2))):
            assert np.isnan(full).any() and np.isinf(full).any() and np.isfinite(full).any()
            assert np.array_equal(np.isnan(got), np.isnan(full)) and np.array_equal(np.isinf(got), np.isinf(full))
            assert np.array_equal(np.sign(got[np.isinf(got)]), np.sign(full[np.isinf(full)]))
        # the distance form gives weight 0 where the distance is NaN (NaN > 0 is false), as torch.where does
        dv = K.pair_dist(x, c, K.PAIR_DIST)
        a, b = K.pair_pull(w, x, c, dv=dv)
        dvn = dv.cpu().numpy().astype(np.float64)
        wd = np.where(dvn > 0, wn / np.where(dvn > 0, dvn, 1.0), 0.0)
        q = wd[..., None] * u
        for got, full in ((a.cpu().numpy(), q.sum(1)), (b.cpu().numpy(), -q.sum(2))):
            assert np.array_equal(np.isnan(got), np.isnan(full)) and np.array_equal(np.isinf(got), np.isinf(full))


# ------------------------------------------------------------------ 7. element offsets beyond 2^31
def test_forward_beyond_two_to_the_31_elements():
    T, m, n = 33, 8200, 8200
    assert T * m * n > 2**31
    rng = np.random.default_rng(71)
    x = dev(30 * rng.standard_normal((T, n, 3)), F32)
    c = dev(30 * rng.standard_normal((T, m, 3)), F32)
    d = jaxutil.distances(x, c)
    assert tuple(d.shape) == (T, m, n) and d.dtype == F32
    xn, cn = host(x), host(c)

    def frame(t, rows):
        return np.sqrt(sum((xn[t, None, :, k] - cn[t, rows, None, k]) ** 2 for k in range(3)))

    try:
        ref = frame(T - 1, slice(None))
        close(d[T - 1], ref, ref, TOL[F32], "last frame")
        del ref
        # some rows of the frames in which the byte offset passes 2^31, 2^32 and 2^33 (the element offset 2^31)
        rows = slice(0, m, 41)
        for t in (7, 15, 31):
            assert t * m * n * 4 < 2 ** (31 + (7, 15, 31).index(t)) < (t + 1) * m * n * 4
            ref = frame(t, rows)
            close(d[t, rows], ref, ref, TOL[F32], f"frame {t}")
    finally:
        del d
        torch.cuda.empty_cache()
