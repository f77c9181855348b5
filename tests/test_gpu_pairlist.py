"""Pair-list distances on the GPU (K9c / K9d, aggforce_amd/_autograd.py: PairListDist / PairListPull / PairListDot;
jaxutil.pair_distances and the upper triangles of jaxutil.distances): every kernel instantiation against a float64
NumPy restatement of the values as stored, both forms of the pull kernel, empty lists, bit-for-bit repeats, the forward
against the gather from the distance matrix it replaces, gradcheck / gradgradcheck, the force-matching double backward,
peak memory against the matrix route, inputs anywhere in memory, NaN coordinates and offsets beyond 2^31.

List kinds: the triangle (i < j), a chain (i, i + 1), a star (site 0 with every other site) and random lists with
repeats, pairs i == j and a site in no pair (tests/pairlist_ref.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd import _lib  # noqa: E402
from aggforce_amd import jaxutil  # noqa: E402
from aggforce_amd._autograd import PairDist  # noqa: E402
from aggforce_amd.jaxutil import PairList, pair_distances  # noqa: E402
from conftest import need_hbm  # noqa: E402
from pairlist_ref import chain, lattice_sites, list_disp, pull_reference, random_list, star, triangle  # noqa: E402

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
TOL = {F32: 2e-5, F64: 1e-12}  # (the K9 bounds of tests/test_gpu_distances.py)
NAME = {F32: "float", F64: "double"}
LANE_DEG = 32  # csrc/aggf_pairlist.hip PLP_LANE_DEG: a table whose longest run is beyond it takes the wave form
FRAMES = (1, 3, 67)


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


# ------------------------------------------------------------------ 1. every K9c / K9d instantiation vs NumPy float64
# (name, pairs, m or None for the self form, n)
CASES = ([(f"triangle{n}", triangle(n), None, n) for n in (2, 5, 65, 130)]
         + [(f"chain{n}", chain(n), None, n) for n in (2, 5, 65, 130)]
         + [(f"star{n}", star(n), None, n) for n in (130, 300)]          # degrees beyond 64 and 256
         + [(f"random{P}", random_list(P, 9, 9, 200 + P), None, 9) for P in (1, 63, 64, 65, 257)]
         + [("cross", random_list(70, 6, 11, 300, self_form=False), 6, 11)])
CASE_IDS = [c[0] for c in CASES]


def list_operands(T, pairs, m, n, dtype):
    seed = 1000 * T + 10 * len(pairs) + n
    x = dev(lattice_sites(T, n, seed), dtype)
    c = x if m is None else dev(lattice_sites(T, m, seed + 1) + 0.4, dtype)
    rng = np.random.default_rng(seed + 2)
    v = dev(rng.standard_normal((T, n, 3)), dtype)
    y = v if m is None else dev(rng.standard_normal((T, m, 3)), dtype)
    w = dev(rng.standard_normal((T, len(pairs))), dtype)
    return x, c, v, y, w


def pull_names(pl, ind, outd, dv):
    forms = {int(deg > LANE_DEG) for _, _, deg in pl.tables()}
    return sorted(f"pairlist_pull_kernel<{NAME[ind]}, {NAME[outd]}, {'true' if dv else 'false'}, {f}>" for f in forms)


def test_the_cases_reach_both_forms_of_the_pull_kernel():
    degs = {name: [deg for _, _, deg in PairList(pairs, n, m).tables()] for name, pairs, m, n in CASES}
    assert max(degs["chain130"]) <= 2 and degs["star300"] == [1, 299] and min(degs["triangle130"]) == 129
    assert max(degs["triangle5"]) <= LANE_DEG < min(degs["triangle65"])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_k9c_every_mode_matches_numpy(case, dtype):
    _, pairs, m, n = case
    pl = PairList(pairs, n, m)
    for T in FRAMES:
        x, c, v, y, _ = list_operands(T, pairs, m, n, dtype)
        u, g = list_disp(host(x), host(c), pairs), list_disp(host(v), host(y), pairs)
        sq = (u * u).sum(-1)
        reset()
        d = K.pair_list_dist(x, c, pl.on(DEV), K.PAIR_DIST)
        s = K.pair_list_dist(x, c, pl.on(DEV), K.PAIR_SQDIST)
        o = K.pair_list_dist(x, c, pl.on(DEV), K.PAIR_DOT, v, y)
        assert launched() == [f"pairlist_kernel<{NAME[dtype]}, {mode}>" for mode in (0, 1, 2)]
        for got in (d, s, o):
            assert got.dtype == dtype and tuple(got.shape) == (T, len(pairs))
        close(d, np.sqrt(sq), np.sqrt(sq), TOL[dtype], "K9c DIST")
        close(s, sq, sq, TOL[dtype], "K9c SQDIST")
        close(o, (g * u).sum(-1), (np.abs(g) * np.abs(u)).sum(-1), TOL[dtype], "K9c DOT")
        same = pairs[:, 0] == pairs[:, 1]
        if m is None and same.any():
            assert (d[:, torch.tensor(same, device=DEV)] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32)], ids=["f32", "f64", "f64-f32"])
def test_k9d_both_sums_match_numpy_and_repeat_bit_for_bit(case, ind, outd):
    _, pairs, m, n = case
    pl = PairList(pairs, n, m)
    tab = pl.on(DEV)
    rows = n if m is None else m
    tol = max(TOL[ind], TOL[outd])
    for T in FRAMES:
        x, c, _, _, w = list_operands(T, pairs, m, n, ind)
        u = list_disp(host(x), host(c), pairs)
        # the weights as given
        a_ref, b_ref, a_bnd, b_bnd = pull_reference(host(w), u, pairs, rows, n)
        reset()
        a, b = K.pair_list_pull(w, x, c, tab, out_dtype=outd)
        assert launched() == pull_names(pl, ind, outd, False)
        assert a.dtype == outd and b.dtype == outd and tuple(a.shape) == (T, n, 3) and tuple(b.shape) == (T, rows, 3)
        close(a, a_ref, a_bnd, tol, "K9d A")
        close(b, b_ref, b_bnd, tol, "K9d B")
        assert not a[:, n - 1].any() or (pairs[:, 1] == n - 1).any()  # a site in no pair: zeros
        a2, b2 = K.pair_list_pull(w, x, c, tab, out_dtype=outd)
        assert torch.equal(a, a2) and torch.equal(b, b2)
        # either output alone: the same bits
        a1, none = K.pair_list_pull(w, x, c, tab, want_b=False, out_dtype=outd)
        assert none is None and torch.equal(a1, a)
        none, b1 = K.pair_list_pull(w, x, c, tab, want_a=False, out_dtype=outd)
        assert none is None and torch.equal(b1, b)
        # the distance form: w / dv where dv > 0, else 0 (a pair i == i has distance zero)
        dv = K.pair_list_dist(x, c, tab, K.PAIR_DIST)
        dvn = host(dv)
        wn = np.where(dvn > 0, host(w) / np.where(dvn > 0, dvn, 1.0), 0.0)
        a_ref, b_ref, a_bnd, b_bnd = pull_reference(wn, u, pairs, rows, n)
        reset()
        a, b = K.pair_list_pull(w, x, c, tab, dv=dv, out_dtype=outd)
        assert launched() == pull_names(pl, ind, outd, True)
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        close(a, a_ref, a_bnd, tol, "K9d A (Dv)")
        close(b, b_ref, b_bnd, tol, "K9d B (Dv)")
        a2, b2 = K.pair_list_pull(w, x, c, tab, dv=dv, out_dtype=outd)
        assert torch.equal(a, a2) and torch.equal(b, b2)
        a1, _ = K.pair_list_pull(w, x, c, tab, dv=dv, want_b=False, out_dtype=outd)
        _, b1 = K.pair_list_pull(w, x, c, tab, dv=dv, want_a=False, out_dtype=outd)
        assert torch.equal(a1, a) and torch.equal(b1, b)


# ------------------------------------------------------------------ 2. empty problems; 3. repeats
def test_empty_lists_and_no_frames_launch_nothing():
    x = dev(lattice_sites(3, 4, 1), F32)
    empty, some = PairList([], 4), PairList([[0, 1], [2, 3]], 4)
    with pytest.raises(ValueError):
        K.pair_list_dist(x, x.double(), some.on(DEV))
    with pytest.raises(ValueError):
        K.pair_list_pull(torch.zeros((3, 3), dtype=F32, device=DEV), x, x, some.on(DEV))
    with pytest.raises(ValueError):
        K.pair_list_pull(torch.zeros((3, 2), dtype=F32, device=DEV), x, x, some.on(DEV), out_dtype=F64)
    with pytest.raises(ValueError):
        K.pair_list_dist(x[:, :3].contiguous(), x[:, :3].contiguous(), some.on(DEV))  # a list for other sites
    reset()
    assert tuple(K.pair_list_dist(x, x, empty.on(DEV)).shape) == (3, 0)
    a, b = K.pair_list_pull(torch.empty((3, 0), dtype=F32, device=DEV), x, x, empty.on(DEV))
    assert tuple(a.shape) == (3, 4, 3) and tuple(b.shape) == (3, 4, 3) and not a.any() and not b.any()
    assert tuple(K.pair_list_dist(x[:0], x[:0], some.on(DEV)).shape) == (0, 2)
    a, b = K.pair_list_pull(torch.empty((0, 2), dtype=F32, device=DEV), x[:0], x[:0], some.on(DEV))
    assert tuple(a.shape) == (0, 4, 3) and tuple(b.shape) == (0, 4, 3)
    xg = x.clone().requires_grad_(True)
    out = pair_distances(xg, [])
    assert tuple(out.shape) == (3, 0) and out.is_cuda
    out.sum().backward()
    assert tuple(xg.grad.shape) == (3, 4, 3) and not xg.grad.any()
    assert tuple(pair_distances(x[:0], some).shape) == (0, 2)
    assert tuple(jaxutil.distances(x[:, :1], return_matrix=False).shape) == (3, 0)
    assert launched() == []


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_two_identical_pull_calls_are_bit_identical(dtype):
    for pairs, n in ((triangle(130), 130), (chain(130), 130)):  # the wave form and the lane form, many blocks
        tab = PairList(pairs, n).on(DEV)
        x, c, _, _, w = list_operands(67, pairs, None, n, dtype)
        dv = K.pair_list_dist(x, c, tab)
        for kw in ({}, {"dv": dv}):
            a, b = K.pair_list_pull(w, x, c, tab, **kw)
            a2, b2 = K.pair_list_pull(w, x, c, tab, **kw)
            assert torch.equal(a, a2) and torch.equal(b, b2)


# ------------------------------------------------------------------ 4. the forward of the triangle route does not move
def _upper_triangles(dist):
    n = dist.shape[-1]
    i0, i1 = torch.triu_indices(n, n, offset=1, device=dist.device)
    return dist[:, i0, i1]


def matrix_route(x, square=False):
    """distances(x, return_matrix=False) before the pair-list kernels: the (T, n, n) matrix, then a gather."""
    return _upper_triangles(PairDist.apply(x, x, square))


@pytest.mark.parametrize("T,n", [(3, 5), (67, 33), (5, 257)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
def test_upper_triangles_equal_the_gather_from_the_matrix_bit_for_bit(T, n, dtype, square):
    x = dev(lattice_sites(T, n, 400 + n), dtype)
    got = jaxutil.distances(x, return_matrix=False, square=square)
    assert tuple(got.shape) == (T, n * (n - 1) // 2)
    assert torch.equal(got, matrix_route(x, square))


# ------------------------------------------------------------------ 5. gradcheck / gradgradcheck (float64)
GC = dict(eps=1e-6, atol=1e-5, rtol=1e-5)
SELF7 = [[0, 1], [1, 2], [0, 4], [3, 2], [4, 1], [2, 0], [3, 4]]


@pytest.mark.parametrize("pairs", [SELF7, SELF7[:6] + [[0, 1]], SELF7[:6] + [[3, 3]]], ids=["plain", "repeat", "self-pair"])
@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
def test_self_lists_gradcheck_and_gradgradcheck(pairs, square):
    x = dev(lattice_sites(2, 5, 501), grad=True)
    pl = PairList(pairs, 5)

    def fn(a):
        return pair_distances(a, pl, square=square)

    reset()
    assert torch.autograd.gradcheck(fn, (x,), **GC)
    assert torch.autograd.gradgradcheck(fn, (x,), **GC)
    assert any(k.startswith("pairlist_pull_kernel<double") for k in launched())


@pytest.mark.parametrize("square", [False, True], ids=["dist", "square"])
def test_cross_lists_gradcheck_and_gradgradcheck(square):
    x = dev(lattice_sites(2, 5, 502), grad=True)
    c = dev(lattice_sites(2, 4, 503) + 0.4, grad=True)
    pairs = [[0, 1], [3, 2], [0, 4], [3, 2], [1, 1], [2, 0], [3, 4]]

    def fn(a, b):
        return pair_distances(a, pairs, cross_xyz=b, square=square)

    assert torch.autograd.gradcheck(fn, (x, c), **GC)
    assert torch.autograd.gradgradcheck(fn, (x, c), **GC)


# ------------------------------------------------------------------ 6. force-matching double backward, triangle route
def force_matching(dist, x):
    u = torch.exp(-(dist(x) - 1) ** 2).sum()
    (g,) = torch.autograd.grad(u, x, create_graph=True)
    (gg,) = torch.autograd.grad((g * g).sum(), x)
    return g.detach(), gg


def cpu_force_matching(xn, skip=()):
    """The same two quantities in float64 on the CPU from the pairs i < j (``skip``: pairs at distance zero, whose
    term exp(-1) is a constant)."""
    x = torch.tensor(xn, requires_grad=True)
    n = x.shape[1]
    i0, i1 = (torch.tensor(a) for a in zip(*[(i, j) for i in range(n) for j in range(i + 1, n) if (i, j) not in skip]))
    return force_matching(lambda z: torch.linalg.vector_norm(z[:, i1] - z[:, i0], dim=-1), x)


@pytest.mark.parametrize("T,n", [(3, 5), (5, 65)])
def test_force_matching_double_backward_on_the_triangle_route(T, n):
    xn = lattice_sites(T, n, 600 + n)
    reset()
    g, gg = force_matching(lambda z: jaxutil.distances(z, return_matrix=False), dev(xn, grad=True))
    names = launched()
    assert "pairlist_kernel<double, 2>" in names  # PairListDot ran
    assert not any(k.startswith(("pairdist_kernel", "pairpull_kernel")) for k in names)
    assert torch.isfinite(gg).all(), "non-finite double backward"
    g_ref, gg_ref = cpu_force_matching(xn)
    torch.testing.assert_close(g.cpu(), g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg.cpu(), gg_ref, rtol=1e-10, atol=1e-9)


def test_force_matching_is_finite_with_two_coincident_sites():
    xn = lattice_sites(3, 5, 605)
    xn[:, 3] = xn[:, 1]
    x = dev(xn, grad=True)
    d = jaxutil.distances(x, return_matrix=False)
    assert (d == 0).sum() == 3
    g, gg = force_matching(lambda z: jaxutil.distances(z, return_matrix=False), x)
    assert torch.isfinite(g).all() and torch.isfinite(gg).all()
    g_ref, gg_ref = cpu_force_matching(xn, skip={(1, 3)})
    torch.testing.assert_close(g.cpu(), g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg.cpu(), gg_ref, rtol=1e-10, atol=1e-9)


# ------------------------------------------------------------------ 7. memory
def peak_above_baseline(route, x):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    route(x).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    x.grad = None
    return peak


def test_the_triangle_route_allocates_well_under_the_matrix_route():
    """Every (T, n, n) array of the matrix route is a (T, P) array here, P / n^2 < 1/2; the gathered copy is gone;
    the (T, n, 3) site arrays add 3 / n each: with n >= 64 the new peak stays under 0.6 of the old one."""
    T, n = 64, 128
    x = dev(lattice_sites(T, n, 701), grad=True)
    PairList.upper_triangle(n).on(DEV)  # (the list's tables are a per-process constant, not part of a call)
    for route in (matrix_route, lambda z: jaxutil.distances(z, return_matrix=False)):
        route(x).sum().backward()  # (workspaces and caches of a first call)
        x.grad = None
    old = peak_above_baseline(matrix_route, x)
    reset()
    new = peak_above_baseline(lambda z: jaxutil.distances(z, return_matrix=False), x)
    names = launched()
    print(f"peak above baseline: matrix route {old} B, pair-list route {new} B, ratio {new / old:.3f}")
    assert names and all(k.startswith("pairlist_") for k in names), names  # K9a / K9b launch nothing
    assert new <= 0.6 * old


# ------------------------------------------------------------------ 8. layouts and special values
PAD = 64


def placed(arr, k):
    """Device copy of `arr` that starts k elements into a larger allocation whose rest is NaN."""
    buf = torch.full((k + arr.numel() + PAD,), float("nan"), dtype=arr.dtype, device=DEV)
    view = buf[k:k + arr.numel()].view(arr.shape)
    view.copy_(arr)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_operands_one_element_off_alignment_give_the_aligned_results(dtype):
    for pairs, n in ((triangle(65), 65), (random_list(257, 9, 9, 801), 9)):  # (P odd: rows only element-aligned)
        tab = PairList(pairs, n).on(DEV)
        x, c, v, y, w = list_operands(5, pairs, None, n, dtype)
        dv = K.pair_list_dist(x, c, tab)
        px, pv, pw, pdv = (placed(t, 1) for t in (x, v, w, dv))
        for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
            assert torch.equal(K.pair_list_dist(px, px, tab, mode, pv, pv), K.pair_list_dist(x, c, tab, mode, v, y))
        for kw, pkw in (({}, {}), ({"dv": dv}, {"dv": pdv})):
            a, b = K.pair_list_pull(w, x, c, tab, **kw)
            pa, pb = K.pair_list_pull(pw, px, px, tab, **pkw)
            assert torch.isfinite(a).all() and torch.isfinite(b).all()
            assert torch.equal(pa, a) and torch.equal(pb, b)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_non_contiguous_inputs(dtype):
    big = dev(lattice_sites(6, 66, 802), dtype)
    x = big[::2, 1::2]           # (3, 33, 3), strided in frames and sites
    c = big[1::2, :12:2]         # (3, 6, 3)
    assert not x.is_contiguous() and not c.is_contiguous()
    pairs = random_list(70, 6, 33, 803, self_form=False)
    xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    xs, cs = x.detach().requires_grad_(True), c.detach().requires_grad_(True)
    d = pair_distances(xs, pairs, cs)
    dr = pair_distances(xr.contiguous(), pairs, cr.contiguous())
    assert torch.equal(d, dr)
    h = dev(np.random.default_rng(804).standard_normal(tuple(d.shape)), dtype)
    got = torch.autograd.grad(d, (xs, cs), h.t().contiguous().t())  # a strided upstream gradient
    ref = torch.autograd.grad(dr, (xr, cr), h)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_mixed_float32_and_float64_operands_promote():
    x = dev(lattice_sites(3, 7, 805), F32, grad=True)
    c = dev(lattice_sites(3, 4, 806) + 0.4, F64, grad=True)
    pairs = random_list(20, 4, 7, 807, self_form=False)
    reset()
    d = pair_distances(x, pairs, c)
    assert d.dtype == F64 and "pairlist_kernel<double, 0>" in launched()
    ref = np.sqrt((list_disp(host(x), host(c), pairs) ** 2).sum(-1))
    close(d, ref, ref, TOL[F64], "promoted forward")
    gx, gc = torch.autograd.grad((d * d).sum(), (x, c), create_graph=True)
    assert gx.dtype == F32 and gc.dtype == F64
    hx, hc = torch.autograd.grad((gx.double() ** 2).sum() + (gc ** 2).sum(), (x, c))
    assert hx.dtype == F32 and hc.dtype == F64


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["triangle", "chain"])  # the wave form and the lane form of the backward
def test_a_nan_coordinate_reaches_exactly_the_pairs_that_touch_it(dtype, kind):
    n = 70
    pairs = triangle(n) if kind == "triangle" else chain(n)
    xn = lattice_sites(3, n, 808)
    xn[1, 17, 2] = np.nan
    x = dev(xn, dtype, grad=True)
    d = pair_distances(x, pairs)
    touched = np.zeros((3, len(pairs)), dtype=bool)
    touched[1] = (pairs == 17).any(axis=1)
    assert np.array_equal(np.isnan(host(d)), touched)
    (g,) = torch.autograd.grad(d.sum(), x)
    # a touched pair's term is weight x displacement with the NaN in the displacement's z: the z of the two sites of
    # every touched pair is NaN (a product with the zero weight of a NaN distance keeps it, as in K9b), all else finite
    sites = np.unique(pairs[touched[1]])
    expect = np.zeros((3, n, 3), dtype=bool)
    expect[1, sites, 2] = True
    assert 17 in sites and np.array_equal(np.isnan(host(g)), expect) and np.isfinite(host(g)[~expect]).all()
    ref = dev(np.nan_to_num(xn), dtype, grad=True)
    (gr,) = torch.autograd.grad(pair_distances(ref, pairs).sum(), ref)
    assert torch.equal(g[0], gr[0]) and torch.equal(g[2], gr[2])


# ------------------------------------------------------------------ 9. element offsets beyond 2^31
def test_forward_beyond_two_to_the_31_elements():
    T, n = 65800, 256
    P = n * (n - 1) // 2
    assert T * P > 2**31
    need_hbm(12)
    rng = np.random.default_rng(901)
    x = dev(30 * rng.standard_normal((T, n, 3)), F32)
    d = jaxutil.distances(x, return_matrix=False)
    try:
        assert tuple(d.shape) == (T, P) and d.dtype == F32
        i, j = np.triu_indices(n, 1)
        for t in (0, T - 1):
            xt = host(x[t])
            ref = np.sqrt(((xt[j] - xt[i]) ** 2).sum(-1))
            close(d[t], ref, ref, TOL[F32], f"frame {t}")
    finally:
        del d
        torch.cuda.empty_cache()
