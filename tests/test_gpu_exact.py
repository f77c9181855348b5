"""Every contraction kernel bit for bit on integer-valued inputs (tests/exact_ref.py): when L * A * B <= 2**p every
partial sum in any order is an exactly representable integer, so the device output must EQUAL the exact result -- in
float32 and float64 alike, whatever the split count, slab layout, FMA contraction or MFMA accumulation order.  The
tolerance-based parity tests admit a single element counted twice or not at all once a reduction is long
(tests/test_exact_ref_host.py records the sizes); equality admits nothing.

Covered: K1 (streaming, tile, EDGE / straddle / tail-row, packed groups, macro-tile, gram_pair), augmented_gram,
sym_group_reduce, gram_quadform, axpby, sumsq, dot, K3 (every tile class, RAGGED, NaN fill, fused sum of squares),
K3c / K8 (trjdot_frames, _cross, _frames_t, _frames_outer), K4 / K5 sums (frames_matmul, feat_contract, group_reduce,
augment_concat), K9 (pair_dist / pair_list_dist in SQUARE and DOT modes, pair_pull / pair_list_pull with and without Dv).

Left out, because they are no sums of products of their array arguments:
  * the gb_* Gaussian kernels (gb_channels, gb_regmat*, gb_apply*, gbasis_*, gauss_*): exponentials of distances;
  * map validation (mapval): Gaussian projections and residual shifts;
  * the equality-QP solve (eq_qp_solve*): factorisation, divisions and square roots;
  * the noise stream (synth_normal, condnormal_*): Philox + Box-Muller, pinned by tests/test_gpu_noise_stream.py;
  * pair_dist_var / pair_dist_moments / pair_min and the DIST mode of K9a / K9c: square roots;
  * the periodic-box forms of K9: rounding to the nearest image, held bit for bit by tests/test_gpu_pbc.py;
  * residual_over_var: a division by a variance that is no power of two in any caller.

The last test judges a run of the whole module: every instantiation of the contraction families was launched here."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd import _lib  # noqa: E402
from aggforce_amd.constraints import group_layout, groups_csr  # noqa: E402
from aggforce_amd.jaxutil import PairList  # noqa: E402
import exact_ref as X  # noqa: E402
import kernel_inventory as inv  # noqa: E402
from pairlist_ref import chain, random_list, star, triangle  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_TILES = json.load(open(os.path.join(ROOT, "profiles", "r05_routing.json")))["thresholds"]["macro_min_tiles"]["value"]
F32, F64 = torch.float32, torch.float64
NAME = {F32: "float", F64: "double"}
GRAM_PAIRS = [(F64, F64), (F32, F64), (F32, F32)]  # (frames, products)
PAIR_IDS = ["f64", "f32-f64", "f32"]
REACHED = set()   # mangled names of every kernel launched by a test of this module
RAN = set()       # names of the test functions of this module that ran to their end


def dev(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _short(pretty):
    return pretty.split("(")[0].replace("void ", "").replace("aggf::", "")


def reset():
    torch.cuda.synchronize()
    _lib.load().aggf_coverage_reset()


def record(test):
    """The instantiations launched since `reset`, added to the module's reach."""
    torch.cuda.synchronize()
    names = set()
    for mangled, (pretty, count) in _lib.coverage(names=True).items():
        if count > 0:
            REACHED.add(mangled)
            names.add(_short(pretty))
    RAN.add(test)
    return names


def same(got, ref):
    """Bit for bit: the device tensor equals the float64 reference cast to its dtype (exact: the reference holds
    integers, or dyadic fractions, within the dtype's range)."""
    want = torch.from_numpy(np.ascontiguousarray(ref)).to(got.dtype)
    assert torch.equal(want.double(), torch.from_numpy(np.ascontiguousarray(ref))), "the reference is not exact in the output dtype"
    return tuple(got.shape) == tuple(want.shape) and torch.equal(got.cpu(), want)


def chains(N, n_groups, size):
    """(goa, n_red, device CSR or (None, None)) for `n_groups` chains of `size` consecutive atoms at the front."""
    cons = {frozenset([g * size + j, g * size + j + 1]) for g in range(n_groups) for j in range(size - 1)}
    goa, n_red = group_layout(N, cons)
    assert n_red == N - n_groups * (size - 1)
    if n_red == N:
        return None, N, None, None
    p, a = groups_csr(goa, n_red)
    return goa, n_red, dev(p, torch.int32), dev(a, torch.int32)


def gram_is_exact(f, layout, dt, cdt, ref=None, **kw):
    goa, n_red, gp, ga = layout
    ref = X.gram_ref(f, goa, n_red) if ref is None else ref
    G = K.gram(dev(f, dt), gp, ga, n_red, cdt, **kw)
    assert same(G, ref) and torch.equal(G, G.T), (f.shape, dt, cdt, kw)
    return G, ref


# ------------------------------------------------------------------ K1 streaming
PANEL_CLASSES = [(40, 5, 3), (80, 10, 3), (170, 28, 6), (100, 1, 2), (200, 20, 3), (300, 50, 3), (256, 1, 2), (400, 80, 4),
                 (144, 0, 1), (320, 0, 1), (470, 1, 2)]
LONG_CLASS = {(F64, F64): (170, 28, 6), (F32, F64): (256, 1, 2), (F32, F32): (40, 5, 3)}


def _dispatch_cases(dt, cdt):
    cases = json.load(open(os.path.join(ROOT, "tests", "dispatch_cases.json")))["cases"]
    want = (str(dt).replace("torch.", ""), str(cdt).replace("torch.", ""))
    return [c for c in cases if (c["in"], c["compute"]) == want]


@pytest.mark.parametrize("dt,cdt", GRAM_PAIRS, ids=PAIR_IDS)
def test_gram_streaming_kernel(dt, cdt):
    """gram_small_kernel: the panel classes of test_small_system_panel_width_classes at T = 333, one class at
    T = 20011, and one system per instantiation (tests/dispatch_cases.json) with a ragged last stage."""
    reset()
    for N, ng, size in PANEL_CLASSES:
        f = X.gram_frames(333, N, [dt, cdt], group=size, seed=N + ng)
        gram_is_exact(f, chains(N, ng, size), dt, cdt)
    N, ng, size = LONG_CLASS[(dt, cdt)]
    gram_is_exact(X.gram_frames(20011, N, [dt, cdt], group=size, seed=1), chains(N, ng, size), dt, cdt)
    cases = _dispatch_cases(dt, cdt)
    assert len(cases) >= 40
    for c in cases:
        f = X.gram_frames(1037, c["N"], [dt, cdt], group=c["group_size"], seed=c["N"])
        gram_is_exact(f, chains(c["N"], c["n_groups"], c["group_size"]), dt, cdt)
    ran = record("test_gram_streaming_kernel")
    assert any(n.startswith("gram_small_kernel<") for n in ran)


# ------------------------------------------------------------------ K1 tile kernel: EDGE, straddle, tail row
TILE_T = 20003


@pytest.mark.parametrize("N", [500, 513, 639, 640, 643, 1001, 1024])
def test_gram_tile_kernel_edge_straddle_and_tail_row(N):
    """The frames read in place at T = 20003 (many splits, a ragged last stage) in the three dtype pairs: one integer
    array and one host reference for all three (the range is the float32 one).  N = 643 and 1001 also accumulate over
    two frame blocks that start at odd rows; N = 640 and 1001 skip the leading 128 columns."""
    f = X.gram_frames(TILE_T + 1, N, [F32, F64], seed=N)
    ref = X.gram_ref(f[1:])
    reset()
    for dt, cdt in GRAM_PAIRS:
        whole = dev(f, dt)
        block = whole[1:]
        G = K.gram(block, None, None, N, cdt)
        assert same(G, ref) and torch.equal(G, G.T), (N, dt, cdt)
        if N in (643, 1001):
            acc = K.gram(whole[1:7003], None, None, N, cdt)
            K.gram(whole[7003:], None, None, N, cdt, out=acc, accumulate=True)
            assert same(acc, ref) and torch.equal(acc, acc.T), (N, dt, cdt, "accumulate")
        if N in (640, 1001):
            part = torch.full((N, N), -7.0, dtype=F64, device="cuda")
            K.gram(block, None, None, N, cdt, out=part, first_col=128)
            # (include/aggf.h: the leading block is left untouched, or -- a layout that is not read in place --
            # overwritten with its own correct values)
            want = ref.copy()
            if bool((part[:128, :128] == -7.0).all()):
                want[:128, :128] = -7.0
            assert same(part, want), (N, dt, cdt, "first_col")
        del whole, block
    ran = record("test_gram_tile_kernel_edge_straddle_and_tail_row")
    assert any(n.startswith("gram_tile_dma_kernel<") for n in ran)
    assert (N % 2 == 1) == any(n.startswith("gram_tail_row_kernel<double>") for n in ran)


@pytest.mark.parametrize("dt,cdt", GRAM_PAIRS, ids=PAIR_IDS)
def test_gram_packed_groups(dt, cdt, monkeypatch):
    """Constraint groups through the pack + tile pipeline: (600, 100, 4), and 534 reduced columns of 800 atoms in bond
    pairs in the serial and in the overlapped form of the pack (AGGF_GRAM_PACK_MIN_FRAMES, the test hook of
    test_overlapped_pack_pipeline_equals_the_serial_form)."""
    reset()
    f = X.gram_frames(333, 600, [dt, cdt], group=4, seed=3)
    gram_is_exact(f, chains(600, 100, 4), dt, cdt)
    T, N = 2051, 800
    cons = {frozenset([3 * i, 3 * i + 1]) for i in range(N // 3)}
    goa, n_red = group_layout(N, cons)
    assert n_red > 512
    p, a = groups_csr(goa, n_red)
    layout = (goa, n_red, dev(p, torch.int32), dev(a, torch.int32))
    f = X.gram_frames(T, N, [dt, cdt], group=2, seed=4)
    _, ref = gram_is_exact(f, layout, dt, cdt)
    monkeypatch.setenv("AGGF_GRAM_PACK_MIN_FRAMES", "256")
    for form in ("overlap", "chunked", "serial"):
        monkeypatch.setenv("AGGF_GRAM_PACK", form)
        gram_is_exact(f, layout, dt, cdt, ref=ref)
    ran = record("test_gram_packed_groups")
    for nt in ("true", "false"):
        assert f"pack_groups_kernel<{NAME[dt]}, {NAME[cdt]}, {nt}>" in ran, ran


# ------------------------------------------------------------------ K1m macro tiles
def _gram_route(f, route):
    old = os.environ.pop("AGGF_GRAM_ROUTE", None)
    if route:
        os.environ["AGGF_GRAM_ROUTE"] = route
    try:
        return K.gram(f, None, None, f.shape[1], F64)
    finally:
        os.environ.pop("AGGF_GRAM_ROUTE", None)
        if old is not None:
            os.environ["AGGF_GRAM_ROUTE"] = old


@pytest.mark.parametrize("T", [1037, 5])
@pytest.mark.parametrize("N", [MIN_TILES * 128, 3968, 4352])
def test_gram_macro_tiles(N, T):
    """gram_tile_dma_kernel_x2 at its threshold and with paired / lone leftover diagonal tiles; the single-tile kernel
    forced on the same frames gives the same bits.  T = 5 is held to the host reference, T = 1037 (a host product of
    more than a second) to torch's float64 matmul on the device, exact under the same bound."""
    f = X.gram_frames(T, N, [F64], seed=N + T)
    fd = dev(f)
    if T == 5:
        ref = dev(X.gram_ref(f))
    else:
        assert X.bound_ok(3 * T, 100, 100, 53) and float(fd.abs().max()) <= 100
        F2 = fd.permute(0, 2, 1).reshape(3 * T, N)
        ref = F2.T @ F2
    reset()
    G = _gram_route(fd, None)
    ran = record("test_gram_macro_tiles")
    tiles = [n for n in ran if n.startswith("gram_tile_dma_kernel")]
    assert len(tiles) == 1 and tiles[0].startswith("gram_tile_dma_kernel_x2<"), ran
    assert torch.equal(G, ref) and torch.equal(G, G.T)
    reset()
    G1 = _gram_route(fd, "single")
    ran = record("test_gram_macro_tiles")
    assert not any(n.startswith("gram_tile_dma_kernel_x2") for n in ran)
    assert torch.equal(G1, G)


# ------------------------------------------------------------------ gram_pair, augmented_gram, reductions, BLAS-1
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_gram_pair(dt):
    reset()
    for T, N, N2 in [(333, 128, 128), (1001, 256, 128)]:
        a = X.gram_frames(T, N, [dt], seed=T)
        b = X.gram_frames(T, N2, [dt], seed=T + 1)
        ad, bd = dev(a, dt), dev(b, dt)
        assert K.gram_pair_ok(ad, bd)
        G = K.gram_pair(ad, bd)
        assert same(G, X.gram_pair_ref(a, b)) and torch.equal(G, G.T)
    ran = record("test_gram_pair")
    assert f"gram_tile_dma_kernel<{NAME[dt]}, 0, 3, 2, 8, true, 1, true, true, false, {NAME[dt]}>" in ran, ran


def test_augmented_gram_sym_group_reduce_and_quadform():
    rng = np.random.default_rng(5)
    n, n2 = 200, 56
    B = X.integers(rng, (n + n2, 40), 9)
    Gx = B @ B.T                                                    # |entries| <= 40 * 81
    C = np.where(rng.random((n2, n)) < 0.03, X.integers(rng, (n2, n), 5), 0.0)
    per_col = int((C != 0).sum(axis=0).max()) + 1                   # terms of a column of Tm
    assert X.bound_ok(per_col * per_col, 40 * 81, 25, 53)
    reset()
    got = K.augmented_gram(dev(Gx), n, K.premap_columns(C, F64, "cuda"))
    Tm = np.block([[np.eye(n), np.zeros((n, n2))], [-C, np.eye(n2)]])
    assert same(got, Tm.T @ Gx @ Tm) and torch.equal(got, got.T)
    goa, n_red = group_layout(n + n2, {frozenset([0, 5]), frozenset([5, 9]), frozenset([20, 21, 22]), frozenset([100, 255])})
    p, a = groups_csr(goa, n_red)
    Cm = np.zeros((n + n2, n_red))
    Cm[np.arange(n + n2), goa] = 1.0
    red = K.sym_group_reduce(dev(Gx), dev(p, torch.int32), dev(a, torch.int32), n_red)
    assert same(red, Cm.T @ Gx @ Cm) and torch.equal(red, red.T)
    W = X.integers(rng, (7, n + n2), 100)
    assert X.bound_ok((n + n2) ** 2, 40 * 81, 100 * 100, 53)
    q = K.gram_quadform(dev(Gx), dev(W))
    assert same(q, np.einsum("ri,ij,rj->r", W, Gx, W))
    ran = record("test_augmented_gram_sym_group_reduce_and_quadform")
    assert "sym_group_reduce_kernel" in ran


def test_axpby_sumsq_and_dot():
    rng = np.random.default_rng(6)
    n = 1_000_003
    x, y = X.integers(rng, (n,), 100), X.integers(rng, (n,), 100)
    reset()
    assert same(K.axpby(3.0, dev(x), -0.5, dev(y)), 3.0 * x - 0.5 * y)
    assert X.bound_ok(n, 100, 100, 53)                               # (products and sums are float64 for either input dtype)
    for dt in (F64, F32):
        assert same(K.sumsq(dev(x, dt)), np.array([float((x.astype(np.int64) ** 2).sum())])), dt
        for dt2 in (F64, F32):
            assert same(K.dot(dev(x, dt), dev(y, dt2)), np.array([float((x.astype(np.int64) * y.astype(np.int64)).sum())]))
    record("test_axpby_sumsq_and_dot")


# ------------------------------------------------------------------ K3 apply
FEW_SITES, FEW_ATOMS = (1, 10, 16), (3, 20, 40, 64, 97, 175, 333)
TILE_SITES, TILE_ATOMS = (17, 32, 33, 48, 49, 64, 65, 128, 130, 256), (24, 32, 77, 130, 255, 256, 512)
APPLY_T = (1, 63, 65, 1001)


def _apply_cases():
    for sites, atoms in ((FEW_SITES, FEW_ATOMS), (TILE_SITES, TILE_ATOMS)):
        for n_cg in sites:
            for N in atoms:
                for T in APPLY_T:
                    yield n_cg, N, T
    yield 4, 20, 100003


def _exact_sumsq(ref):
    """Sum of squares as a Python integer if it is <= 2**53, else None: the terms are non-negative integers, so every
    partial sum of the device's float64 squares, in any order, is then an exact integer."""
    assert np.abs(ref).max() <= 2 ** 24 and ref[0].size < 2 ** 14  # (no int64 overflow below)
    per_frame = (ref.astype(np.int64) ** 2).reshape(ref.shape[0], -1).sum(axis=1)
    total = sum(int(v) for v in per_frame)
    return total if total <= 2 ** 53 else None


def _apply_is_exact(pts, mat, pdt, mdt, probe, holes=None, fill=None):
    """The output, bit for bit; the NaN probe; the fused sum of squares as an exact integer.  False: the output is exact
    but the sum of squares of THIS data is beyond 2**53 and was not compared."""
    given = pts
    if holes is not None:
        given, pts = pts.copy(), pts.copy()
        given[holes] = np.nan
        pts[holes] = fill
    ref = X.apply_ref(pts, mat)
    total = _exact_sumsq(ref)
    probe.zero_()
    out, ss = K.linearmap_apply(dev(given, pdt), dev(mat, mdt), nan_fill=fill, want_sumsq=True, nan_probe=probe)
    assert out.dtype == mdt and same(out, ref) and int(probe.item()) == int(holes is not None), (pts.shape, mat.shape, fill)
    assert total is None or float(ss.item()) == float(total), (pts.shape, mat.shape, fill)
    return total is not None


@pytest.mark.parametrize("pdt,mdt", [(F64, F64), (F32, F64), (F32, F32), (F64, F32)], ids=["f64", "f32-f64", "f32", "f64-f32"])
def test_apply_every_tile_class(pdt, mdt):
    """aggf_linearmap_apply by site count (few-sites stage classes, 32- / 48- / 64- / 128-site tiles, the LDS-DMA forms
    and their RAGGED instantiations at N % 16 != 0) in the plain mode with the fused sum of squares, and in NaN-fill mode
    with an integer fill."""
    reset()
    probe = torch.zeros(1, dtype=torch.int32, device="cuda")
    for n_cg, N, T in _apply_cases():
        seed = 1000 * n_cg + N + T
        rng = np.random.default_rng(seed)
        holes = (rng.integers(0, T, size=5), rng.integers(0, N, size=5), rng.integers(0, 3, size=5))
        holes = tuple(np.concatenate([h, [e]]) for h, e in zip(holes, (T - 1, N - 1, 2)))  # ... and the last element
        pts, mat = X.operand_pair(N, (T, N, 3), (n_cg, N), [pdt, mdt], seed=seed)
        fill = float(-(int(np.abs(pts).max()) // 2 + 1))
        ok = _apply_is_exact(pts, mat, pdt, mdt, probe)
        ok = _apply_is_exact(pts, mat, pdt, mdt, probe, holes, fill) and ok
        if not ok:
            # the sum of squares of the widest range leaves float64's integers: once more with the range under which
            # 3 T n_cg (N r^2)^2 <= 2**53 holds whatever the data
            cap = int((2 ** 53 // (3 * T * n_cg * N * N)) ** 0.25)
            assert cap >= 2 and 3 * T * n_cg * (N * cap * cap) ** 2 <= 2 ** 53
            pts, mat = X.operand_pair(N, (T, N, 3), (n_cg, N), [pdt, mdt], seed=seed, cap=cap)
            assert _apply_is_exact(pts, mat, pdt, mdt, probe) and _apply_is_exact(pts, mat, pdt, mdt, probe, holes, -1.0)
    record("test_apply_every_tile_class")


# ------------------------------------------------------------------ K3c / K8
@pytest.mark.parametrize("pd,fd", [(F64, F64), (F64, F32), (F32, F64), (F32, F32)], ids=["f64", "f64-f32", "f32-f64", "f32"])
def test_trjdot_frames(pd, fd):
    reset()
    for T, n_cg, N in [(200, 257, 1001), (2000, 10, 166), (3, 1, 1), (7, 17, 33), (67, 33, 130)]:
        pts, fac = X.operand_pair(N, (T, N, 3), (T, n_cg, N), [pd, fd], seed=T + N)
        out = K.trjdot_frames(dev(pts, pd), dev(fac, fd))
        assert out.dtype == torch.promote_types(pd, fd) and same(out, X.frames_ref(pts, fac)), (T, n_cg, N)
        for td in (F32, F64):
            r = X.int_range(N + 1, [pd, fd, td])                      # the translation: one more term, <= r * r
            rng = np.random.default_rng(T + N + 1)
            pts2, fac2, trans = X.integers(rng, (T, N, 3), r), X.integers(rng, (T, n_cg, N), r), X.integers(rng, (T, n_cg, 3), r)
            out = K.trjdot_frames(dev(pts2, pd), dev(fac2, fd), dev(trans, td))
            assert same(out, X.frames_ref(pts2, fac2, trans)), (T, n_cg, N, td)
    record("test_trjdot_frames")


CROSS_SHAPES = [(257, 4096, 2000), (10, 166, 2000), (17, 1001, 2000), (1, 7, 3)]  # (n_a, n_b, T) of test_gpu_autograd.py
CROSS_REF = {}


def _cross_case(n_a, n_b, T):
    """One integer pair and one host reference per shape, shared by the dtype pairs (the float32 range)."""
    key = (n_a, n_b, T)
    if key not in CROSS_REF:
        a, b = X.operand_pair(3 * T, (T, n_a, 3), (T, n_b, 3), [F32, F64], seed=n_a + n_b)
        CROSS_REF[key] = (a, b, X.cross_ref(a, b))
    return CROSS_REF[key]


@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32), (F32, F64)], ids=["f32", "f64", "f64-f32", "f32-f64"])
def test_trjdot_cross(ind, outd):
    """K8a at the shapes of test_gpu_autograd.py, and T = 20003 (many splits) accumulated onto a first block."""
    reset()
    for n_a, n_b, T in CROSS_SHAPES:
        a, b, ref = _cross_case(n_a, n_b, T)
        assert same(K.trjdot_cross(dev(a, ind), dev(b, ind), outd), ref), (n_a, n_b, T)
    a, b, ref = _cross_case(10, 166, 20003)
    ad, bd = dev(a, ind), dev(b, ind)
    assert same(K.trjdot_cross(ad, bd, outd), ref)
    acc = K.trjdot_cross(ad[:7001], bd[:7001], outd)
    K.trjdot_cross(ad[7001:], bd[7001:], outd, out=acc, accumulate=True)
    assert same(acc, ref)
    record("test_trjdot_cross")


FRAME_SHAPES = [(200, 257, 1001), (2000, 10, 166), (3, 1, 1), (7, 17, 33), (67, 300, 130)]  # (T, n_cg, N)


@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32)], ids=["f32", "f64", "f64-f32"])
def test_trjdot_frames_t_and_outer(ind, outd):
    reset()
    for T, n_cg, N in FRAME_SHAPES:
        g, f = X.operand_pair(n_cg, (T, n_cg, 3), (T, n_cg, N), [ind, outd], seed=T)
        assert same(K.trjdot_frames_t(dev(g, ind), dev(f, ind), outd), X.frames_t_ref(g, f)), (T, n_cg, N)
        g, p = X.operand_pair(3, (T, n_cg, 3), (T, N, 3), [ind, outd], seed=T + 1)
        assert same(K.trjdot_frames_outer(dev(g, ind), dev(p, ind), outd), X.frames_outer_ref(g, p)), (T, n_cg, N)
    record("test_trjdot_frames_t_and_outer")


# ------------------------------------------------------------------ K4 / K5 sums
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
def test_frames_matmul(dt):
    rng = np.random.default_rng(8)
    reset()
    for T, Kd, J in [(333, 30, 12), (1037, 97, 130), (65, 1, 1), (64, 33, 65)]:
        # alpha = 2 and the difference x - sub double the operand twice over; `add` is one more term within the bound
        r = X.int_range(Kd + 1, [dt], 4, 1)
        x, sub, b = X.integers(rng, (T, Kd), r), X.integers(rng, (T, Kd), r), X.integers(rng, (J, Kd), r)
        add = X.integers(rng, (T, J), r)
        xd, sd, bd, addd = dev(x, dt), dev(sub, dt), dev(b, dt), dev(add, dt)
        assert same(K.frames_matmul(xd, bd), x @ b.T)
        assert same(K.frames_matmul(xd, bd, sub=sd), (x - sub) @ b.T)
        assert same(K.frames_matmul(xd, bd, sub=sd, add=addd, alpha=2.0), add + 2.0 * ((x - sub) @ b.T)), (T, Kd, J)
    ran = record("test_frames_matmul")
    assert f"frames_matmul_kernel<{NAME[dt]}>" in ran


@pytest.mark.parametrize("fdt,xdt", [(F64, F64), (F64, F32), (F32, F64), (F32, F32)], ids=["f64", "f64-f32", "f32-f64", "f32"])
def test_feat_contract(fdt, xdt):
    rng = np.random.default_rng(9)
    reset()
    for T, N, n_feat, ld in [(203, 11, 9, 16), (67, 130, 300, 300), (5, 257, 33, 64)]:
        forces, feat = X.operand_pair(N + 1, (T, N, 3), (T, N, n_feat), [fdt, xdt], seed=T)
        div = 2.0 * X.integers(rng, (T, n_feat, 3), 50)              # alpha = 0.5 of an even integer: one more term
        want = np.einsum("taf,tad->tfd", feat, forces)
        got = K.feat_contract(dev(forces, fdt), dev(feat, xdt), None, 0.0, ld)
        assert same(got[:, :n_feat], want) and not got[:, n_feat:].any()
        got = K.feat_contract(dev(forces, fdt), dev(feat, xdt), dev(div, xdt), 0.5, ld)
        assert got.dtype == torch.promote_types(fdt, xdt) and tuple(got.shape) == (T, ld, 3)
        assert same(got[:, :n_feat], want + 0.5 * div) and not got[:, n_feat:].any(), (T, N, n_feat, ld)
    record("test_feat_contract")


@pytest.mark.parametrize("ind,outd", [(F64, F64), (F64, F32), (F32, F64), (F32, F32)], ids=["f64", "f64-f32", "f32-f64", "f32"])
def test_group_reduce(ind, outd):
    """Sums, and means over groups of 1, 2 and 4 members (the weight 1 / size is a power of two: exact quotients)."""
    rng = np.random.default_rng(10)
    T, N = 333, 45
    sizes = [1, 2, 4] * 6 + [3]
    atoms = rng.permutation(N)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    assert ptr[-1] == N
    x = X.integers(rng, (T, N, 3), X.int_range(4, [ind, outd], 1, 4))  # (a mean's terms carry two more binary places)
    reset()
    sums = X.group_sum_ref(x, ptr, atoms)
    gp, ga = dev(ptr, torch.int32), dev(atoms, torch.int32)
    assert same(K.group_reduce(dev(x, ind), gp, ga, len(sizes), False, outd), sums)
    pow2 = [g for g, s in enumerate(sizes) if s != 3]
    got = K.group_reduce(dev(x, ind), gp, ga, len(sizes), True, outd)
    assert same(got[:, pow2], sums[:, pow2] / np.array(sizes, dtype=np.float64)[pow2][None, :, None])
    ran = record("test_group_reduce")
    assert f"group_reduce_kernel<{NAME[ind]}, {NAME[outd]}>" in ran


@pytest.mark.parametrize("cdt,gdt", [(F64, F64), (F32, F64), (F64, F32), (F32, F32)], ids=["f64", "f32-f64", "f64-f32", "f32"])
def test_augment_concat(cdt, gdt):
    rng = np.random.default_rng(11)
    T, N, n = 333, 9, 4
    x, F, corr = (X.integers(rng, (T, N, 3), 100) for _ in range(3))
    y, lg = X.integers(rng, (T, n, 3), 100), X.integers(rng, (T, n, 3), 100)
    reset()
    for kbt in (0.5, 4.0):
        oc, of = K.augment_concat(dev(x, cdt), dev(F, cdt), dev(y, gdt), dev(corr, gdt), dev(lg, gdt), kbt)
        assert oc.dtype == of.dtype == torch.promote_types(cdt, gdt)
        assert same(oc, np.concatenate([x, y], axis=1)) and same(of, np.concatenate([F + kbt * corr, kbt * lg], axis=1))
    record("test_augment_concat")


# ------------------------------------------------------------------ K9 pair distances and pulls
K9_SHAPES = [(1, 1, 1), (3, 5, 4), (67, 17, 33), (5, 65, 257), (2, 257, 65), (3, 1, 300), (3, 300, 1), (3, 9, 200)]  # (T, m, n)
K9_ALL = [(s, False) for s in K9_SHAPES] + [((T, n, n), True) for T, _, n in K9_SHAPES[:-1]]


def _sites(T, m, n, self_form, dtypes, L, seed, dv_bits=0):
    """x (T, n, 3), c (T, m, 3) (x itself in the self form), v, y alike, weights (T, m, n): displacements are differences
    (twice the range), weights over a power-of-two Dv carry `dv_bits` more binary places."""
    r = X.int_range(L, dtypes, 2, 2 ** dv_bits if dv_bits else 2)
    rng = np.random.default_rng(seed)
    x, v = X.integers(rng, (T, n, 3), r), X.integers(rng, (T, n, 3), r)
    c, y = (x, v) if self_form else (X.integers(rng, (T, m, 3), r), X.integers(rng, (T, m, 3), r))
    return x, c, v, y, rng, r


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_pair_dist_square_and_dot(dtype):
    reset()
    for (T, m, n), self_form in K9_ALL:
        x, c, v, y, _, _ = _sites(T, m, n, self_form, [dtype], 3, T + m + n)
        u, g = X.pair_disp(x, c), X.pair_disp(v, y)
        xd, vd = dev(x, dtype), dev(v, dtype)
        cd, yd = (xd, vd) if self_form else (dev(c, dtype), dev(y, dtype))
        assert same(K.pair_dist(xd, cd, K.PAIR_SQDIST), (u * u).sum(-1)), (T, m, n, self_form)
        assert same(K.pair_dist(xd, cd, K.PAIR_DOT, vd, yd), (g * u).sum(-1)), (T, m, n, self_form)
    record("test_pair_dist_square_and_dot")


@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32)], ids=["f32", "f64", "f64-f32"])
def test_pair_pull(ind, outd):
    """K9b: both sums, one panel and several, frames per wave (at most 128 rows) and per workgroup; with a Dv of powers
    of two that includes zeros (weight 0)."""
    reset()
    for (T, m, n), self_form in K9_ALL:
        for dv_bits in (0, 3):
            x, c, _, _, rng, r = _sites(T, m, n, self_form, [ind, outd], max(m, n), T + m + n, dv_bits)
            w = X.integers(rng, (T, m, n), r)
            u = X.pair_disp(x, c)
            xd = dev(x, ind)
            cd = xd if self_form else dev(c, ind)
            if dv_bits:
                dv = X.powers_of_two(rng, (T, m, n), zeros=0.1, kmax=dv_bits)
                weights = np.where(dv > 0, w / np.where(dv > 0, dv, 1.0), 0.0)
                a, b = K.pair_pull(dev(w, ind), xd, cd, dv=dev(dv, ind), out_dtype=outd)
            else:
                weights = w
                a, b = K.pair_pull(dev(w, ind), xd, cd, out_dtype=outd)
            a_ref, b_ref = X.pair_pull_ref(weights, u)
            assert same(a, a_ref) and same(b, b_ref), (T, m, n, self_form, dv_bits)
    record("test_pair_pull")


LIST_CASES = ([(f"triangle{n}", triangle(n), None, n) for n in (5, 65, 130)] + [("chain130", chain(130), None, 130)]
              + [("star300", star(300), None, 300)] + [(f"random{P}", random_list(P, 9, 9, 200 + P), None, 9) for P in (1, 64, 257)]
              + [("cross", random_list(70, 6, 11, 300, self_form=False), 6, 11)])


def _list_sites(T, pairs, m, n, dtypes, L, dv_bits=0):
    x, c, v, y, rng, r = _sites(T, n if m is None else m, n, m is None, dtypes, L, T + len(pairs) + n, dv_bits)
    return x, c, v, y, rng, r


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_pair_list_dist_square_and_dot(dtype):
    reset()
    for _, pairs, m, n in LIST_CASES:
        tab = PairList(pairs, n, m).on("cuda")
        for T in (1, 67):
            x, c, v, y, _, _ = _list_sites(T, pairs, m, n, [dtype], 3)
            u = x[:, pairs[:, 1]] - c[:, pairs[:, 0]]
            g = v[:, pairs[:, 1]] - y[:, pairs[:, 0]]
            xd, vd = dev(x, dtype), dev(v, dtype)
            cd, yd = (xd, vd) if m is None else (dev(c, dtype), dev(y, dtype))
            assert same(K.pair_list_dist(xd, cd, tab, K.PAIR_SQDIST), (u * u).sum(-1))
            assert same(K.pair_list_dist(xd, cd, tab, K.PAIR_DOT, vd, yd), (g * u).sum(-1))
    record("test_pair_list_dist_square_and_dot")


@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32)], ids=["f32", "f64", "f64-f32"])
def test_pair_list_pull(ind, outd):
    """K9d in both forms (longest incidence run <= 32: a lane per site; beyond: a wave per site), with and without Dv."""
    reset()
    forms = set()
    for _, pairs, m, n in LIST_CASES:
        pl = PairList(pairs, n, m)
        tab = pl.on("cuda")
        degs = [deg for _, _, deg in pl.tables()]
        forms |= {int(d > 32) for d in degs}
        rows = n if m is None else m
        for T in (1, 67):
            for dv_bits in (0, 3):
                x, c, _, _, rng, r = _list_sites(T, pairs, m, n, [ind, outd], max(max(degs), 1), dv_bits)
                w = X.integers(rng, (T, len(pairs)), r)
                u = x[:, pairs[:, 1]] - c[:, pairs[:, 0]]
                xd = dev(x, ind)
                cd = xd if m is None else dev(c, ind)
                if dv_bits:
                    dv = X.powers_of_two(rng, (T, len(pairs)), zeros=0.1, kmax=dv_bits)
                    weights = np.where(dv > 0, w / np.where(dv > 0, dv, 1.0), 0.0)
                    a, b = K.pair_list_pull(dev(w, ind), xd, cd, tab, dv=dev(dv, ind), out_dtype=outd)
                else:
                    weights = w
                    a, b = K.pair_list_pull(dev(w, ind), xd, cd, tab, out_dtype=outd)
                a_ref, b_ref = X.list_pull_ref(weights, u, pairs, rows, n)
                assert same(a, a_ref) and same(b, b_ref), (len(pairs), m, n, T, dv_bits)
    assert forms == {0, 1}
    ran = record("test_pair_list_pull")
    for dvs in ("true", "false"):
        for form in (0, 1):
            assert f"pairlist_pull_kernel<{NAME[ind]}, {NAME[outd]}, {dvs}, {form}>" in ran, ran


# ------------------------------------------------------------------ teeth
def _three(shape, member=None):
    perts = X.perturbations(shape, member)
    return [perts[0], perts[len(perts) // 2], perts[-1]]


def test_a_single_changed_element_fails_the_comparison():
    """One long float32 case per family: three of `perturbations` applied to the input OF THE REFERENCE ONLY -- the
    unchanged device output no longer equals it.  (tests/test_exact_ref_host.py: the tolerance-based tests pass such a
    change.)"""
    reset()
    f = X.gram_frames(TILE_T, 500, [F32], seed=500)
    G = K.gram(dev(f, F32), None, None, 500, F32)
    assert same(G, X.gram_ref(f))
    for _, idx in _three(f.shape):
        assert not same(G, X.gram_ref(X.perturb(f, idx))), ("gram", idx)
    pts, mat = X.operand_pair(20, (100003, 20, 3), (4, 20), [F32], seed=2)
    out = K.linearmap_apply(dev(pts, F32), dev(mat, F32))
    assert same(out, X.apply_ref(pts, mat))
    for _, idx in _three(pts.shape):
        assert not same(out, X.apply_ref(X.perturb(pts, idx), mat)), ("apply", idx)
    a, b = X.operand_pair(3 * TILE_T, (TILE_T, 10, 3), (TILE_T, 166, 3), [F32], seed=3)
    out = K.trjdot_cross(dev(a, F32), dev(b, F32), F32)
    assert same(out, X.cross_ref(a, b))
    for _, idx in _three(a.shape):
        assert not same(out, X.cross_ref(X.perturb(a, idx), b)), ("K8a", idx)
    T, m, n = 5, 257, 257
    x, c, _, _, rng, r = _sites(T, m, n, False, [F32], n, 4)
    w = X.integers(rng, (T, m, n), r)
    A, B = K.pair_pull(dev(w, F32), dev(x, F32), dev(c, F32))
    a_ref, b_ref = X.pair_pull_ref(w, X.pair_disp(x, c))
    assert same(A, a_ref) and same(B, b_ref)
    for _, idx in _three(w.shape):
        a_ref, b_ref = X.pair_pull_ref(X.perturb(w, idx), X.pair_disp(x, c))
        assert not same(A, a_ref) and not same(B, b_ref), ("K9b", idx)
    record("test_a_single_changed_element_fails_the_comparison")


# ------------------------------------------------------------------ reach
FAMILIES = ("gram_small_kernel", "gram_tile_dma_kernel", "gram_tile_dma_kernel_x2", "gram_tail_row_kernel", "gram_reduce",
            "pack_groups_kernel", "apply_dma_kernel", "apply_kernel", "apply_small_kernel", "trjdot_", "frames_matmul_kernel",
            "feat_contract", "group_reduce", "sym_group_reduce_kernel", "pairpull", "pairlist_pull_kernel")

# instantiation -> (reason, the existing test that reaches it)
EXCUSED = {}


def test_zz_every_contraction_instantiation_ran_on_exact_data(request):
    """Judges a run of the whole module only (a `-k` selection or a partial run skips it)."""
    declared = {n for n, v in globals().items() if n.startswith("test_") and callable(v)} - {request.node.name.split("[")[0]}
    if request.config.option.keyword or RAN != declared:
        pytest.skip("the reach of the exact tests is judged on a run of the whole module only")
    compiled = inv.compiled_kernels(_lib.LIB_PATH)
    pretty = {k: _short(v) for k, v in inv.demangle(sorted(compiled)).items()}
    family = {k: v for k, v in pretty.items() if v.startswith(FAMILIES)}  # mangled -> short name
    assert len(family) > 250, "kernel inventory looks wrong"
    assert not [k for k in REACHED if k not in compiled and not k.startswith("?")], "launched kernels missing from the inventory"
    assert set(EXCUSED) <= set(family.values()), sorted(set(EXCUSED) - set(family.values()))
    assert 10 * len(EXCUSED) <= len(family), f"{len(EXCUSED)} of {len(family)} instantiations excused: more than one in ten"
    missing = sorted(v for k, v in family.items() if k not in REACHED and v not in EXCUSED)
    idle = sorted(v for k, v in family.items() if k in REACHED and v in EXCUSED)
    n_reached = len([k for k in family if k in REACHED])
    print(f"exact reach: {n_reached} of {len(family)} instantiations, {len(EXCUSED)} excused")
    assert not missing, f"{len(missing)} of {len(family)} instantiations ran on no exact data:\n" + "\n".join(missing)
    assert not idle, f"excused but reached: {idle}"
