"""GPU: every kernel route on inputs that sit anywhere in memory, and the small kernels of the NaN policy on IEEE special
values.

Layouts.  The C ABI asks of an input only the alignment of its element type (include/aggf.h: K1, K3), yet the kernels
issue 16-byte loads and LDS-DMA.  `forces[1:]`, a cross-validation fold or a chunk of a memory-mapped trajectory give
such pointers, and `as_device` keeps them as they are.  `placed` puts an array k elements into a larger allocation --
or its first element one element before a 4 KiB boundary, so that 16-byte pieces cross pages -- and fills the rest of
the allocation with NaN: a read outside the array shows up in the result.  Each result is compared ELEMENTWISE with a
float64 NumPy restatement of the values as stored: |got - ref| <= tol * bound, bound = the same contraction over
absolute values (a misread piece at a row end moves one small entry, which a max-relative measure cannot see).  Each
check also asserts the kernel family that ran, and that an offset input runs the same kernels as an aligned copy.

Special values.  `has_nan`, `allclose` (the np.allclose of the NaN policy, map/core.py:230-232) and `sumsq` against
NumPy on NaN, +-inf, -0.0, subnormals and the top of the float32 range; the NaN policy of LinearMap / JLinearMap
against a NumPy restatement of the reference (map/core.py:219-237, jaxlinearmap.py:15-40 / 95-115), overflow to
infinity included."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from aggforce_amd import LinearMap, _lib, project_forces  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd.map import JLinearMap  # noqa: E402
import mapval_ref as mv  # noqa: E402

F32, F64 = np.float32, np.float64
TD = {F32: torch.float32, F64: torch.float64}
TOL = {F32: 5e-5, F64: 1e-12}
# element offsets: float32 at 4, 8 and 12 bytes past a 16-byte boundary, float64 at 8; "page": first element one
# element before a 4 KiB boundary
OFFSETS = {F32: (1, 2, 3, "page"), F64: (1, "page")}
PAD = 64  # elements behind the array: covers any 16-byte overrun


def placed(arr, k):
    """Device copy of `arr` (contiguous, same shape and dtype) that starts k elements into a larger allocation, or
    (k = "page") with its first element one element before a 4 KiB boundary.  The rest of the allocation is NaN.
    Returns (view, whole allocation)."""
    arr = np.ascontiguousarray(arr)
    es = arr.itemsize
    lead = 4096 // es if k == "page" else k
    buf = torch.full((lead + arr.size + PAD,), float("nan"), dtype=TD[arr.dtype.type], device="cuda")
    if k == "page":
        k = ((4096 - es - buf.data_ptr() % 4096) % 4096) // es
        assert (buf.data_ptr() + (k + 1) * es) % 4096 == 0
    view = buf[k:k + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(arr))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view, buf


def aligned(arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def bits(t):
    """The bytes of a tensor (NaN == NaN)."""
    return t.detach().view(torch.int32 if t.dtype == torch.float32 else torch.int64).clone()


def close(got, ref, bound, tol, what=""):
    """|got - ref| <= tol * bound elementwise (bound: the same contraction over |terms|, float64)."""
    got = host(got) if hasattr(got, "detach") else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    lim = tol * bound + 1e-300
    worst = float(np.max(err / lim)) if err.size else 0.0
    assert worst <= 1.0, f"{what}: error {worst:.3g} x the {tol:g} bound"


def launched():
    """Demangled names of the kernels launched since the last reset."""
    return sorted(p.split("(")[0].replace("void ", "") for p, c in _lib.coverage(names=True).values() if c > 0)


def reset():
    _lib.load().aggf_coverage_reset()


def same_route(run, offset_args, aligned_args, family):
    """run(*offset_args) launches what run(*aligned_args) launches, and a kernel of `family` among them."""
    reset()
    got = run(*offset_args)
    torch.cuda.synchronize()
    names = launched()
    reset()
    run(*aligned_args)
    torch.cuda.synchronize()
    assert names == launched(), (names, launched())
    assert any(family in n for n in names), (family, names)
    return got


def frames(T, N, dt, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal((T, N, 3))).astype(dt)


# ------------------------------------------------------------------ K3 linearmap_apply: every route at every offset
# (n_cg, N, T): tests/test_gpu_dispatch_classes.py's APPLY_SHAPES (the T of the two long few-site shapes cut to keep
# the run short: 40 frames per stage still leave a ragged last stage), then LDS-DMA shapes with N % 16 == 0 -- 17-32,
# 33-48, 49-64 (float32 frames: the three-slot MODE 0 form), 65-128 and more than 128 sites.
APPLY_SHAPES = [(10, 175, 1003), (4, 20, 20003), (5, 64, 5003), (16, 40, 5001), (16, 97, 5003), (7, 130, 5003),
                (3, 300, 5003), (20, 77, 333), (40, 200, 257), (60, 130, 300), (130, 150, 200), (200, 1001, 129),
                (20, 24, 333), (40, 28, 257), (60, 30, 300), (130, 31, 200),
                (24, 64, 301), (40, 48, 97), (50, 48, 257), (100, 64, 130), (150, 32, 100)]


def apply_family(n_cg, N, T, pdt, mdt, replace):
    """The K3 kernel family aggf_linearmap_apply picks (aggf_apply.hip: apply_typed)."""
    frame, cap = 3 * N * np.dtype(pdt).itemsize, 5 * 512 * 16
    if n_cg <= 16 and 8 * frame <= cap and T >= 64:
        return "apply_small_kernel"
    if mdt == F64 and not replace and N >= 32 and n_cg > 16:
        return "apply_dma_kernel"
    return "aggf::apply_kernel<"


def apply_ref(pts, mat):
    """(trjdot in float64 of the stored values, the same over absolute values); the map's dtype is the product's."""
    p = pts.astype(mat.dtype).astype(F64)  # float64 frames with a float32 map are read as float32
    m = mat.astype(F64)
    return np.matmul(m, p), np.matmul(np.abs(m), np.abs(p))


@pytest.mark.parametrize("pdt,mdt", [(F64, F64), (F32, F64), (F32, F32), (F64, F32)])
def test_apply_every_route_at_every_offset(pdt, mdt):
    """aggf_linearmap_apply with the frames, the map, or both at element offsets: both NaN modes, fused sum of squares
    and NaN probe, elementwise against NumPy."""
    rng = np.random.default_rng(11)
    tol = TOL[F32] if F32 in (pdt, mdt) else TOL[F64]
    for n_cg, N, T in APPLY_SHAPES:
        pts = frames(T, N, pdt, n_cg + N, 50.0)
        mat = rng.standard_normal((n_cg, N)).astype(mdt)
        holes = rng.integers(0, T, size=7), rng.integers(0, N, size=7), rng.integers(0, 3, size=7)
        holes = (np.r_[holes[0], T - 1], np.r_[holes[1], N - 1], np.r_[holes[2], 2])  # the array's last element too
        bad = pts.copy()
        bad[holes] = np.nan
        filled = pts.copy()
        filled[holes] = -1.0
        ref, bound = apply_ref(pts, mat)
        ref_f, bound_f = apply_ref(filled, mat)
        m_al = aligned(mat)
        m_off, _ = placed(mat, 1)
        for replace in (False, True):
            src, want, wbound = (bad, ref_f, bound_f) if replace else (pts, ref, bound)

            def run(p, m, replace=replace):
                probe = torch.zeros(1, dtype=torch.int32, device="cuda")
                out, ss = K.linearmap_apply(p, m, nan_fill=-1.0 if replace else None, want_sumsq=True, nan_probe=probe)
                return out, ss, int(probe.item())

            fam = apply_family(n_cg, N, T, pdt, mdt, replace)
            p_al = aligned(src)
            cases = [(placed(src, k)[0], m_al, f"P+{k}") for k in OFFSETS[pdt]]
            cases += [(p_al, m_off, "M+1"), (placed(src, OFFSETS[pdt][-2])[0], m_off, "both")]
            for p, m, where in cases:
                what = f"({n_cg}, {N}, {T}) {where} replace={replace}"
                out, ss, seen = same_route(run, (p, m), (p_al, m_al), fam)
                assert out.dtype == TD[mdt] and seen == int(replace), what
                close(out, want, wbound, tol, what)
                o = host(out)
                assert abs(float(ss.item()) - float((o * o).sum())) <= 1e-5 * float((o * o).sum()), what


@pytest.mark.parametrize("pdt,odt", [(F64, F64), (F32, F64), (F32, F32), (F64, F32)])
def test_slice_gather_at_every_offset(pdt, odt):
    """aggf_slice_gather (K3b, the one-hot map) from frames at element offsets, NaN probe included: exact."""
    T, N = 3001, 175
    pts = frames(T, N, pdt, 3, 20.0)
    idx = np.array([0, 1, 17, 98, 173, N - 1], dtype=np.int32)
    di = torch.from_numpy(idx).cuda()

    def run(p):
        probe = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = K.slice_gather(p, di, TD[odt], nan_probe=probe)
        return out, int(probe.item())

    want = pts[:, idx, :].astype(odt)
    for k in OFFSETS[pdt]:
        out, seen = same_route(run, (placed(pts, k)[0],), (aligned(pts),), "slice_gather_kernel")
        assert seen == 0 and np.array_equal(out.cpu().numpy(), want), k
    bad = pts.copy()
    bad[T - 1, N - 1, 2] = np.nan
    out, seen = run(placed(bad, OFFSETS[pdt][0])[0])
    assert seen == 1 and np.isnan(out[T - 1, -1, 2].item())


# ------------------------------------------------------------------ K1 Gram: small-system, streaming and tile routes
def groups_of(N, pairs):
    """(group of each atom, n_red, grp_ptr, grp_atoms) for bond pairs (3i, 3i+1) or none."""
    goa = np.arange(N)
    if pairs:
        for i in range(N // 3):
            goa[3 * i + 1] = -1
        keep = goa >= 0
        goa[keep] = np.arange(keep.sum())
        for i in range(N // 3):
            goa[3 * i + 1] = goa[3 * i]
    n_red = int(goa.max()) + 1
    order = np.argsort(goa, kind="stable").astype(np.int32)
    ptr = np.searchsorted(goa[order], np.arange(n_red + 1)).astype(np.int32)
    return goa, n_red, ptr, order


# (N, route of the no-group layout): 61/62 atoms the small-system kernel, 200/201 a two-tile panel of the streaming
# kernel, 601/602 (five tiles) the LDS-DMA tile kernel; odd and even N, none a multiple of 128
GRAM_CASES = [(61, "gram_small_kernel"), (62, "gram_small_kernel"), (200, "gram_small_kernel"),
              (201, "gram_small_kernel"), (601, "gram_tile_dma_kernel"), (602, "gram_tile_dma_kernel")]


@pytest.mark.parametrize("dt,cdt", [(F64, F64), (F32, F64), (F32, F32)])
def test_gram_every_route_at_every_offset(dt, cdt):
    """aggf_gram on frame blocks at element offsets -- float32 at 1, 2 and 3 elements, which `x[1:]` cannot give --
    with and without constraint groups, elementwise against the float64 Gram of the stored values."""
    T = 1201
    for N, family in GRAM_CASES:
        f = frames(T, N, dt, N, 3.0)
        for pairs in (False, True):
            goa, n_red, gptr, gat = groups_of(N, pairs)
            C = np.zeros((n_red, N))
            C[goa, np.arange(N)] = 1.0
            S, Sa = np.matmul(C, f.astype(F64)), np.matmul(C, np.abs(f.astype(F64)))  # group sums (T, n_red, 3)
            ref = np.tensordot(S, S, axes=([0, 2], [0, 2]))
            bound = np.tensordot(Sa, Sa, axes=([0, 2], [0, 2]))
            gp = ga = None
            if pairs:
                gp, ga = torch.from_numpy(gptr).cuda(), torch.from_numpy(gat).cuda()

            def run(x):
                return K.gram(x, gp, ga, n_red, TD[cdt])

            fam = family if not pairs else "gram_"
            for k in OFFSETS[dt]:
                G = same_route(run, (placed(f, k)[0],), (aligned(f),), fam)
                close(G, ref, bound, TOL[cdt], f"N={N} pairs={pairs} +{k}")
                assert torch.equal(G, G.T)


def test_gram_from_column_on_odd_rows_matches_and_packs_once():
    """aggf_gram_from_column as qp/gbfeat.py:415/419/564 call it: float64 rows that are not whole 16-byte pieces
    (odd N), N % 128 != 0, first_col > 0, aligned and at an offset.  Off the leading block it equals the full Gram;
    the workspace it is given was planned for its own first_col, so the pack pass runs as ONE chunk (planned with
    first_col = 0 the pack chunks were carved out of a slab-only workspace: one pack, table, tile and reduce launch
    per few thousand frames)."""
    T, N = 4001, 601
    f = frames(T, N, F64, 5, 2.0)
    ref = np.tensordot(f, f, axes=([0, 2], [0, 2]))
    bound = np.tensordot(np.abs(f), np.abs(f), axes=([0, 2], [0, 2]))
    for first in (128, 256, 512):
        mask = np.ones((N, N), dtype=bool)
        mask[:first, :first] = False
        for x in (aligned(f), placed(f, 1)[0]):
            full = K.gram(x, None, None, N, torch.float64)
            part = torch.full((N, N), -7.0, dtype=torch.float64, device="cuda")
            reset()
            K.gram(x, None, None, N, torch.float64, out=part, first_col=first)
            torch.cuda.synchronize()
            packs = sum(c for p, c in _lib.coverage(names=True).values() if "pack_groups_kernel" in p)
            assert packs <= 1, (first, packs)
            p = host(part)
            close(p[mask], ref[mask], bound[mask], TOL[F64], f"first_col={first}")
            assert float(np.max(np.abs(p[mask] - host(full)[mask]))) <= 1e-12 * float(np.max(np.abs(ref)))


# ------------------------------------------------------------------ K3c, K7, K8 at offsets
@pytest.mark.parametrize("dt", [F32, F64])
def test_trjdot_frames_and_k8_contractions_at_offsets(dt):
    """K3c trjdot_frames (with and without the translation term) and the K8 backward contractions trjdot_cross,
    trjdot_frames_t and trjdot_frames_outer, every operand at an element offset."""
    rng = np.random.default_rng(21)
    T, N, n_cg = 1037, 45, 13
    p = frames(T, N, dt, 1)
    fac = rng.standard_normal((T, n_cg, N)).astype(dt)
    tr = rng.standard_normal((T, n_cg, 3)).astype(dt)
    g = rng.standard_normal((T, n_cg, 3)).astype(dt)
    P, Fa, Tr, Gg = (x.astype(F64) for x in (p, fac, tr, g))
    tol = TOL[dt]
    for k in OFFSETS[dt]:
        args = [placed(x, k)[0] for x in (p, fac, tr, g)]
        al = [aligned(x) for x in (p, fac, tr, g)]
        out = same_route(lambda a, b: K.trjdot_frames(a, b), args[:2], al[:2], "trjdot_frames_kernel")
        close(out, np.matmul(Fa, P), np.matmul(np.abs(Fa), np.abs(P)), tol, f"trjdot_frames +{k}")
        out = same_route(K.trjdot_frames, args[:3], al[:3], "trjdot_frames_kernel")
        close(out, np.matmul(Fa, P) + Tr, np.matmul(np.abs(Fa), np.abs(P)) + np.abs(Tr), tol, f"trjdot_frames+t +{k}")
        out = same_route(lambda a, b: K.trjdot_cross(a, b, TD[dt]), (args[0], args[3]), (al[0], al[3]), "trjdot_cross")
        close(out, np.tensordot(P, Gg, axes=([0, 2], [0, 2])),
              np.tensordot(np.abs(P), np.abs(Gg), axes=([0, 2], [0, 2])), tol, f"trjdot_cross +{k}")
        out = same_route(lambda a, b: K.trjdot_frames_t(a, b, TD[dt]), (args[3], args[1]), (al[3], al[1]),
                         "trjdot_frames_t_kernel")
        close(out, np.einsum("tca,tcd->tad", Fa, Gg), np.einsum("tca,tcd->tad", np.abs(Fa), np.abs(Gg)), tol,
              f"trjdot_frames_t +{k}")
        out = same_route(lambda a, b: K.trjdot_frames_outer(a, b, TD[dt]), (args[3], args[0]), (al[3], al[0]),
                         "trjdot_frames_outer_kernel")
        close(out, np.einsum("tcd,tad->tca", Gg, P), np.einsum("tcd,tad->tca", np.abs(Gg), np.abs(P)), tol,
              f"trjdot_frames_outer +{k}")


@pytest.mark.parametrize("dt", [F32, F64])
def test_mapval_kernels_at_offsets(dt):
    """K7: gauss_pair_forces (forces and energies), gauss_proj, gauss_shift and dot, every input at an element offset,
    against tests/mapval_ref.py with its L1 scales."""
    rng = np.random.default_rng(31)
    T, n = 53, 67
    X = (10.0 * rng.random((T, n, 3))).astype(dt)
    Fo = rng.standard_normal((T, n, 3)).astype(dt)
    offs = np.array([45.0, 60.0, 80.0])
    width = 30.0
    tol = 1e-3 if dt == F32 else 1e-11
    floor = 1e-30 if dt == F32 else 1e-300
    Xd, Fd = X.astype(F64), Fo.astype(F64)
    Gr, Gs = mv.forces(Xd, offs[0], width, scale=True)
    Er = mv.literal_energies(Xd, offs[0], width)
    proj = [mv.proj_terms(Xd, Fd, o, width) for o in offs]
    gsq = [mv.forces(Xd, o, width, scale=True) for o in offs]
    od = torch.from_numpy(offs).cuda()
    for k in OFFSETS[dt]:
        x, f = placed(X, k)[0], placed(Fo, k)[0]
        xa, fa = aligned(X), aligned(Fo)
        G, E = same_route(lambda a: K.gauss_pair_forces(a, offs[0], width, want_energies=True), (x,), (xa,),
                          "gauss_site_forces_kernel")
        assert np.all(np.abs(host(G) - Gr) <= tol * Gs + floor) and np.all(np.abs(host(E) - Er) <= tol * Er + floor), k
        P = host(same_route(lambda a, b: K.gauss_proj(a, b, od, width), (x, f), (xa, fa), "gauss_proj_kernel"))
        for s, (v, l1) in enumerate(proj):
            assert abs(P[s] - v) <= tol * l1, (k, s)
        ip, sq = same_route(lambda a, b: K.gauss_shift(a, b, od, width), (x, f), (xa, fa), "gauss_shift_kernel")
        for s, ((v, l1), (g, gs)) in enumerate(zip(proj, gsq)):
            assert abs(host(ip)[s] - v) <= tol * l1 and abs(host(sq)[s] - (g * g).sum()) <= tol * (gs * gs).sum(), (k, s)
        d = same_route(K.dot, (x, f), (xa, fa), "dot_kernel")
        assert abs(float(d.item()) - float((Xd * Fd).sum())) <= 1e-12 * float(np.abs(Xd * Fd).sum()), k


@pytest.mark.parametrize("dt", [F32, F64])
def test_sumsq_take_frames_concat_scale_at_offsets(dt):
    """sumsq, take_frames, concat_sites and scale on inputs at element offsets (sumsq then runs its scalar path:
    its value is pinned here, not its speed)."""
    T, N = 2111, 37
    a = frames(T, N, dt, 41, 3.0)
    b = frames(T, 5, dt, 42, 3.0)
    idx = np.array([0, T - 1, 5, 5, 1000, T - 2])
    A = a.astype(F64)
    for k in OFFSETS[dt]:
        x, y = placed(a, k)[0], placed(b, k)[0]
        s = same_route(K.sumsq, (x,), (aligned(a),), "sumsq_kernel")
        assert abs(float(s.item()) - float((A * A).sum())) <= 1e-13 * float((A * A).sum()), k
        out = same_route(lambda v: K.take_frames(v, idx), (x,), (aligned(a),), "take_frames_kernel")
        assert np.array_equal(out.cpu().numpy(), a[idx]), k
        out = same_route(K.concat_sites, (x, y), (aligned(a), aligned(b)), "concat_sites_kernel")
        assert np.array_equal(out.cpu().numpy(), np.concatenate([a, b], axis=1)), k
        out = same_route(lambda v: K.scale(v, -2.5), (x,), (aligned(a),), "scale_kernel")
        assert np.array_equal(out.cpu().numpy(), (dt(-2.5) * a).astype(dt)), k


# ------------------------------------------------------------------ end to end on offset views
@pytest.mark.parametrize("dt", [F32, F64])
def test_maps_and_project_forces_on_offset_views(dt):
    """LinearMap, JLinearMap with a backward pass, and project_forces on offset views give what they give on
    contiguous copies (to rounding), and leave their inputs -- and the memory around them -- as they were."""
    T, N, n_cg = 2001, 175, 10
    rng = np.random.default_rng(51)
    f = frames(T, N, dt, 52, 20.0)
    c = (rng.random((T, N, 3)) * 5 + np.arange(N)[None, :, None] * 1.5).astype(dt)
    dense = np.zeros((n_cg, N))
    for i in range(n_cg):
        dense[i, i * 17:(i + 1) * 17] = rng.random(17)
    tol = 1e-12 if dt == F64 else 1e-5
    cons = {frozenset([3 * i, 3 * i + 1]) for i in range(N // 3)}
    for k in OFFSETS[dt][1:]:
        fv, fbuf = placed(f, k)
        cv, cbuf = placed(c, k)
        before = bits(fbuf), bits(cbuf)
        for lm in (LinearMap(dense), LinearMap(dense.astype(F32)), LinearMap([[i * 17] for i in range(n_cg)], n_fg_sites=N)):
            want = host(lm(aligned(f)))
            got = host(lm(fv))
            assert np.max(np.abs(got - want)) <= tol * np.max(np.abs(want)), k
        # JLinearMap forward and backward: the gradient reaches the offset view's own allocation
        jl = JLinearMap(dense)
        w = torch.from_numpy(rng.standard_normal((T, n_cg, 3))).cuda()
        lead = (fv.data_ptr() - fbuf.data_ptr()) // fv.element_size()
        grads = []
        for src, at in ((fbuf, lead), (aligned(f).reshape(-1), 0)):
            leaf = src.detach().clone().requires_grad_()
            view = leaf[at:at + f.size].view(f.shape)
            assert (view.data_ptr() % 16 != 0) == (at != 0)
            out = jl(view)
            (out * w.to(out.dtype)).sum().backward()
            grads.append((host(out), host(leaf.grad[at:at + f.size].view(f.shape))))
        (o1, g1), (o2, g2) = grads
        assert np.max(np.abs(o1 - o2)) <= tol * np.max(np.abs(o2)) and np.max(np.abs(g1 - g2)) <= tol * np.max(np.abs(g2))
        cmap = LinearMap([[i * 17] for i in range(n_cg)], n_fg_sites=N)
        a = project_forces(coords=cv, forces=fv, coord_map=cmap, constrained_inds=cons, l2_regularization=1e-3)
        b = project_forces(coords=aligned(c), forces=aligned(f), coord_map=cmap, constrained_inds=cons,
                           l2_regularization=1e-3)
        for key in ("mapped_coords", "mapped_forces"):
            x, y = host(K.as_device(a[key])), host(K.as_device(b[key]))
            assert np.max(np.abs(x - y)) <= (1e-10 if dt == F64 else 1e-4) * np.max(np.abs(y)), (k, key)
        assert abs(a["residual"] - b["residual"]) <= 1e-8 * abs(b["residual"])
        torch.cuda.synchronize()
        assert torch.equal(bits(fbuf), before[0]) and torch.equal(bits(cbuf), before[1]), k


# ------------------------------------------------------------------ special values: has_nan
NAN_COUNTS = [1, 3, 15, 16, 17, 4095, 4097, 2**20 + 3]


def nan_sites(n):
    """Index 0, the last index, and the positions around the 256-thread, 1024-element and 4096-element steps and the
    tail of the array."""
    cand = {0, n - 1, n - 2, n - 3, n - 4, n // 2}
    for step in (64, 256, 1024, 4096, 65536):
        for base in range(step, n, step) if n <= 4 * step else (step, (n // step) * step):
            cand |= {base - 1, base, base + 1}
    return sorted(i for i in cand if 0 <= i < n)


@pytest.mark.parametrize("dt", [F32, F64])
def test_has_nan_finds_one_nan_anywhere(dt):
    rng = np.random.default_rng(61)
    for n in NAN_COUNTS:
        x = rng.standard_normal(n).astype(dt)
        x[rng.integers(0, n, size=min(n, 3))] = np.inf
        x[rng.integers(0, n, size=min(n, 3))] = -np.inf
        x[rng.integers(0, n, size=min(n, 3))] = -0.0
        t = aligned(x)
        assert not K.has_nan(t), n
        for k in OFFSETS[dt][:1]:
            assert not K.has_nan(placed(x, k)[0][: n]), (n, k)
        for i in nan_sites(n):
            t[i] = float("nan")
            assert K.has_nan(t), (n, i)
            t[i] = float(x[i])
        assert not K.has_nan(t), n


# ------------------------------------------------------------------ special values: allclose
def allclose_table(dt):
    fi = np.finfo(dt)
    return [(1.0, np.inf), (np.inf, 1.0), (np.inf, np.inf), (np.inf, -np.inf), (-np.inf, np.inf), (np.nan, np.nan),
            (1.0, np.nan), (np.nan, 1.0), (-0.0, 0.0), (float(fi.max), np.inf), (-float(fi.max), -np.inf),
            (float(fi.smallest_subnormal), 0.0), (1.0, 1.0 + 1e-5), (1.0 + 1e-5, 1.0), (1.0, 1.0 + 3e-5)]


@pytest.mark.parametrize("dt", [F32, F64])
def test_allclose_matches_numpy_on_special_values(dt):
    """K.allclose against np.allclose (equal_nan=False): each pair planted once, alone, at the start, the middle and
    the end of otherwise equal arrays of 2^20 + 3 elements."""
    n = 2**20 + 3
    base = np.random.default_rng(71).standard_normal(n).astype(dt)
    a_t, b_t = aligned(base), aligned(base)
    assert K.allclose(a_t, b_t)
    for x, y in allclose_table(dt):
        xv, yv = dt(x), dt(y)
        # (the kernel compares the stored values in float64)
        want = bool(np.isclose(F64(xv), F64(yv), rtol=1e-5, atol=1e-8, equal_nan=False))
        for i in (0, n // 2 + 1, n - 1):
            a_t[i], b_t[i] = float(xv), float(yv)
            assert K.allclose(a_t, b_t) == want, (x, y, i, want)
            a_t[i], b_t[i] = float(base[i]), float(base[i])
    assert K.allclose(a_t, b_t)


# ------------------------------------------------------------------ special values: sumsq
def sumsq_counts(dt):
    """Counts on either side of one 256-piece chunk (a piece: 16 bytes), of the grid's first sweep (1024 chunks) and
    of the four-chunk unroll (4 x 1024 chunks), with ragged ends (aggf_util.hip: sumsq_kernel)."""
    v = 16 // np.dtype(dt).itemsize
    ch, g = 256 * v, 1024
    return [1, v - 1, ch - 1, ch, ch + 1, ch + v + 1, g * ch - 1, g * ch + 3, (4 * g - 1) * ch + 1, 4 * g * ch - 1,
            4 * g * ch, 4 * g * ch + 1, (4 * g + 1) * ch + v + 3]


@pytest.mark.parametrize("dt", [F32, F64])
def test_sumsq_on_special_values_and_chunk_edges(dt):
    """sumsq around the 256-piece chunk and the four-chunk unroll of aligned arrays (and on an offset view), its sum
    in float64 of float64 squares: any inf gives inf, any NaN NaN, float32 values of 1e20 a finite n * 1e40, float32
    subnormals NumPy's nonzero sum."""
    rng = np.random.default_rng(81)
    for n in sumsq_counts(dt):
        x = rng.standard_normal(n).astype(dt)
        xd = x.astype(F64)
        want = float((xd * xd).sum())
        for t in (aligned(x), placed(x, 1)[0]):
            assert abs(float(K.sumsq(t).item()) - want) <= 1e-11 * want, n
        t = aligned(x)
        for i in sorted({0, n // 2, n - 1}):
            t[i] = float("inf")
            assert float(K.sumsq(t).item()) == np.inf, (n, i)
            t[i] = float("-inf")
            assert float(K.sumsq(t).item()) == np.inf, (n, i)
            t[i] = float("nan")
            assert np.isnan(float(K.sumsq(t).item())), (n, i)
            t[i] = float(x[i])
    for n in (1, 1023, 4097):
        big = np.full(n, 1e20, dtype=dt)
        s = float(K.sumsq(aligned(big)).item())
        assert np.isfinite(s) and abs(s - n * float(big[0]) ** 2) <= 1e-13 * n * float(big[0]) ** 2, n
        if dt == F32:
            tiny = (np.arange(1, n + 1) % 7 + 1).astype(F32) * np.finfo(F32).smallest_subnormal
            want = float((tiny.astype(F64) ** 2).sum())
            assert want > 0
            assert float(K.sumsq(aligned(tiny)).item()) == pytest.approx(want, rel=1e-12), n


# ------------------------------------------------------------------ NaN policy end to end
def policy_ref(points, mat, fill, thr=1e-6):
    """The reference's NaN policy (map/core.py:219-237 with fill -1; jaxlinearmap.py:15-40 / 95-115 with fill 1) in
    NumPy, in the result dtype: the NaN->0 product, or ValueError."""
    dt = np.result_type(points.dtype, mat.dtype)
    if not np.isnan(points).any():
        return np.matmul(mat.astype(dt), points.astype(dt))
    raw = np.where(np.isnan(points), 0.0, points).astype(dt)
    pushed = np.where(np.isnan(points), fill, points).astype(dt)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.matmul(mat.astype(dt), raw)
        p = np.matmul(mat.astype(dt), pushed)
        if not np.allclose(r, p, atol=thr):
            raise ValueError("depends on NaN positions")
    return r


def check_policy(call, points, mat, fill, tol, what):
    try:
        want = policy_ref(points, mat, fill)
    except ValueError:
        with pytest.raises(ValueError):
            call()
        return
    got = host(call())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what
    fin = np.isfinite(want)
    bound = np.matmul(np.abs(mat.astype(F64)), np.abs(np.nan_to_num(points.astype(F64))))
    close(got[fin], want[fin].astype(F64), bound[fin], tol, what)


@pytest.mark.parametrize("pdt,mdt", [(F32, F64), (F64, F64), (F32, F32)])
def test_nan_policy_at_stage_edges(pdt, mdt):
    """One NaN at the first atom, the last atom, inside the ragged last 16-atom stage and in the last frame of a ragged
    frame stage, for dense maps of the few-site, 17-64-site and wide routes and for one-hot maps: with the NaN's
    column of the map zeroed the result is the NaN->0 product, otherwise ValueError -- as the reference decides."""
    T, N = 1001, 100
    rng = np.random.default_rng(91)
    pts = frames(T, N, pdt, 92, 5.0)
    tol = TOL[F32] if F32 in (pdt, mdt) else TOL[F64]
    for t, a, d in ((0, 0, 0), (500, N - 1, 2), (T - 1, 97, 1), (T - 1, 50, 0)):
        bad = pts.copy()
        bad[t, a, d] = np.nan
        for n_cg in (5, 20, 70):
            mat = rng.standard_normal((n_cg, N)).astype(mdt)
            for zero_col in (False, True):
                m = mat.copy()
                if zero_col:
                    m[:, a] = 0.0
                for cls, fill in ((LinearMap, -1.0), (JLinearMap, 1.0)):
                    check_policy(lambda: cls(m)(aligned(bad)), bad, m, fill, tol, (cls.__name__, t, a, n_cg, zero_col))
        for sel in ([a, (a + 7) % N], [(a + 1) % N, (a + 7) % N]):
            m = np.zeros((2, N))
            m[0, sel[0]] = m[1, sel[1]] = 1.0
            onehot = LinearMap([[s] for s in sel], n_fg_sites=N)
            check_policy(lambda: onehot(aligned(bad)), bad, m, -1.0, 0.0, ("one-hot", t, a, sel))


@pytest.mark.parametrize("cls,fill", [(LinearMap, -1.0), (JLinearMap, 1.0)])
def test_nan_policy_when_the_pushed_product_overflows(cls, fill):
    """float32 map and frames: the NaN->0 product is finite, the NaN->fill product overflows to infinity at one entry.
    np.allclose calls them not close, so the reference raises ValueError; an allclose that lets inf match a finite
    value (inf <= inf) would return the NaN->0 product instead."""
    T, N, n_cg = 70, 40, 3
    rng = np.random.default_rng(95)
    pts = (0.01 * rng.standard_normal((T, N, 3))).astype(F32)
    pts[:, 0, :] = 1.0
    pts[:, 7, :] = 0.0
    pts[T - 1, 7, 1] = np.nan
    mat = (0.01 * rng.standard_normal((n_cg, N))).astype(F32)
    mat[0, 0] = 3e38
    mat[0, 7] = 1e38 * fill  # NaN->fill gives 3e38 + 1e38: inf in float32; NaN->0 gives 3e38
    mat[1:, 7] = 0.0  # the overflow is the only difference between the two products
    with pytest.raises(ValueError):
        policy_ref(pts, mat, fill)
    check_policy(lambda: cls(mat)(aligned(pts)), pts, mat, fill, TOL[F32], "overflow")
    # the same NaN where the map's column is zero: no dependence, the NaN->0 product
    m = mat.copy()
    m[:, 7] = 0.0
    check_policy(lambda: cls(m)(aligned(pts)), pts, m, fill, TOL[F32], "zero column")
