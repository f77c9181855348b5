"""The nearest image of a triclinic cell on the GPU (``Cell(vectors, images="nearest")``): the nearest-image forms of
K9c / K9d (pairlist_pbc_kernel<.., 3>, pairlist_pull_pbc_kernel<.., 3>), K9e (pairmin_kernel<.., true, 3>) and K7
(gauss_site_forces_kernel<.., true, 3>, gauss_proj_kernel<.., true, 3>, gauss_shift_kernel<.., true, 3>) -- every
instantiation launched and checked by name.

1. Against the float64 reference (tests/nearest_ref.py) in a rhombic dodecahedron and a truncated octahedron, one cell
   or one per frame, with the helpers and tolerances of the triclinic tests of the same kernels (tests/test_gpu_cell.py:
   ``close``, ``TOL``; tests/test_gpu_mapval_pbc.py: 1e-11 / 1e-3 of the L1 scale).  The inputs are those of
   tests/nearest_ref.py, whose conditions tests/test_nearest_host.py asserts: at least 5 % of the elements have a
   nearest image that is not the brick image (a fallback to the brick form fails), and the few elements within 1e-3 of
   a tie between two candidates are left out (their weights are zero where they enter a sum; the K7 inputs have none).
2. Bit for bit on dyadic inputs: sites each moved by their own lattice vectors give, under the nearest form, what the
   OPEN kernels give on the unmoved sites -- every candidate's squared length is exact in float32.
3. Bit for bit in K9c / K9d / K9e: a diagonal cell gives the box form's results, sites within the safe radius the
   triclinic form's.  (Not K7: the products of its sums are fused as the compiler chooses per instantiation -- the
   brick form of the projection kernel computes fma(d1, e1, d0 e0), the nearest form fma(d0, e0, d1 e1) -- so equal
   images give sums equal to rounding only; K7 is pinned bit for bit by the dyadic inputs of 2.)
4. Gradients against the host body, bad frames, a cell on the GPU, the caller's stream, the public functions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cell_ref as R  # noqa: E402
import mapval_ref as mref  # noqa: E402
import nearest_ref as N  # noqa: E402
import stream_gate as SG  # noqa: E402
import test_gpu_pairlist as base  # noqa: E402  (close, TOL, dev, host, reset, force_matching)
from aggforce_amd import Cell, guess_pairwise_constraints  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd import _lib  # noqa: E402
from aggforce_amd import jaxmapval as mv  # noqa: E402
from aggforce_amd import pbc  # noqa: E402
from aggforce_amd.jaxutil import PairList, distances_in_box, min_distances, pair_distances  # noqa: E402
from pairlist_ref import pull_reference, random_list, triangle  # noqa: E402
from pbc_ref import frame_boxes  # noqa: E402

DEV = base.DEV
F32, F64 = torch.float32, torch.float64
TOL, NAME, LANE_DEG = base.TOL, base.NAME, base.LANE_DEG
MV_TOL = {F64: 1e-11, F32: 1e-3}  # tests/test_gpu_mapval_pbc.py
NP = {F32: np.float32, F64: np.float64}
dev, host, close, reset = base.dev, base.host, base.close, base.reset
T = N.GPU_T

# (name, pairs, m or None for the self form, n): 171 pairs and 2415 / 300 pairs -- either side of a 256-thread block;
# triangle70 and cross have sites with more than 32 entries (the wave form of K9d), triangle19 has 18 (the lane form)
CASES = [("triangle19", triangle(19), None, 19), ("triangle70", triangle(70), None, 70),
         ("cross", random_list(300, 6, 11, 300, self_form=False), 6, 11)]
CASE_IDS = [c[0] for c in CASES]
CELLS = [(kind, per_frame) for kind in N.GPU_KINDS for per_frame in (False, True)]
CELL_IDS = [f"{kind}-{'cell_per_frame' if pf else 'one_cell'}" for kind, pf in CELLS]


def launched():
    """Names of the kernels launched since the last reset, without return type and namespace."""
    torch.cuda.synchronize()
    return sorted(p.split("(")[0].replace("void ", "").replace("aggf::", "")
                  for p, c in _lib.coverage(names=True).values() if c > 0)


def rows(H, dtype, frames=T):
    """The (T, 9) device rows of a cell H ((3, 3) or (T, 3, 3)) in ``dtype``: what the kernel wrappers take."""
    return dev(np.ascontiguousarray(np.broadcast_to(H, (frames, 3, 3))).reshape(frames, 9), dtype).contiguous()


def near_cell(H):
    return Cell(H, images="nearest")


def close_kept(got, ref, bound, keep, tol, what):
    """``close`` on the elements of ``keep`` (the others sit on a tie between two candidates)."""
    k = torch.as_tensor(keep, device=got.device)
    close(got[k], ref[keep], bound[keep], tol, what)


def pull_names(pl, ind, outd, dv):
    forms = {int(deg > LANE_DEG) for _, _, deg in pl.tables()}
    return sorted(f"pairlist_pull_pbc_kernel<{NAME[ind]}, {NAME[outd]}, {'true' if dv else 'false'}, {f}, 3>" for f in forms)


def test_the_cases_reach_both_forms_of_the_pull_kernel_and_both_sides_of_a_block():
    degs = {name: [deg for _, _, deg in PairList(pairs, n, m).tables()] for name, pairs, m, n in CASES}
    assert max(degs["triangle19"]) <= LANE_DEG < min(degs["triangle70"]) and max(degs["cross"]) > LANE_DEG
    assert len(CASES[0][1]) < 256 < len(CASES[2][1]) < len(CASES[1][1])


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,per_frame", CELLS, ids=CELL_IDS)
def test_k9c_nearest_form_every_mode_matches_the_reference(case, dtype, kind, per_frame):
    _, pairs, m, n = case
    H, xn, cn, raw, tie = N.list_case(kind, per_frame, pairs, m, n, dtype)
    keep = ~tie
    tab = PairList(pairs, n, m).on(DEV)
    x = dev(xn, dtype)
    c = x if m is None else dev(cn, dtype)
    rng = np.random.default_rng(len(pairs))
    v = dev(rng.standard_normal((T, n, 3)), dtype)
    y = v if m is None else dev(rng.standard_normal((T, m, 3)), dtype)
    g = host(v)[:, pairs[:, 1]] - host(y)[:, pairs[:, 0]]
    u, b = N.wrap(raw, H), N.comp_bound(raw, H)
    sq, bsq = (u * u).sum(-1), (b * b).sum(-1)
    cell = rows(H, dtype)
    reset()
    d = K.pair_list_dist(x, c, tab, K.PAIR_DIST, box=cell, near=True)
    s = K.pair_list_dist(x, c, tab, K.PAIR_SQDIST, box=cell, near=True)
    o = K.pair_list_dist(x, c, tab, K.PAIR_DOT, v, y, box=cell, near=True)
    assert launched() == [f"pairlist_pbc_kernel<{NAME[dtype]}, {mode}, 3>" for mode in (0, 1, 2)]
    for got in (d, s, o):
        assert got.dtype == dtype and tuple(got.shape) == (T, len(pairs)) and bool(torch.isfinite(got).all())
    close_kept(d, np.sqrt(sq), np.sqrt(bsq), keep, TOL[dtype], "K9c nearest DIST")
    close_kept(s, sq, bsq, keep, TOL[dtype], "K9c nearest SQDIST")
    close_kept(o, (g * u).sum(-1), (np.abs(g) * b).sum(-1), keep, TOL[dtype], "K9c nearest DOT")
    for again in (K.pair_list_dist(x, c, tab, K.PAIR_DIST, box=cell, near=True),
                  pair_distances(x, PairList(pairs, n, m), None if m is None else c, box=near_cell(H))):
        assert torch.equal(again, d)  # a repeat, and the public function from a Cell on the host
    # the brick form gives other numbers on these inputs
    brick = K.pair_list_dist(x, c, tab, K.PAIR_DIST, box=cell)
    assert float(((brick - d) > 1e-3).double().mean()) >= 0.05 and bool((brick >= d * (1 - 1e-5)).all())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("ind,outd", [(F32, F32), (F64, F64), (F64, F32)], ids=["f32", "f64", "f64-f32"])
@pytest.mark.parametrize("kind,per_frame", CELLS, ids=CELL_IDS)
def test_k9d_nearest_form_both_sums_match_the_reference_and_repeat_bit_for_bit(case, ind, outd, kind, per_frame):
    _, pairs, m, n = case
    H, xn, cn, raw, tie = N.list_case(kind, per_frame, pairs, m, n, ind)
    pl = PairList(pairs, n, m)
    tab = pl.on(DEV)
    nrows = n if m is None else m
    tol = max(TOL[ind], TOL[outd])
    x = dev(xn, ind)
    c = x if m is None else dev(cn, ind)
    wn = N.stored(np.random.default_rng(len(pairs) + 2).standard_normal((T, len(pairs))), ind)
    wn[tie] = 0.0  # an element on a tie adds nothing, whichever image it takes
    w = dev(wn, ind)
    u, b = N.wrap(raw, H), N.comp_bound(raw, H)
    cell = rows(H, ind)

    def bounds(weights):
        ab, bb, _, _ = pull_reference(np.abs(weights), b, pairs, nrows, n)
        return ab, -bb

    a_ref, b_ref, _, _ = pull_reference(wn, u, pairs, nrows, n)
    a_bnd, b_bnd = bounds(wn)
    reset()
    a, bsum = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=cell, near=True)
    assert launched() == pull_names(pl, ind, outd, False)
    assert a.dtype == outd and bsum.dtype == outd and tuple(a.shape) == (T, n, 3) and tuple(bsum.shape) == (T, nrows, 3)
    close(a, a_ref, a_bnd, tol, "K9d nearest A")
    close(bsum, b_ref, b_bnd, tol, "K9d nearest B")
    a2, b2 = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=cell, near=True)
    assert torch.equal(a, a2) and torch.equal(bsum, b2)
    a1, none = K.pair_list_pull(w, x, c, tab, want_b=False, out_dtype=outd, box=cell, near=True)
    assert none is None and torch.equal(a1, a)
    # the distance form: w / dv where dv > 0, else 0
    dv = K.pair_list_dist(x, c, tab, K.PAIR_DIST, box=cell, near=True)
    dvn = host(dv)
    wq = np.where(dvn > 0, wn / np.where(dvn > 0, dvn, 1.0), 0.0)
    a_ref, b_ref, _, _ = pull_reference(wq, u, pairs, nrows, n)
    a_bnd, b_bnd = bounds(wq)
    reset()
    a, bsum = K.pair_list_pull(w, x, c, tab, dv=dv, out_dtype=outd, box=cell, near=True)
    assert launched() == pull_names(pl, ind, outd, True)
    assert torch.isfinite(a).all() and torch.isfinite(bsum).all()
    close(a, a_ref, a_bnd, tol, "K9d nearest A (Dv)")
    close(bsum, b_ref, b_bnd, tol, "K9d nearest B (Dv)")
    a2, b2 = K.pair_list_pull(w, x, c, tab, dv=dv, out_dtype=outd, box=cell, near=True)
    assert torch.equal(a, a2) and torch.equal(bsum, b2)


def pairmin_names(dtype, split):
    return sorted([f"pairmin_kernel<{NAME[dtype]}, true, 3>"] + ([f"pairmin_reduce_kernel<{NAME[dtype]}>"] if split else []))


@pytest.mark.parametrize("frames,m,n,split", [(T, 11, 70, False), (T, None, 19, False), (200, 3, 7, True)])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,per_frame", CELLS, ids=CELL_IDS)
def test_min_distances_under_a_nearest_cell_match_the_reference_and_the_list_kernels(frames, m, n, split, dtype, kind, per_frame):
    H, xn, cn, raw, tie = N.matrix_case(kind, per_frame, m, n, dtype, T=frames)
    rows_m = n if m is None else m
    x = dev(xn, dtype)
    c = x if m is None else dev(cn, dtype)
    u, b = N.wrap(raw, H), N.comp_bound(raw, H)
    dist = np.linalg.norm(u, axis=-1)
    arg = dist.argmin(0)
    ref = np.take_along_axis(dist, arg[None], 0)[0]
    bnd = np.take_along_axis(np.linalg.norm(b, axis=-1), arg[None], 0)[0]
    # a pair is left out if a frame on a tie could be its minimum: the two readings of such a frame differ by less than
    # 1e-3 in squared length, so a frame further than that above the minimum is not the minimum under either
    keep = ~(tie & (dist <= ref[None] * (1 + 2 * N.TIE))).any(axis=0)
    assert keep.mean() >= 0.98
    if split:
        assert _lib.load().aggf_pair_min_workspace_bytes(frames, rows_m, n, K.dtype_code(dtype)) // (rows_m * n * x.element_size()) == 4
    for square in (False, True):
        reset()
        got = min_distances(x, None if m is None else c, square=square, box=near_cell(H))
        assert launched() == pairmin_names(dtype, split)
        assert tuple(got.shape) == (rows_m, n) and got.dtype == dtype and not got.requires_grad
        close_kept(got, ref * ref if square else ref, bnd * bnd if square else bnd, keep, TOL[dtype],
                   f"K9e nearest square={square}")
        flat = pair_distances(x, PairList.all_pairs(n, m), None if m is None else c, square=square, box=near_cell(H))
        assert torch.equal(got, flat.amin(0).reshape(rows_m, n))
    own = min_distances(x, box=near_cell(dev(np.broadcast_to(H, (frames, 3, 3)).copy())))  # (a cell on the GPU)
    assert (own.diagonal() == 0).all()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,per_frame", CELLS, ids=CELL_IDS)
def test_from_cutoff_between_the_two_radii_is_the_reference_list(dtype, kind, per_frame):
    n = 30
    H = N.gpu_cell(kind, per_frame, dtype)
    Hs = np.broadcast_to(H, (T, 3, 3))
    # sites that keep their places (0.1 of noise per frame): the minima over the frames spread over the whole cell
    rng = np.random.default_rng(61)
    places = np.einsum("nk,tkj->tnj", rng.random((n, 3)), Hs) + 0.1 * rng.standard_normal((T, n, 3))
    xn = N.stored(R.wrap_positions(places, H), dtype)
    i, j = np.triu_indices(n, 1)
    true = np.min([R.brute_min(xn[t][j] - xn[t][i], Hs[t])[1] for t in range(T)], axis=0)  # the TRUE minimum image
    r_safe, r_img = R.safe_radius(H), N.image_radius(H)
    v = np.sort(true[(true >= r_safe + 0.5 * (r_img - r_safe)) & (true <= r_img)])
    k = int(np.argmax(np.diff(v)))
    cut = float(0.5 * (v[k] + v[k + 1]))
    assert r_safe * 1.1 < cut <= r_img and np.min(np.abs(true - cut)) > 2e-3 * cut  # no minimum within 2e-3 of the cutoff
    want = [(a, b) for a, b, d in zip(i, j, true) if d <= cut]
    ref = np.linalg.norm(N.wrap(xn[:, j] - xn[:, i], H), axis=-1).min(0)
    assert want == [(a, b) for a, b, d in zip(i, j, ref) if d <= cut]  # the reference's list
    brick = np.linalg.norm(R.wrap(xn[:, j] - xn[:, i], H), axis=-1).min(0)
    assert len(want) > sum(brick <= cut) and 20 < len(want) < len(i)  # the brick form misses pairs
    x = dev(xn, dtype)
    reset()
    pl = PairList.from_cutoff(x, cut, box=near_cell(H))
    assert launched() == pairmin_names(dtype, False)
    assert [tuple(p) for p in pl.pairs] == want
    assert [tuple(p) for p in PairList.from_cutoff(x, cut, box=near_cell(dev(Hs.copy()))).pairs] == want  # a cell on the GPU
    with pytest.raises(ValueError, match="safe radius"):
        PairList.from_cutoff(x, cut, box=Cell(H))
    PairList.from_cutoff(x, r_img, box=near_cell(H))
    with pytest.raises(ValueError, match="image radius"):
        PairList.from_cutoff(x, 1.0001 * r_img, box=near_cell(H))
    PairList.from_cutoff(x, 1.0001 * r_img, box=near_cell(dev(Hs.copy())))  # (on the GPU the condition is the caller's part)
    assert tuple(pair_distances(x, pl, box=near_cell(H)).shape) == (T, len(want))  # the list feeds the list kernels


_mv_cases = {}


def mv_case(kind, per_frame, dtype):
    """The K7 inputs of tests/nearest_ref.py and their references, computed once."""
    key = (kind, per_frame, dtype)
    if key not in _mv_cases:
        H, X, F, outer = N.mapval_case(kind, per_frame, dtype)
        kw = dict(inner=1.0, outer=outer, width=0.5)
        _mv_cases[key] = dict(H=H, X=X, F=F, kw=kw, proj=N.mv_random_force_proj(X, F, 37, 42, H=H, **kw),
                              shift=N.mv_random_residual_shift(X, F, 37, 42, H=H, **kw))
    return _mv_cases[key]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind,per_frame", CELLS, ids=CELL_IDS)
def test_k7_site_forces_projections_and_shifts_match_the_reference(kind, per_frame, dtype):
    c = mv_case(kind, per_frame, dtype)
    H, kw, tol, npdt = c["H"], c["kw"], MV_TOL[dtype], NP[dtype]
    X, F, box = c["X"].astype(npdt), c["F"].astype(npdt), near_cell(c["H"])
    assert R.safe_radius(H) < kw["outer"] < N.image_radius(H)
    floor = 1e-300 if dtype == F64 else 1e-30  # float32 exp2 results below the normal range lose bits
    offs, w = mref.offsets(42, 2, **kw)
    if dtype == F32:
        w = 5.0  # (tests/test_gpu_mapval_pbc.py: the narrow field is checked entry by entry in float64 alone)
    reset()
    for offset in offs:
        G, E = pbc.sq_gaussian_forces(X, offset, w, box), pbc.sq_gaussian_energies(X, offset, w, box)
        assert isinstance(G, np.ndarray) and G.dtype == npdt and E.dtype == npdt and E.shape == (T,)
        Gr, scale = N.mv_forces(c["X"], offset, w, H)
        Er = N.mv_energies(c["X"], offset, w, H)
        print(f"  forces {np.max(np.abs(G - Gr) / (scale + floor)):.3g}, energies {np.max(np.abs(E - Er) / Er):.3g} "
              f"of the scale (tolerance {tol:g})")
        assert scale.max() > 0
        assert np.all(np.abs(G - Gr) <= tol * scale + floor)
        assert np.all(np.abs(E - Er) <= tol * Er + floor)
    assert f"gauss_site_forces_kernel<{NAME[dtype]}, true, 3>" in launched()
    (Pr, Ps), (Rr, Rs) = c["proj"], c["shift"]
    assert Ps.max() > 0 and Rs.max() > 0  # the offsets met pairs
    reset()
    P = np.array(mv.random_force_proj(X, F, 37, np.random.default_rng(42), average=False, box=box, **kw))
    Rv = np.array(mv.random_residual_shift(X, F, 37, np.random.default_rng(42), box=box, **kw))
    names = launched()
    assert f"gauss_proj_kernel<{NAME[dtype]}, {NAME[dtype]}, true, 3>" in names
    assert f"gauss_shift_kernel<{NAME[dtype]}, {NAME[dtype]}, true, 3>" in names
    assert not any(k.endswith(", true>") for k in names)  # no brick form
    print(f"  proj {np.max(np.abs(P - Pr) / Ps):.3g}, shift {np.max(np.abs(Rv - Rr) / Rs):.3g} of the scale")
    assert np.all(np.abs(P - Pr) <= tol * Ps)
    assert np.all(np.abs(Rv - Rr) <= tol * Rs)
    # twice, from device tensors and a cell on the GPU: the same bits; the method of pbc takes the fused path
    Hd = near_cell(dev(np.broadcast_to(H, (T, 3, 3)).copy(), dtype))
    assert mv.random_force_proj(dev(X, dtype), dev(F, dtype), 37, np.random.default_rng(42), average=False, box=Hd,
                                method=pbc.rsqpg_forces, **kw) == list(P)
    # the brick form measures something else on these sites, and refuses this outer on the host
    Pb = np.array(mv.random_force_proj(X, F, 37, np.random.default_rng(42), average=False,
                                       box=Cell(dev(np.broadcast_to(H, (T, 3, 3)).copy(), dtype)), **kw))
    assert np.any(np.abs(Pb - Pr) > tol * Ps)
    with pytest.raises(ValueError, match="half the smallest box length"):
        mv.random_force_proj(X, F, 37, np.random.default_rng(42), average=False, box=Cell(H), **kw)
    G = pbc.rsqpg_forces(dev(X, dtype), randg=np.random.default_rng(1), box=box, **kw)
    offset = np.random.default_rng(1).random() * (kw["outer"] ** 2 - kw["inner"] ** 2) + kw["inner"] ** 2
    assert torch.equal(G, pbc.sq_gaussian_forces(dev(X, dtype), offset, kw["width"] ** 2, box))


# ------------------------------------------------------------------ 2. bit for bit on dyadic inputs
@pytest.mark.parametrize("n,cross", [(19, None), (70, None), (11, 6)], ids=["self19", "self70", "cross"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_dyadic_sites_moved_by_lattice_vectors_give_the_open_kernels_bits_in_k9c_k9d_k9e(dtype, n, cross):
    x0n, x1n, c0n, c1n, H = N.dyadic_case(T, n, 3, cross)
    pairs = triangle(n) if cross is None else random_list(300, cross, n, 300, self_form=False)
    pl = PairList(pairs, n, cross)
    tab = pl.on(DEV)
    x0, x1 = dev(x0n, dtype), dev(x1n, dtype)
    c0, c1 = (x0, x1) if cross is None else (dev(c0n, dtype), dev(c1n, dtype))
    assert torch.equal(x1.double().cpu(), torch.from_numpy(x1n))  # the moved sites are exact in this dtype
    rng = np.random.default_rng(n)
    v = dev(rng.standard_normal((T, n, 3)), dtype)
    y = v if cross is None else dev(rng.standard_normal((T, cross, 3)), dtype)
    w = dev(rng.standard_normal((T, len(pairs))), dtype)
    cell = rows(H, dtype)
    reset()
    for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
        got = K.pair_list_dist(x1, c1, tab, mode, v, y, box=cell, near=True)
        assert torch.equal(got, K.pair_list_dist(x0, c0, tab, mode, v, y)), mode
    dv = K.pair_list_dist(x0, c0, tab)
    for outd in ((F32,) if dtype == F32 else (F64, F32)):
        for kw in ({}, {"dv": dv}):
            a, b = K.pair_list_pull(w, x1, c1, tab, out_dtype=outd, box=cell, near=True, **kw)
            a0, b0 = K.pair_list_pull(w, x0, c0, tab, out_dtype=outd, **kw)
            assert torch.equal(a, a0) and torch.equal(b, b0), (outd, sorted(kw))
    for square in (False, True):
        assert torch.equal(K.pair_min(x1, c1, square, box=cell, near=True), K.pair_min(x0, c0, square))
    names = launched()
    form = int(max(deg for _, _, deg in pl.tables()) > LANE_DEG)
    for name in ([f"pairlist_pbc_kernel<{NAME[dtype]}, {mode}, 3>" for mode in (0, 1, 2)]
                 + [f"pairmin_kernel<{NAME[dtype]}, true, 3>"]
                 + [f"pairlist_pull_pbc_kernel<{NAME[dtype]}, {NAME[o]}, {d}, {form}, 3>"
                    for o in ((F32,) if dtype == F32 else (F64, F32)) for d in ("true", "false")]):
        assert name in names, name
    # the brick form does not recover the unmoved distances, nor do the open kernels on the moved sites
    open0 = K.pair_list_dist(x0, c0, tab)
    assert not torch.equal(K.pair_list_dist(x1, c1, tab, box=cell), open0)
    assert not torch.equal(K.pair_list_dist(x1, c1, tab), open0)
    # the public functions: distances_in_box from a Cell, and its gradient is the open one's
    xg0, xg1 = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
    if cross is None:
        d1 = distances_in_box(xg1, near_cell(H), return_matrix=False)
        d0 = pair_distances(xg0, PairList.upper_triangle(n))
        assert torch.equal(d1, d0)
        (g1,), (g0,) = torch.autograd.grad(d1.sum(), xg1), torch.autograd.grad(d0.sum(), xg0)
        assert torch.equal(g1, g0)


MV_PAIRS = [(F32, F32), (F32, F64), (F64, F32), (F64, F64)]


# (7, 19), (7, 70): several frames per workgroup and per LDS stage; (2, 1100): past the LDS tile and the 256-site block
MV_DYADIC = [(T, n, xd, fd) for n in (19, 70) for xd, fd in MV_PAIRS] + [(2, 1100, F32, F64)]


@pytest.mark.parametrize("frames,n,xd,fd", MV_DYADIC, ids=[f"{t}x{n}-{NAME[a]}-{NAME[b]}" for t, n, a, b in MV_DYADIC])
def test_dyadic_sites_moved_by_lattice_vectors_give_the_open_kernels_bits_in_k7(frames, n, xd, fd):
    x0n, x1n, _, _, H = N.dyadic_case(frames, n, 5)
    Fn = np.random.default_rng(n).integers(-512, 512, size=(frames, n, 3)) / 16.0
    Xo, Xm, Fd = dev(x0n, xd), dev(x1n, xd), dev(Fn, fd)
    box, cell = near_cell(H), rows(H, xd, frames)
    width = 4.0
    reset()
    for offset in (3.0, 8.5):
        G, E = pbc.sq_gaussian_forces(Xm, offset, width, box), pbc.sq_gaussian_energies(Xm, offset, width, box)
        assert torch.equal(G, mv.sq_gaussian_forces(Xo, offset, width)), (offset, "forces")
        assert torch.equal(E, mv.sq_gaussian_energies(Xo, offset, width)), (offset, "energies")
        assert bool(torch.isfinite(G).all()) and float(G.abs().max()) > 0
    for S in (1, 37, 1030):  # 1030: two offset chunks
        o = dev(np.random.default_rng(S).uniform(1.0, 10.0, S))
        assert torch.equal(K.gauss_proj(Xm, Fd, o, width, box=cell, near=True), K.gauss_proj(Xo, Fd, o, width)), S
        ip, gsq = K.gauss_shift(Xm, Fd, o, width, box=cell, near=True)
        ip0, gsq0 = K.gauss_shift(Xo, Fd, o, width)
        assert torch.equal(ip, ip0) and torch.equal(gsq, gsq0), S
        assert float(ip0.abs().max()) > 0 and float(gsq0.min()) > 0
    names = launched()
    for name in (f"gauss_site_forces_kernel<{NAME[xd]}, true, 3>", f"gauss_proj_kernel<{NAME[xd]}, {NAME[fd]}, true, 3>",
                 f"gauss_shift_kernel<{NAME[xd]}, {NAME[fd]}, true, 3>"):
        assert name in names, name
    # the brick form sees other distances on the moved sites
    assert not torch.equal(pbc.sq_gaussian_energies(Xm, 3.0, width, Cell(H)), mv.sq_gaussian_energies(Xo, 3.0, width))


# ------------------------------------------------------------------ 3. where the forms must agree bit for bit
def diagonal(L, frames):
    return np.stack([np.diag(l) for l in np.broadcast_to(L, (frames, 3))])


def assert_same_bits_as(x, c, v, y, w, tab, near_rows, other_box):
    """K9c / K9d / K9e under the nearest form of ``near_rows`` against the same calls with ``box=other_box``."""
    dtype = x.dtype
    for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
        assert torch.equal(K.pair_list_dist(x, c, tab, mode, v, y, box=near_rows, near=True),
                           K.pair_list_dist(x, c, tab, mode, v, y, box=other_box))
    dvs = K.pair_list_dist(x, c, tab, box=other_box)
    for outd in ((F32,) if dtype == F32 else (F64, F32)):
        for kw in ({}, {"dv": dvs}):
            a, b = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=near_rows, near=True, **kw)
            a0, b0 = K.pair_list_pull(w, x, c, tab, out_dtype=outd, box=other_box, **kw)
            assert torch.equal(a, a0) and torch.equal(b, b0)
    for square in (False, True):
        assert torch.equal(K.pair_min(x, c, square, box=near_rows, near=True), K.pair_min(x, c, square, box=other_box))


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_box", "box_per_frame"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_diagonal_cell_gives_the_box_forms_bits(dtype, per_frame):
    L = frame_boxes(T, 900) if per_frame else R.DIAG_LENGTHS
    for _, pairs, m, n in CASES[1:]:
        tab = PairList(pairs, n, m).on(DEV)
        x, c, v, y, w = base.list_operands(T, pairs, m, n, dtype)
        reset()
        assert_same_bits_as(x, c, v, y, w, tab, rows(diagonal(L, T), dtype), dev(L, dtype))
        names = launched()
        assert any(k.endswith(", 3>") for k in names) and any(not k.endswith(", 3>") for k in names)
        raw = host(x)[:, pairs[:, 1]] - host(c)[:, pairs[:, 0]]
        assert (np.abs(np.rint(raw / R.DIAG_LENGTHS)) >= 1).any()
    # the public functions from a Cell
    public = near_cell(diagonal(L, T) if per_frame else np.diag(L))
    assert public.image_radius == public.safe_radius
    assert torch.equal(min_distances(x, c, box=public), min_distances(x, c, box=L))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,per_frame", CELLS, ids=CELL_IDS)
def test_sites_within_the_safe_radius_give_the_triclinic_forms_bits(dtype, kind, per_frame):
    H = N.gpu_cell(kind, per_frame, dtype)
    Hf = np.broadcast_to(H, (T, 3, 3))
    r_safe = R.safe_radius(H)
    for _, pairs, m, n in CASES[1:]:
        rng = np.random.default_rng(n)

        def cluster(k):  # within a ball of diameter 0.9 r_safe, then moved by lattice vectors
            p = rng.standard_normal((T, k, 3))
            p *= 0.45 * r_safe * rng.random((T, k, 1)) ** (1 / 3) / np.linalg.norm(p, axis=-1, keepdims=True)
            return N.stored(p + np.einsum("tnk,tkj->tnj", rng.integers(-2, 3, (T, k, 3)).astype(np.float64), Hf), dtype)

        xn = cluster(n)
        cn = xn if m is None else cluster(m)
        raw = xn[:, pairs[:, 1]] - cn[:, pairs[:, 0]]
        assert np.linalg.norm(R.wrap(raw, H), axis=-1).max() < 0.95 * r_safe and np.abs(R.brick(raw, H)[1]).max() >= 2
        assert R.tie_distance(raw, H) > 1e-3  # (far inside the brick: no stage near a tie)
        x = dev(xn, dtype)
        c = x if m is None else dev(cn, dtype)
        v = dev(rng.standard_normal((T, n, 3)), dtype)
        y = v if m is None else dev(rng.standard_normal((T, m, 3)), dtype)
        w = dev(rng.standard_normal((T, len(pairs))), dtype)
        assert_same_bits_as(x, c, v, y, w, PairList(pairs, n, m).on(DEV), rows(H, dtype), rows(H, dtype))


# ------------------------------------------------------------------ 4. gradients, bad frames, a cell on the GPU
@pytest.mark.parametrize("frames,n", [(3, 5), (T, 19)])
@pytest.mark.parametrize("kind,per_frame", CELLS, ids=CELL_IDS)
def test_first_gradients_and_the_force_matching_double_backward_against_the_host_body(frames, n, kind, per_frame):
    H = N.gpu_cell(kind, per_frame, F64, T=frames)
    i, j = np.triu_indices(n, 1)
    # (the host body and the kernels round differently: keep every element 1e-6 away from a tie between two candidates)
    (xn,) = N.free_sites(lambda k: (N.spread_sites(frames, n, H, 600 + n + 31 * k),), lambda a: a[:, j] - a[:, i], H, F64,
                         nearest_margin=1e-6)
    assert (N.nearest(xn[:, j] - xn[:, i], H)[1] != 0).mean() >= 0.05
    reset()
    g, gg = base.force_matching(lambda z: distances_in_box(z, near_cell(H), return_matrix=False), dev(xn, grad=True))
    names = launched()
    assert "pairlist_pbc_kernel<double, 2, 3>" in names and "pairlist_pbc_kernel<double, 0, 3>" in names
    assert any(k.startswith("pairlist_pull_pbc_kernel") and k.endswith(", 3>") for k in names)
    assert not any(k.endswith(", 2>") or k.startswith(("pairdist_kernel", "pairpull_kernel")) for k in names)
    assert torch.isfinite(gg).all(), "non-finite double backward"
    g_ref, gg_ref = base.force_matching(lambda z: pair_distances(z, triangle(n), box=near_cell(H)),  # the host body
                                        torch.tensor(xn, requires_grad=True))
    torch.testing.assert_close(g.cpu(), g_ref, rtol=1e-10, atol=1e-9)
    torch.testing.assert_close(gg.cpu(), gg_ref, rtol=1e-10, atol=1e-9)
    # and they are not the brick form's
    g_brick, _ = base.force_matching(lambda z: distances_in_box(z, Cell(H), return_matrix=False), dev(xn, grad=True))
    assert not torch.allclose(g_brick, g, rtol=1e-6, atol=1e-6)


BAD = [("zero", (1, 1), 0.0), ("negative", (0, 0), -4.1), ("nan", (2, 2), float("nan")), ("inf", (1, 1), float("inf")),
       ("skew_nan", (2, 1), float("nan")), ("skew_inf", (1, 0), float("-inf"))]  # tests/test_gpu_cell.py's


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("bad", BAD, ids=[b[0] for b in BAD])
def test_a_bad_cell_in_one_frame_makes_that_frame_nan_and_leaves_the_others_exact(dtype, bad):
    _, (r, cidx), value = bad
    frames = 3
    H = N.gpu_cell("octahedron", True, dtype, T=frames)
    broken = H.copy()
    broken[1, r, cidx] = value
    good, bcell = rows(H, dtype, frames), rows(broken, dtype, frames)
    for pairs, n in ((triangle(70), 70), (triangle(5), 9)):  # (the second leaves sites without entries)
        tab = PairList(pairs, n).on(DEV)
        x = dev(N.spread_sites(frames, n, H, 91), dtype)
        rng = np.random.default_rng(n)
        v, w = dev(rng.standard_normal((frames, n, 3)), dtype), dev(rng.standard_normal((frames, len(pairs))), dtype)
        for mode in (K.PAIR_DIST, K.PAIR_SQDIST, K.PAIR_DOT):
            ref = K.pair_list_dist(x, x, tab, mode, v, v, box=good, near=True)
            got = K.pair_list_dist(x, x, tab, mode, v, v, box=bcell, near=True)
            assert torch.isnan(got[1]).all() and torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
            assert torch.isfinite(ref).all()
        for kw in ({}, {"dv": K.pair_list_dist(x, x, tab, box=good, near=True)}):
            ra, rb = K.pair_list_pull(w, x, x, tab, box=good, near=True, **kw)
            ga, gb = K.pair_list_pull(w, x, x, tab, box=bcell, near=True, **kw)
            for got, ref in ((ga, ra), (gb, rb)):
                assert torch.isnan(got[1]).all() and torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2])
                assert torch.isfinite(ref).all()
        assert torch.isnan(K.pair_min(x, x, box=bcell, near=True)).all()
        assert torch.isfinite(K.pair_min(x, x, box=good, near=True)).all()
        # gradients through the public function, from a cell on the GPU (taken as it is)
        xg = x.clone().requires_grad_(True)
        d = pair_distances(xg, PairList(pairs, n), box=near_cell(bcell.reshape(frames, 3, 3)))
        (gx,) = torch.autograd.grad(d[[0, 2]].sum(), xg)
        assert torch.isnan(d[1]).all() and torch.isfinite(d[[0, 2]]).all()
        assert torch.isnan(gx[1]).all() and torch.isfinite(gx[[0, 2]]).all()
    # K7
    F = dev(rng.standard_normal(tuple(x.shape)), dtype)
    o = dev(np.random.default_rng(3).uniform(1.0, 4.0, 5))
    G, E = K.gauss_pair_forces(x, 2.0, 1.0, want_energies=True, box=bcell, near=True)
    G0, E0 = K.gauss_pair_forces(x, 2.0, 1.0, want_energies=True, box=good, near=True)
    assert torch.isnan(G[1]).all() and torch.isnan(E[1]) and torch.equal(G[[0, 2]], G0[[0, 2]]) and torch.equal(E[[0, 2]], E0[[0, 2]])
    assert torch.isfinite(G0).all() and torch.isfinite(E0).all()
    assert torch.isnan(K.gauss_proj(x, F, o, 1.0, box=bcell, near=True)).all()
    assert torch.isfinite(K.gauss_proj(x, F, o, 1.0, box=good, near=True)).all()
    assert all(torch.isnan(t).all() for t in K.gauss_shift(x, F, o, 1.0, box=bcell, near=True))
    # an upper-triangular entry is not read; the nearest form needs the rows of a cell
    upper = H.copy()
    upper[:, 0, 1], upper[:, 0, 2], upper[:, 1, 2] = float("nan"), 7.0, float("inf")
    assert torch.equal(K.pair_list_dist(x, x, tab, box=rows(upper, dtype, frames), near=True),
                       K.pair_list_dist(x, x, tab, box=good, near=True))
    with pytest.raises(ValueError, match="rows of a cell"):
        K.pair_list_dist(x, x, tab, box=dev(R.DIAG_LENGTHS, dtype), near=True)
    with pytest.raises(ValueError, match="reduced|finite|positive"):
        near_cell(broken)


def test_a_cell_on_the_gpu_is_not_read_on_the_host():
    n = 19
    H = N.gpu_cell("dodecahedron", True, F64)
    x = dev(N.spread_sites(T, n, H, 5))
    F = dev(np.random.default_rng(0).standard_normal((T, n, 3)))
    pl = PairList.upper_triangle(n)
    o = dev(np.random.default_rng(1).uniform(1.0, 4.0, 5))
    unreduced = H.copy()
    unreduced[:, 1, 0] = 0.9 * unreduced[:, 0, 0]
    Hd, Ud = dev(H), dev(unreduced)
    host_cell = near_cell(H)
    want = pair_distances(x, pl, box=host_cell)  # (warm: tables, workspaces, library)
    want_min = min_distances(x, box=host_cell)
    want_g = pbc.sq_gaussian_forces(x, 2.0, 1.0, host_cell)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        cell = near_cell(Hd)
        near_cell(Ud)  # (taken as it is: the reduced condition is the caller's part)
        radius = cell.image_radius
        d = pair_distances(x, pl, box=cell)
        m = min_distances(x, box=cell)
        g = pbc.sq_gaussian_forces(x, 2.0, 1.0, cell)
        p = K.gauss_proj(x, F, o, 1.0, box=cell.rows(T).contiguous(), near=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert isinstance(radius, torch.Tensor) and radius.is_cuda and radius.dim() == 0
    assert abs(float(radius) - N.image_radius(H)) < 1e-12 and cell.images == "nearest" and cell.is_cuda
    assert torch.equal(d, want) and torch.equal(m, want_min) and torch.equal(g, want_g) and bool(torch.isfinite(p).all())


def test_the_brick_form_functions_accept_a_nearest_cell():
    x, H = split_pair()
    for cell in (near_cell(H), near_cell(dev(H))):
        xs = dev(x) if cell.is_cuda else x
        assert guess_pairwise_constraints(xs, box=cell, threshold=1e-3) == guess_pairwise_constraints(
            xs, box=Cell(cell.vectors), threshold=1e-3)
        assert frozenset((0, 1)) in guess_pairwise_constraints(xs, box=cell, threshold=1e-3)
    tree = pbc.MoleculeTree(np.array([-1, 0, -1, 2]))
    a, ka = pbc.make_whole(dev(x), near_cell(H), tree, return_images=True)
    b, kb = pbc.make_whole(dev(x), Cell(H), tree, return_images=True)
    assert torch.equal(a, b) and torch.equal(ka, kb)


def split_pair(frames=40, seed=51):
    """Four atoms in a rhombic dodecahedron, 0 and 1 a rigid pair drifting across the skewed face
    (tests/test_gpu_cell.py's system)."""
    H = R.rhombic_dodecahedron()
    rng = np.random.default_rng(seed)
    centre = np.cumsum(0.4 * rng.standard_normal((frames, 1, 3)), axis=0) + 0.3 * H[2]
    rigid = np.concatenate([centre, centre + np.array([0.5, 0.3, 0.7])], axis=1)
    return R.wrap_positions(np.concatenate([rigid, rng.uniform(0, 4, (frames, 2, 3))], axis=1), H), H


# ------------------------------------------------------------------ 5. the caller's stream
class GateCase:
    def __init__(self, name, families, build):
        self.name, self.group, self.entries, self.families = name, "nearest", (), tuple(families)
        self.build, self.synchronises, self.env, self.cleanup = build, None, None, None


def gate_cases():
    m, n, P = 6, 11, 70
    H = N.gpu_cell("dodecahedron", True, F64)
    cell = H.reshape(T, 9)
    sites = lambda k, seed: N.spread_sites(T, k, H, seed)  # noqa: E731

    def lists(pull):
        def build():
            tab = PairList(random_list(P, m, n, 300, self_form=False), n, m).on(DEV)
            floats = [dev(sites(n, 58)), dev(sites(m, 59))]
            floats += [dev(np.random.default_rng(60).standard_normal((T, P)))] if pull else []
            floats += [dev(cell)]

            def call(x_, c_, *rest):
                if pull:
                    return K.pair_list_pull(rest[0], x_, c_, tab, box=rest[1], near=True)
                return K.pair_list_dist(x_, c_, tab, box=rest[0], near=True)
            return floats, call
        return build

    def pair_min():
        return [dev(sites(n, 51)), dev(sites(m, 52)), dev(cell)], lambda x_, c_, b: K.pair_min(x_, c_, box=b, near=True)

    def k7(which):
        def build():
            floats = [dev(sites(19, 53)), dev(np.random.default_rng(54).standard_normal((T, 19, 3))), dev(cell)]
            o = dev(np.random.default_rng(55).uniform(1.0, 4.0, 37))
            if which == "site":
                return floats, lambda x_, f_, b: K.gauss_pair_forces(x_, 2.0, 1.0, want_energies=True, box=b, near=True)
            fn = K.gauss_proj if which == "proj" else K.gauss_shift
            return floats, lambda x_, f_, b: fn(x_, f_, o, 1.0, box=b, near=True)
        return build

    return [GateCase("near_pair_list_dist", ["pairlist_pbc_kernel<double, 0, 3>"], lists(False)),
            GateCase("near_pair_list_pull", ["pairlist_pull_pbc_kernel<double, double, false, 0, 3>"], lists(True)),
            GateCase("near_pair_min", ["pairmin_kernel<double, true, 3>"], pair_min),
            GateCase("near_gauss_pair_forces", ["gauss_site_forces_kernel<double, true, 3>"], k7("site")),
            GateCase("near_gauss_proj", ["gauss_proj_kernel<double, double, true, 3>"], k7("proj")),
            GateCase("near_gauss_shift", ["gauss_shift_kernel<double, double, true, 3>"], k7("shift"))]


def test_the_nearest_forms_run_on_the_callers_stream_and_never_wait(monkeypatch):
    """The method of tests/test_gpu_streams.py (tests/stream_gate.py) on the new launches: behind a gate that holds the
    caller's stream the calls return at once, and their results are those of the true data, not of the poison."""
    SG.run_behind_gate(gate_cases(), monkeypatch)
