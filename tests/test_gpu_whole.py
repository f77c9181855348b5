"""K11 on the GPU (csrc/aggf_whole.hip: whole_lds_kernel, whole_edge_kernel, whole_jump_kernel, whole_shift_kernel --
every instantiation launched and checked by name) against the NumPy reference of tests/whole_ref.py.

Parity: the image counts (``return_images``) equal the reference's EXACTLY -- they are integers, whatever the schedule
or form.  Coordinates agree within 1 ulp at the magnitude max(|x|, |u|) (``whole_ref.assert_coords``): the kernel's fma
rounds once, a reference that multiplies and subtracts rounds at most twice; derived, not measured (the reference
here rounds once too and is held to that bound; its independent two-rounding form to its own 2 ulp).  Bit-for-bit
identities: LDS form == global form, in place == out of place, a (3,) box == the same box tiled, a whole input and
``make_whole`` of its own output unchanged, a forest of roots returns the input.

Inputs: random-walk molecules with every bond component below 0.44 L, longer than the cell overall, wrapped into
[0, L) (``whole_ref.molecules``); N in {1, 2, 63, 64, 65, 131, 1025} and T in {1, 3, 9, 70}, and one N just above the
LDS form's bound at T = 2, which the library's own choice sends to the global form."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import whole_ref as R  # noqa: E402
from aggforce_amd import LinearMap, MoleculeTree, _lib, make_whole, project_forces  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd.agg import project_forces_grid_cv  # noqa: E402
from aggforce_amd.jaxutil import pair_distances  # noqa: E402

DEV = "cuda"
NAME = {"float32": "float", "float64": "double"}
SITES = (1, 2, 63, 64, 65, 131, 1025)
FRAMES = (1, 3, 9, 70)
DTYPES = ["float32", "float64"]
BOXES = [False, True]
BOX_IDS = ["one_box", "box_per_frame"]


def dev(a):
    return torch.as_tensor(np.array(a)).to(DEV)  # (a copy: the shared inputs are read-only arrays)


def launched():
    """Names of the kernels launched since the last reset, without return type and namespace."""
    torch.cuda.synchronize()
    return sorted(p.split("(")[0].replace("void ", "").replace("aggf::", "")
                  for p, c in _lib.coverage(names=True).values() if c > 0)


def reset():
    torch.cuda.synchronize()
    _lib.load().aggf_coverage_reset()


def lds_names(dtype):
    return [f"whole_lds_kernel<{NAME[dtype]}>"]


def global_names(dtype, rounds):
    return sorted([f"whole_edge_kernel<{NAME[dtype]}>", f"whole_shift_kernel<{NAME[dtype]}>"]
                  + (["whole_jump_kernel"] if rounds else []))


def shapes(tree):
    """(N, T) of a forest: all of SITES x FRAMES for the small forests; a chain only where it reaches its depth."""
    need = int(tree[5:]) + 1 if tree.startswith("chain") else 1
    return [(N, T) for N in SITES if N >= need for T in FRAMES]


# ------------------------------------------------------------------ 1. parity and the bit-for-bit identities
@pytest.mark.parametrize("tree", sorted(R.TREES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("per_frame", BOXES, ids=BOX_IDS)
def test_counts_exact_coordinates_within_one_ulp_and_the_forms_agree_bit_for_bit(tree, dtype, per_frame):
    longest = 0
    for N, T in shapes(tree):
        w, _, box, par = R.molecules(tree, N, T, dtype, per_frame)
        u, k = R.reference(tree, N, T, dtype, per_frame)
        mt = MoleculeTree(par)
        x, b = dev(w), dev(box)
        reset()
        got, images = make_whole(x, b, mt, return_images=True)
        assert launched() == lds_names(dtype)  # (the library's choice below the bound)
        assert got.dtype == x.dtype and images.dtype == torch.int32 and torch.equal(x, dev(w))  # input untouched
        assert np.array_equal(images.cpu().numpy(), k), f"image counts {tree} N={N} T={T}"
        R.assert_coords(got.cpu().numpy(), u, w, f"{tree} N={N} T={T} {dtype}")
        R.assert_coords(got.cpu().numpy(), R.shift_plain(w, box, k), w, f"plain form {tree} N={N} T={T}", ulps=2)
        longest = max(longest, int(np.abs(k).max()))
        tab = mt.on(DEV)
        reset()
        im2 = torch.empty_like(images)
        glob = K.make_whole(x, b, tab, images=im2, _form=K.WHOLE_GLOBAL)
        assert launched() == global_names(dtype, mt.n_rounds)
        assert torch.equal(glob, got) and torch.equal(im2, images), "LDS form != global form"
        assert torch.equal(K.make_whole(x, b, tab, _form=K.WHOLE_LDS), got)
        for form in (K.WHOLE_LDS, K.WHOLE_GLOBAL):  # in place
            y = x.clone()
            assert K.make_whole(y, b, tab, out=y, _form=form) is y and torch.equal(y, got), f"in place, form {form}"
        y = x.clone()
        assert make_whole(y, b, mt, inplace=True) is y and torch.equal(y, got)
        if not per_frame:
            tiled = b.expand(T, 3).contiguous()
            assert torch.equal(make_whole(x, tiled, mt), got), "a (3,) box != the same box tiled"
            assert torch.equal(K.make_whole(x, tiled, tab, _form=K.WHOLE_GLOBAL), got)
        again, zero = make_whole(got, b, mt, return_images=True)  # whole already: unchanged, bit for bit
        assert torch.equal(again, got) and not zero.any()
        assert torch.equal(got[:, dev(par < 0)], x[:, dev(par < 0)])  # a root never moves
        roots = MoleculeTree(R.TREES["none"](N))
        assert torch.equal(make_whole(x, b, roots), x) and torch.equal(K.make_whole(x, b, roots.on(DEV), _form=2), x)
    if tree == "chain130":
        assert longest >= 2, "the molecules are not longer than the cell"


def test_the_whole_input_is_returned_unchanged():
    """The open walk with its roots in the cell is whole: every count is 0 and the output is the input bit for bit."""
    for dtype in DTYPES:
        for per_frame in BOXES:
            w, x, box, par = R.molecules("chain17", 131, 9, dtype, per_frame)
            out, images = make_whole(dev(x), dev(box), MoleculeTree(par), return_images=True)
            assert torch.equal(out, dev(x)) and not images.any()
            assert not torch.equal(dev(w), dev(x))


@pytest.mark.parametrize("dtype", DTYPES)
def test_just_above_the_lds_bound_the_library_takes_the_global_form(dtype):
    N = K.whole_lds_max_sites() + 1
    T = 2
    assert N == 6825
    for tree in ("random", "chain17"):
        w, _, box, par = R.molecules(tree, N, T, dtype, True)
        u, k = R.reference(tree, N, T, dtype, True)
        mt = MoleculeTree(par)
        x, b = dev(w), dev(box)
        reset()
        got, images = make_whole(x, b, mt, return_images=True)
        assert launched() == global_names(dtype, mt.n_rounds) and mt.n_rounds > 0
        assert np.array_equal(images.cpu().numpy(), k)
        R.assert_coords(got.cpu().numpy(), u, w, f"global {tree} N={N} {dtype}")
        with pytest.raises(_lib.AggfError, match="LDS form"):
            K.make_whole(x, b, mt.on(DEV), _form=K.WHOLE_LDS)
        # the largest frame the LDS form holds, against the global form
        xs, ts = x[:, :N - 1].contiguous(), MoleculeTree(np.where(par[:N - 1] < N - 1, par[:N - 1], -1))
        reset()
        lds = K.make_whole(xs, b, ts.on(DEV), _form=K.WHOLE_LDS)
        assert launched() == lds_names(dtype)
        assert torch.equal(lds, K.make_whole(xs, b, ts.on(DEV), _form=K.WHOLE_GLOBAL))
        assert torch.equal(lds, make_whole(xs, b, ts))
    # frames beyond the workspace cap go in further calls
    cap, K._WHOLE_WS_BYTES = K._WHOLE_WS_BYTES, 1
    try:
        assert torch.equal(make_whole(x, b, mt), got)
    finally:
        K._WHOLE_WS_BYTES = cap


# ------------------------------------------------------------------ 2. views: rows off the 16-byte grid
@pytest.mark.parametrize("dtype", DTYPES)
def test_views_whose_rows_start_off_the_16_byte_grid(dtype):
    for tree, N in (("random", 65), ("chain5", 131), ("mixed", 63), ("chain130", 1025)):
        T = 9
        w, _, box, par = R.molecules(tree, N, T + 1, dtype, True)
        mt = MoleculeTree(par)
        big, b = dev(w), dev(box)
        whole_all = make_whole(big, b, mt)
        # xyz[1:] of a larger array, and a frame slice from the middle
        for sl in (slice(1, None), slice(3, 7)):
            view = big[sl]
            assert view.is_contiguous()
            if dtype == "float32" and N % 4:
                assert big[1:].data_ptr() % 16 != 0  # an odd N in float32: the second row is off the grid
            assert torch.equal(make_whole(view, b[sl], mt), whole_all[sl]), (tree, sl)
        # every phase of the input and of the output against the 16-byte grid, both forms, out of place and in place
        esz = big.element_size()
        n_el = T * N * 3
        ref = whole_all[:T]
        for shift_in in range(16 // esz):
            buf = torch.zeros(n_el + 8, dtype=big.dtype, device=DEV)
            xin = buf[shift_in:shift_in + n_el].view(T, N, 3)
            xin.copy_(big[:T])
            assert xin.data_ptr() % 16 == (buf.data_ptr() + shift_in * esz) % 16
            for shift_out in range(16 // esz):
                obuf = torch.full((n_el + 8,), 7.0, dtype=big.dtype, device=DEV)
                out = obuf[shift_out:shift_out + n_el].view(T, N, 3)
                for form in (K.WHOLE_LDS, K.WHOLE_GLOBAL):
                    out.fill_(7.0)
                    K.make_whole(xin, b[:T], mt.on(DEV), out=out, _form=form)
                    assert torch.equal(out, ref), (tree, shift_in, shift_out, form)
                    assert (obuf[:shift_out] == 7).all() and (obuf[shift_out + n_el:] == 7).all()  # nothing beyond
            K.make_whole(xin, b[:T], mt.on(DEV), out=xin, _form=K.WHOLE_LDS)
            assert torch.equal(xin, ref) and not buf[:shift_in].any() and not buf[shift_in + n_el:].any()
    # a non-contiguous view is copied, not written through
    w, _, box, par = R.molecules("star", 64, 9, dtype, False)
    x = dev(w)
    strided = x[::2]
    assert torch.equal(make_whole(strided, dev(box), MoleculeTree(par)), make_whole(x, dev(box), MoleculeTree(par))[::2])
    with pytest.raises(ValueError, match="contiguous"):
        make_whole(strided, dev(box), MoleculeTree(par), inplace=True)


# ------------------------------------------------------------------ 3. edge behaviour
@pytest.mark.parametrize("form", [K.WHOLE_LDS, K.WHOLE_GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_bad_box_on_the_device_marks_its_frame_only(dtype, form):
    for tree, N, T in (("chain17", 131, 9), ("random", 65, 70), ("star", 2, 3)):
        w, _, box, par = R.molecules(tree, N, T, dtype, True)
        tab = MoleculeTree(par).on(DEV)
        x = dev(w)
        good_im = torch.empty((T, N, 3), dtype=torch.int32, device=DEV)
        good = K.make_whole(x, dev(box), tab, images=good_im, _form=form)
        for value in (0.0, -1.5, float("inf"), float("nan")):
            bad = box.copy()
            bad[T // 2, 1] = value
            images = torch.full((T, N, 3), 99, dtype=torch.int32, device=DEV)
            got = K.make_whole(x, dev(bad), tab, images=images, _form=form)
            others = torch.ones(T, dtype=torch.bool, device=DEV)
            others[T // 2] = False
            assert torch.equal(got[others], good[others]) and torch.equal(images[others], good_im[others])
            # the bad component is NaN with counts 0; the frame's other two components are untouched
            assert torch.isnan(got[T // 2, :, 1]).all() and not images[T // 2, :, 1].any()
            assert torch.equal(got[T // 2][:, [0, 2]], good[T // 2][:, [0, 2]])
            assert torch.equal(images[T // 2][:, [0, 2]], good_im[T // 2][:, [0, 2]])
        bad = dev(box)
        bad[T // 2] = 0.0  # all three lengths: the whole frame
        images = torch.full((T, N, 3), 99, dtype=torch.int32, device=DEV)
        got = K.make_whole(x, bad, tab, images=images, _form=form)
        assert torch.isnan(got[T // 2]).all() and not images[T // 2].any()
    # the public function does not synchronise for a box on the device, and checks one on the host
    assert torch.isnan(make_whole(x, bad, MoleculeTree(par))[T // 2]).all()
    with pytest.raises(ValueError, match="positive and finite"):
        make_whole(x, bad.cpu(), MoleculeTree(par))


@pytest.mark.parametrize("form", [K.WHOLE_LDS, K.WHOLE_GLOBAL], ids=["lds", "global"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_finite_coordinate_stays_and_shifts_nothing_else(dtype, form):
    w, _, box, par = R.molecules("chain5", 65, 9, dtype, True)
    tab = MoleculeTree(par).on(DEV)
    good = K.make_whole(dev(w), dev(box), tab, _form=form)
    x = w.copy()
    x[2, 7, 0], x[3, 8, 2], x[5, 0, 1] = np.nan, np.inf, -np.inf
    ref_u, ref_k = R.whole(x, box, par)
    images = torch.empty((9, 65, 3), dtype=torch.int32, device=DEV)
    got = K.make_whole(dev(x), dev(box), tab, images=images, _form=form)
    assert np.array_equal(images.cpu().numpy(), ref_k)
    R.assert_coords(got.cpu().numpy(), ref_u, x, f"non-finite {dtype}")
    assert torch.isnan(got[2, 7, 0]) and got[3, 8, 2] == float("inf") and got[5, 0, 1] == -float("inf")
    touched = np.zeros(x.shape, dtype=bool)  # the atom and what hangs below it in its chain of six
    touched[2, 7:12, 0] = touched[3, 8:12, 2] = touched[5, 0:6, 1] = True
    keep = dev(~touched)
    assert torch.equal(got[keep], good[keep])


@pytest.mark.parametrize("form", [K.WHOLE_LDS, K.WHOLE_GLOBAL], ids=["lds", "global"])
def test_an_index_out_of_range_gives_nan_and_reads_nothing_outside(form):
    """The host constructor refuses such forests; tables handed to the kernel directly are tested against N there."""
    w, _, box, par = R.molecules("chain5", 65, 3, "float64", False)
    mt = MoleculeTree(par)
    good = K.make_whole(dev(w), dev(box), mt.on(DEV), _form=form)
    for bad_value in (65, -2, 1 << 30):
        p = par.astype(np.int32)
        p[20] = bad_value  # atom 20 (a chain of 18..23): it and the atoms below it are marked
        got = K.make_whole(dev(w), dev(box), K.TreeTables(dev(p), dev(mt.jumps)), _form=form)
        assert torch.isnan(got[:, 20]).all()
        fine = np.ones(65, dtype=bool)
        fine[20:24] = False
        assert torch.equal(got[:, dev(fine)], good[:, dev(fine)])
        j = mt.jumps.copy()
        j[1, 40] = bad_value  # atom 40 (36..41) in the second round
        got = K.make_whole(dev(w), dev(box), K.TreeTables(dev(par.astype(np.int32)), dev(j)), _form=form)
        fine = np.ones(65, dtype=bool)
        fine[40:42] = False
        assert torch.isnan(got[:, 40]).all() and torch.equal(got[:, dev(fine)], good[:, dev(fine)])


def test_empty_shapes_and_refusals():
    mt = MoleculeTree(R.star(5))
    b = dev(R.BOX)
    assert make_whole(torch.zeros((0, 5, 3), device=DEV), b, mt).shape == (0, 5, 3)
    assert make_whole(torch.zeros((4, 0, 3), device=DEV), b, MoleculeTree(np.zeros(0, dtype=np.int64))).shape == (4, 0, 3)
    x = torch.zeros((4, 5, 3), device=DEV)
    with pytest.raises(ValueError, match="box"):
        K.make_whole(x, b.double(), mt.on(DEV))  # the box in another dtype
    with pytest.raises(ValueError, match="tree"):
        K.make_whole(x, b.float(), MoleculeTree(R.star(6)).on(DEV))
    with pytest.raises(ValueError, match="images"):
        K.make_whole(x, b.float(), mt.on(DEV), images=torch.zeros((4, 5, 3), device=DEV))
    out = make_whole(torch.arange(60, device=DEV).reshape(4, 5, 3), b, mt)  # integers are computed in float64
    assert out.dtype == torch.float64


# ------------------------------------------------------------------ 4. bond lengths
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("per_frame", BOXES, ids=BOX_IDS)
def test_open_bond_lengths_of_the_whole_molecule_are_the_minimum_image_ones(dtype, per_frame):
    """|u_c - u_p| (open, on the output) against |min_image(x_c - x_p)| (on the input under the box), over the forest's
    own (child, parent) pairs.  Tolerance: 8 ulp at the largest coordinate magnitude M = max(|x|, |u|) of the frame
    set.  Per component the two displacements differ by the roundings of u_c and u_p (1/2 ulp(M) each), of the raw
    difference x_c - x_p (1/2 ulp of a value below 2 M: 1 ulp(M)) and of u_c - u_p (below 1/2 ulp(M)): 2.5 ulp(M);
    the norm of three such components differs by at most sqrt(3) * 2.5 = 4.4 ulp(M), and the three roundings of each
    dot product and the root add less than 2 ulp of a distance that is below M each way: under 8."""
    for tree, N, T in (("chain130", 1025, 9), ("random", 131, 70), ("mixed", 65, 9), ("star", 64, 3)):
        w, _, box, par = R.molecules(tree, N, T, dtype, per_frame)
        mt = MoleculeTree(par)
        x, b = dev(w), dev(box)
        u = make_whole(x, b, mt)
        open_d = pair_distances(u, mt.pairs)
        box_d = pair_distances(x, mt.pairs, box=b)
        assert open_d.shape == (T, int((par >= 0).sum()))
        M = float(torch.maximum(x.abs().max(), u.abs().max()))
        ulp = float(np.spacing(np.asarray(M, dtype=dtype)))
        worst = float((open_d - box_d).abs().max()) / ulp
        print(f"{tree} {dtype}: bond lengths differ by at most {worst:.3g} ulp(M) (bound 8)")
        assert worst <= 8
        assert (open_d <= 0.5 * b.reshape(-1, 3).norm(dim=1).max()).all()  # (every component within half its length)
        child = np.flatnonzero(par >= 0)
        raw = np.abs(w[:, child].astype(np.float64) - w[:, par[child]])
        assert (raw > 0.5 * box.reshape(-1, 1, 3)).any()  # the wrapped input does have split bonds


# ------------------------------------------------------------------ 5. autograd
def test_the_backward_is_the_identity():
    w, _, box, par = R.molecules("random", 65, 3, "float32", True)
    mt = MoleculeTree(par)
    x = dev(w).requires_grad_()
    reset()
    out = make_whole(x, dev(box), mt)
    assert launched() == lds_names("float32") and out.requires_grad
    assert torch.equal(out.detach(), make_whole(dev(w), dev(box), mt))
    out.sum().backward()
    assert torch.equal(x.grad, torch.ones_like(x))
    weights = torch.randn_like(out)
    g, = torch.autograd.grad((make_whole(x, dev(box), mt) * weights).sum(), x)
    assert torch.equal(g, weights)
    whole, images = make_whole(x, dev(box), mt, return_images=True)
    assert whole.requires_grad and not images.requires_grad and images.dtype == torch.int32
    with pytest.raises(ValueError, match="inplace"):
        make_whole(x, dev(box), mt, inplace=True)
    with pytest.raises(ValueError, match="constant"):
        make_whole(x, dev(box).requires_grad_(), mt)


def test_gradcheck_in_float64():
    """T = 2, N = 5: a chain wrapped across the faces; the finite differences (1e-6) stay far from any tie of the wrap
    (bond components are at most 0.44 L, a tie is at 0.5 L)."""
    w, _, box, par = R.molecules("chain4", 5, 2, "float64", True, seed=3)
    assert R.reference("chain4", 5, 2, "float64", True, seed=3)[1].any()
    mt = MoleculeTree(par)
    x = dev(w).requires_grad_()
    b = dev(box)
    assert torch.autograd.gradcheck(lambda a: make_whole(a, b, mt), (x,), eps=1e-6, atol=1e-6, rtol=1e-6)
    assert torch.autograd.gradgradcheck(lambda a: make_whole(a, b, mt) ** 2, (x,), eps=1e-6, atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------ 6. end to end
N_BEADS, BEAD, E2E_T = 16, 4, 41
E2E_BOX = np.array([4.1, 5.3, 6.7])


def bead_trajectory(T=E2E_T):
    """64 atoms in 16 four-atom beads, T (41) frames: (whole, wrapped, forces, bonds).  A bead is a rigid triangle plus a
    fourth atom on a fluctuating bond, its first atom diffusing inside the cell; ``whole`` is that trajectory with
    every bead's first atom (the root of its bonds) in the cell, ``wrapped`` every atom wrapped into [0, L)."""
    rng = np.random.default_rng(20261018)
    n = N_BEADS * BEAD
    centre = E2E_BOX * rng.random((1, N_BEADS, 3)) + 0.2 * rng.standard_normal((T, N_BEADS, 3))
    centre -= E2E_BOX * np.floor(centre / E2E_BOX)  # the roots in the cell
    shape = rng.uniform(-0.6, 0.6, (1, N_BEADS, BEAD, 3))
    shape[:, :, 0] = 0.0
    x = centre[:, :, None, :] + shape
    x[:, :, 3] += 0.15 * rng.standard_normal((T, N_BEADS, 3))
    whole = x.reshape(T, n, 3)
    wrapped = whole - E2E_BOX * np.floor(whole / E2E_BOX)
    forces = 30 * rng.standard_normal(whole.shape)
    first = np.arange(N_BEADS) * BEAD
    bonds = np.concatenate([np.stack([first, first + 1], 1), np.stack([first + 1, first + 2], 1),
                            np.stack([first + 2, first], 1), np.stack([first + 2, first + 3], 1)])
    return whole, wrapped, forces, bonds


def bead_map():
    return LinearMap([list(range(BEAD * c, BEAD * c + BEAD)) for c in range(N_BEADS)], n_fg_sites=N_BEADS * BEAD)


RIGID = {frozenset((BEAD * c + i, BEAD * c + j)) for c in range(N_BEADS) for i, j in ((0, 1), (0, 2), (1, 2))}
COORD_TOL = 64 * np.finfo(np.float64).eps * float(E2E_BOX.max())  # see test_project_forces_makes_the_beads_whole


def straddles(wrapped):
    """(T, N_BEADS): does the bead have two atoms more than half a box length apart in some component?"""
    b = wrapped.reshape(-1, N_BEADS, BEAD, 3)
    spread = b.max(axis=2) - b.min(axis=2)
    return (spread > 0.5 * E2E_BOX).any(axis=2)


@pytest.mark.parametrize("on_gpu", [False, True], ids=["numpy", "gpu_tensors"])
def test_project_forces_makes_the_beads_whole(on_gpu):
    """The wrapped trajectory with ``box=`` and ``bonds=`` against the whole one.  The made-whole coordinates are
    w - k L where w = fl(x - m L): they equal x up to the roundings of the wrap and the unwrap, a few ulp of the
    largest coordinate (below max(L)); an average of four of them and the map's float64 products add a few more:
    COORD_TOL = 64 eps max(L) is that with room, and 1e14 times below the box length the defect is off by."""
    whole, wrapped, forces, bonds = bead_trajectory()
    split = straddles(wrapped)
    assert split.any(axis=1).sum() >= 10 and not split.all(), f"{int(split.sum())} (frame, bead) pairs lie across a face"
    assert not straddles(whole).any()
    cmap = bead_map()
    conv = dev if on_gpu else (lambda a: a)
    host = (lambda a: a.cpu().numpy()) if on_gpu else (lambda a: a)
    kw = dict(l2_regularization=1.0)
    ref = project_forces(conv(whole), conv(forces), cmap, **kw)
    assert ref["constraints"] == RIGID
    given = conv(wrapped)
    keep = given.clone() if on_gpu else given.copy()
    got = project_forces(given, conv(forces), cmap, box=conv(E2E_BOX) if on_gpu else E2E_BOX, bonds=bonds, **kw)
    assert (torch.equal(given, keep) if on_gpu else np.array_equal(given, keep)), "the caller's array was written"
    assert type(got["mapped_coords"]) is type(ref["mapped_coords"]) and type(got["mapped_forces"]) is type(ref["mapped_forces"])
    assert got["constraints"] == RIGID
    assert np.array_equal(got["tmap"].force_map.standard_matrix, ref["tmap"].force_map.standard_matrix)
    assert np.array_equal(host(got["mapped_forces"]), host(ref["mapped_forces"]))
    err = np.abs(host(got["mapped_coords"]) - host(ref["mapped_coords"])).max()
    print(f"mapped_coords: max |wrapped + bonds - whole| = {err:.3e}, bound {COORD_TOL:.3e}")
    assert err <= COORD_TOL
    # a MoleculeTree and a PairList do the same
    tree = MoleculeTree.from_bonds(N_BEADS * BEAD, bonds)
    again = project_forces(given, conv(forces), cmap, box=E2E_BOX, bonds=tree, **kw)
    assert np.array_equal(host(again["mapped_coords"]), host(got["mapped_coords"]))
    # the defect, and today's behaviour of bonds=None: the box alone leaves the mapped coordinates of the split beads
    # off by a quarter, a half or three quarters of a box length (one to three of four atoms on the far side)
    boxed = project_forces(given, conv(forces), cmap, box=E2E_BOX, **kw)
    assert boxed["constraints"] == RIGID  # (the guess is right with the box alone)
    off = np.abs(host(boxed["mapped_coords"]) - host(ref["mapped_coords"]))
    per_bead = off.max(axis=2)
    print(f"box alone: mapped_coords off by up to {off.max():.3f} (box {E2E_BOX})")
    assert (per_bead[split] >= 0.25 * E2E_BOX.min() - 1e-9).all() and off.max() <= 0.75 * E2E_BOX.max() + 1e-9
    assert (per_bead[~split] <= COORD_TOL).all()
    plain = wrapped.reshape(E2E_T, N_BEADS, BEAD, 3).mean(axis=2)  # coord_map of the coordinates as given
    assert np.abs(host(boxed["mapped_coords"]) - plain).max() <= COORD_TOL


CV_T = 120
KBT = 0.6955215
CV_MATCH, CV_DIFFER = 1e-5, 1e-3


@pytest.mark.parametrize("reuse", [True, False], ids=["one_pass", "loop"])
def test_grid_cv_makes_the_beads_whole_before_the_folds(reuse):
    """The check of test_project_forces_makes_the_beads_whole through project_forces_grid_cv, with a method whose
    scores depend on the coordinates: ``qp_feat_linear_map`` with ``gb_feat`` (Gaussians of the distances between the
    atoms' constraint groups and the mapped sites), in its one-pass form (``_grid_cv_feat_reuse``) and in the loop
    over ``project_forces``.  The linear optimiser would not do: its scores are a function of the forces and the
    constraint set alone.

    wrapped + box + bonds must reproduce the scores of the whole input: the coordinates agree to COORD_TOL (a few
    float64 ulp), the features are float32, so a handful of them may round the other way, each by 6e-8 relative:
    CV_MATCH = 1e-5, the bound tests/test_gpu_feat.py holds two arithmetic forms of this same score to.  wrapped + box
    WITHOUT bonds must not: its split beads put group means and mapped sites a fraction of a box length off, which
    moves distances across several Gaussian widths; it has to differ by more than CV_DIFFER = 100 CV_MATCH."""
    from aggforce_amd import agg
    from aggforce_amd.qp import Multifeaturize, gb_feat, id_feat, qp_feat_linear_map
    from aggforce_amd.util import Curry

    whole, wrapped, forces, bonds = bead_trajectory(CV_T)
    split = straddles(wrapped)
    assert split.any(axis=1).sum() >= CV_T // 2 and not straddles(whole).any()
    cmap = bead_map()
    feat = Multifeaturize([id_feat, Curry(gb_feat, outer=6.0, inner=0.0, n_basis=4, width=1.0)])
    grid = {"l2_regularization": [1.0, 1e3]}
    calls = {"n": 0}
    real = agg._grid_cv_feat_reuse

    def counted(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    def go(coords, **extra):
        return project_forces_grid_cv(grid, coords, forces, n_folds=2, rng=np.random.default_rng(0), reuse_gram=reuse,
                                      method_rng=np.random.default_rng(17), coord_map=cmap, constrained_inds=set(RIGID),
                                      method=qp_feat_linear_map, featurizer=feat, kbt=KBT, n_constraint_frames=6, **extra)

    agg._grid_cv_feat_reuse = counted
    try:
        ref = go(whole)
        keep = wrapped.copy()
        got = go(wrapped, box=E2E_BOX, bonds=bonds)
        assert np.array_equal(wrapped, keep), "the caller's array was written"
        boxed = go(wrapped, box=E2E_BOX)
    finally:
        agg._grid_cv_feat_reuse = real
    assert calls["n"] == (3 if reuse else 0)  # the one-pass form ran where it was asked for, bonds= or not
    assert set(got["scores"]) == set(ref["scores"]) == set(boxed["scores"]) and len(ref["scores"]) == 2
    for key, want in ref["scores"].items():
        with_bonds = abs(got["scores"][key] - want) / abs(want)
        without = abs(boxed["scores"][key] - want) / abs(want)
        print(f"{key}: whole {want!r}; wrapped with bonds {got['scores'][key]!r} (rel {with_bonds:.2e}, bound "
              f"{CV_MATCH}); wrapped, box alone {boxed['scores'][key]!r} (rel {without:.2e}, must exceed {CV_DIFFER})")
        assert got["n_runs"][key] == ref["n_runs"][key] == boxed["n_runs"][key] == 2
        assert with_bonds <= CV_MATCH
        assert without > CV_DIFFER
