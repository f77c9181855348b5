"""NumPy float64 reference of the NEAREST IMAGE of a triclinic cell (``Cell(vectors, images="nearest")``,
csrc/aggf_common.h ``nearest_image``), shared by tests/test_nearest_host.py and tests/test_gpu_nearest.py.

The brick reduction of tests/cell_ref.py, then the shortest of the brick image's 27 translates d + i a + j b + k c,
i, j, k in {-1, 0, 1}, by squared length, in the documented order ``ORDER``: (0, 0, 0) first, then k = -1, 0, 1
outermost, j inside it, i innermost; a candidate replaces the best so far only if it is strictly shorter.  A translate
is formed c first, ((d + k c) + j b) + i a, as the kernels nest their fmas.  ``image_radius`` is half the shortest of
the 26 lattice vectors.  Also here: the test cells, the brute force that validates the guarantee, the distance of an
element from a tie between two candidates, sites whose pairs reach between the two radii, and the restatement of map
validation (tests/mapval_pbc_ref.py) with the nearest displacement."""
import numpy as np
import torch

import cell_ref as R
import mapval_ref as mref
from mapval_pbc_ref import _coef

ORDER = [(0, 0, 0)] + [(i, j, k) for k in (-1, 0, 1) for j in (-1, 0, 1) for i in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]
TIE = 1e-3  # an element whose two shortest candidates differ by less than this (relative, squared length) is "on a tie"

D = R.D


def dodecahedron_square(d=D):
    return R.rhombic_dodecahedron(d)


def dodecahedron_hexagonal(d=D):
    return np.array([[d, 0, 0], [d / 2, np.sqrt(3) * d / 2, 0], [d / 2, np.sqrt(3) * d / 6, np.sqrt(6) * d / 3]])


def octahedron(d=D):
    """The truncated octahedron of image distance d (tests/cell_ref.py's: its three vectors have length d)."""
    return R.truncated_octahedron(d)


STANDARD = {"dodecahedron": dodecahedron_square, "dodecahedron_hex": dodecahedron_hexagonal, "octahedron": octahedron}
# a dyadic reduced cell shaped like the square dodecahedron: power-of-two diagonal (every quotient of the brick stages
# is exact), safe radius 2, image radius sqrt(48) / 2 = 3.46
DYADIC_NEAR = np.array([[8.0, 0, 0], [0, 8.0, 0], [4.0, 4.0, 4.0]])


def frame_cells(kind, T, seed=0):
    """(T, 3, 3): the standard cell ``kind`` breathing by a few percent from frame to frame (an isotropic factor keeps
    it reduced)."""
    s = 1 + 0.03 * np.random.default_rng(8000 + seed).uniform(-1, 1, T)
    return STANDARD[kind]()[None] * s[:, None, None]


def is_reduced(H):
    H = np.asarray(H, dtype=np.float64)
    ax, bx, by, cx, cy = H[..., 0, 0], H[..., 1, 0], H[..., 1, 1], H[..., 2, 0], H[..., 2, 1]
    return bool(np.all((np.abs(bx) <= ax / 2) & (np.abs(cx) <= ax / 2) & (np.abs(cy) <= by / 2)))


def random_reduced_cell(rng, ratio=4.0):
    """A reduced lower-triangular cell with diagonal entries in [1, ratio] and skews anywhere in the allowed range."""
    ax, by, cz = rng.uniform(1, ratio, 3)
    return np.array([[ax, 0, 0], [rng.uniform(-ax / 2, ax / 2), by, 0],
                     [rng.uniform(-ax / 2, ax / 2), rng.uniform(-by / 2, by / 2), cz]])


def image_radius(H):
    """Half the length of the shortest of the 26 lattice vectors i a + j b + k c over all frames of H."""
    H = np.asarray(H, dtype=np.float64)
    ijk = np.array(ORDER[1:], dtype=np.float64)
    return float(np.linalg.norm(ijk @ H, axis=-1).min()) / 2


def candidates(b, H):
    """(27, ..., 3) translates of the brick image b (T, ..., 3) in ``ORDER`` and their squared lengths (27, ...)."""
    ax, bx, by, cx, cy, cz = R.entries(H, b)
    out = []
    for i, j, k in ORDER:
        x = ((b[..., 0] + k * cx) + j * bx) + i * ax
        y = (b[..., 1] + k * cy) + j * by
        z = b[..., 2] + k * cz
        out.append(np.stack([x, y, z], axis=-1))
    c = np.stack(out)
    return c, (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]


def nearest(d, H, prune=False):
    """(image, pick, gap): the nearest image of d (T, ..., 3) under H ((3, 3) or (T, 3, 3)); the index into ``ORDER`` of
    the chosen candidate (0: the brick image); and the relative gap in squared length between the two shortest
    candidates (below ``TIE``: on a tie).  ``prune``: skip the search where the brick image's squared length is at
    most min(ax, by, cz)^2 / 4, as the kernels do -- the same numbers."""
    b = R.wrap(d, H)
    c, q = candidates(b, H)
    best, pick = q[0].copy(), np.zeros(q.shape[1:], dtype=np.int64)
    for s in range(1, 27):
        shorter = q[s] < best
        best, pick = np.where(shorter, q[s], best), np.where(shorter, s, pick)
    if prune:
        ax, _, by, _, _, cz = R.entries(H, b)
        m = np.minimum(np.minimum(ax, by), cz)
        pick = np.where(q[0] <= 0.25 * (m * m), 0, pick)
    image = np.take_along_axis(c, np.broadcast_to(pick[None, ..., None], (1,) + b.shape), axis=0)[0]
    two = np.sort(q, axis=0)[:2]
    gap = (two[1] - two[0]) / np.maximum(two[1], 1e-300)
    return image, pick, gap


def wrap(d, H):
    return nearest(d, H)[0]


def comp_bound(d, H):
    """Per component, the magnitudes the nearest image is formed from: those of the brick image (cell_ref.comp_bound)
    plus |i| ax + |j| |bx| + |k| |cx|, |j| by + |k| |cy|, |k| cz of the chosen translate."""
    ax, bx, by, cx, cy, cz = R.entries(H, d)
    ijk = np.abs(np.array(ORDER, dtype=np.float64))[nearest(d, H)[1]]
    i, j, k = ijk[..., 0], ijk[..., 1], ijk[..., 2]
    extra = np.stack([i * ax + j * np.abs(bx) + k * np.abs(cx), j * by + k * np.abs(cy), k * cz], axis=-1)
    return R.comp_bound(d, H) + extra


def brute_from_brick(d, H, reach=3):
    """The minimum image of d (M, 3) under ONE cell H (3, 3) by brute force over the shifts in [-reach, reach]^3 of its
    BRICK image: (image, length)."""
    return R.brute_min(R.wrap(d[None], H)[0], H, reach=reach)


def torch_wrap(d, H):
    """The nearest image of d (T, ..., 3 tensor) under H, differentiable in d: the brick image of cell_ref.torch_wrap
    plus the lattice vector this reference chooses (a constant)."""
    b = R.torch_wrap(d, H)
    bn = b.detach().numpy()
    shift = torch.as_tensor(nearest(d.detach().numpy(), H)[0] - R.wrap(d.detach().numpy(), H))
    assert np.allclose(bn + shift.numpy(), nearest(d.detach().numpy(), H)[0], atol=1e-12)
    return b + shift


# ------------------------------------------------------------------ sites whose pairs reach between the two radii
def spread_sites(T, n, H, seed):
    """(T, n, 3): sites uniform over the cell of every frame, then every site moved by its own lattice vectors (counts
    in -2..2): pair displacements of every length the cell has, raw displacements several cells long."""
    rng = np.random.default_rng(seed)
    Hf = np.broadcast_to(np.asarray(H, dtype=np.float64), (T, 3, 3))
    x = np.einsum("tnk,tkj->tnj", rng.random((T, n, 3)), Hf)
    return x + np.einsum("tnk,tkj->tnj", rng.integers(-2, 3, (T, n, 3)).astype(np.float64), Hf)


def free_sites(make, disp, H, dtype, nearest_margin=None, tries=400):
    """The first of make(0), make(1), ... (arrays as stored in ``dtype``) whose displacements ``disp(*sites)`` are
    further than twice pbc_ref.MARGIN[dtype] from a tie of the brick stages and, with ``nearest_margin``, all further
    than that from a tie between two candidates.  Returns the sites as float64."""
    for k in range(tries):
        sites = tuple(np.asarray(torch.as_tensor(s).to(dtype).double().numpy()) for s in make(k))
        d = disp(*sites)
        if R.tie_distance(d, H) <= 2 * R.MARGIN[dtype]:
            continue
        if nearest_margin is not None and nearest(d, H)[2].min() <= nearest_margin:
            continue
        return sites
    raise AssertionError("no tie-free input found")


def input_conditions(d, H):
    """(fraction of the elements of d whose nearest image differs from the brick image, fraction on a tie)."""
    _, pick, gap = nearest(d, H)
    return float((pick != 0).mean()), float((gap < TIE).mean())


# ------------------------------------------------------------------ the constructions of tests/test_gpu_nearest.py
# (their conditions -- enough elements whose nearest image is not the brick image, few on a tie -- are asserted on this
# reference alone by tests/test_nearest_host.py)
GPU_KINDS = ["dodecahedron", "octahedron"]
GPU_T = 7


def stored(a, dtype):
    """``a`` as float64 after a round trip through the torch dtype ``dtype``: what the device holds."""
    return torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype).double().numpy()


def gpu_cell(kind, per_frame, dtype, T=GPU_T, seed=0):
    """The cell of a GPU case as stored in ``dtype``: (3, 3), or (T, 3, 3) breathing from frame to frame."""
    return stored(frame_cells(kind, T, seed) if per_frame else STANDARD[kind](), dtype)


def list_case(kind, per_frame, pairs, m, n, dtype, seed=0, T=GPU_T):
    """(H, x, c, raw, tie): the cell, the sites of a list call as stored in ``dtype`` (c is x in the self form, m None),
    the raw displacements of the pairs, and the elements (T, P) on a tie between two candidates."""
    H = gpu_cell(kind, per_frame, dtype, T, seed)
    base = 1000 * T + 10 * len(pairs) + n + seed

    def make(k):
        x = spread_sites(T, n, H, base + 7919 * k)
        return (x, x if m is None else spread_sites(T, m, H, base + 7919 * k + 1))

    def disp(x, c):
        return x[:, pairs[:, 1]] - c[:, pairs[:, 0]]

    x, c = free_sites(make, disp, H, dtype)
    raw = disp(x, c)
    return H, x, c, raw, nearest(raw, H)[2] < TIE


def matrix_case(kind, per_frame, m, n, dtype, seed=0, T=GPU_T):
    """As ``list_case`` for all (i, j) of m x n sites (m None: the self form): raw is (T, m, n, 3)."""
    H = gpu_cell(kind, per_frame, dtype, T, seed)

    def make(k):
        x = spread_sites(T, n, H, 500 + seed + 7919 * k)
        return (x, x if m is None else spread_sites(T, m, H, 501 + seed + 7919 * k))

    def disp(x, c):
        return x[:, None, :, :] - c[:, :, None, :]

    x, c = free_sites(make, disp, H, dtype)
    raw = disp(x, c)
    return H, x, c, raw, nearest(raw, H)[2] < TIE


MV_N = 19


def mapval_case(kind, per_frame, dtype, seed=0, T=GPU_T, n=MV_N):
    """(H, X, F, outer): sites as stored in ``dtype`` with NO pair on a tie (every pair enters every sum), forces, and
    an ``outer`` between the safe radius and the image radius."""
    H = gpu_cell(kind, per_frame, dtype, T, seed)

    def make(k):
        return (spread_sites(T, n, H, 900 + seed + 7919 * k),)

    (X,) = free_sites(make, lambda x: x[:, :, None, :] - x[:, None, :, :] + 0.0, H, dtype, nearest_margin=TIE)
    F = stored(30.0 * np.random.default_rng(seed).standard_normal((T, n, 3)), dtype)
    outer = 0.5 * (R.safe_radius(H) + image_radius(H)) + 0.2 * (image_radius(H) - R.safe_radius(H))
    return H, X, F, outer


def dyadic_case(T, n, seed, cross=None):
    """(x0, x1, c0, c1, H): dyadic sites in a small cluster inside DYADIC_NEAR -- every pair displacement is its own
    nearest image, strictly, and some are longer than the safe radius -- and the same sites each moved by its own
    integer combination of lattice vectors (counts in -2..2).  Multiples of 1/16 throughout: every candidate's squared
    length is exact in float32.  ``cross``: the number of sites of a second set c (else c is x)."""
    rng = np.random.default_rng(seed)
    H = DYADIC_NEAR

    def cluster(k):
        # a 1 x 1 x 3 column: displacements up to 3.3 < the image radius, |dz| beyond cz / 2 = 2 for one pair in nine
        x = rng.integers(0, [17, 17, 49], size=(T, k, 3)) / 16.0
        return x, x + rng.integers(-2, 3, size=(T, k, 3)).astype(np.float64) @ H

    x0, x1 = cluster(n)
    c0, c1 = (x0, x1) if cross is None else cluster(cross)
    return x0, x1, c0, c1, H


# ------------------------------------------------------------------ map validation with the nearest displacement
def mv_displacements(X, H):
    X = np.asarray(X, dtype=np.float64)
    d = wrap(X[:, :, None, :] - X[:, None, :, :], H)
    return d, (d * d).sum(-1)


def mv_energies(X, offset, width, H):
    _, x = mv_displacements(X, H)
    return np.exp(-(((x - offset) / width) ** 2)).sum(axis=(1, 2))


def mv_forces(X, offset, width, H):
    """(G (T, n, 3), its L1 scale per entry)."""
    d, x = mv_displacements(X, H)
    c = _coef(x, offset, width)
    return (c[..., None] * d).sum(axis=2), (np.abs(c)[..., None] * np.abs(d)).sum(axis=2)


def mv_proj_terms(X, F, offset, width, H):
    d, x = mv_displacements(X, H)
    t = _coef(x, offset, width) * (d * np.asarray(F, dtype=np.float64)[:, :, None, :]).sum(-1)
    return t.sum(), np.abs(t).sum()


def mv_shift_terms(X, F, offset, width, H):
    G, S = mv_forces(X, offset, width, H)
    ip, l1 = mv_proj_terms(X, F, offset, width, H)
    return (G * G).sum() - 2.0 * ip, (S * S).sum() + 2.0 * l1


def mv_random_force_proj(X, F, n_samples, seed, inner, outer, width, H, sq_args=True):
    offs, w = mref.offsets(seed, n_samples, inner, outer, width, sq_args)
    vals, scales = zip(*(mv_proj_terms(X, F, o, w, H) for o in offs))
    return np.array(vals) / np.shape(X)[0], np.array(scales) / np.shape(X)[0]


def mv_random_residual_shift(X, F, n_samples, seed, inner, outer, width, H, sq_args=True):
    offs, w = mref.offsets(seed, n_samples, inner, outer, width, sq_args)
    vals, scales = zip(*(mv_shift_terms(X, F, o, w, H) for o in offs))
    return np.array(vals) / np.size(F), np.array(scales) / np.size(F)
