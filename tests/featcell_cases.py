"""Inputs shared by tests/test_feat_cell_host.py (CPU: the constructions themselves, the refusals, the plain-torch
routes) and tests/test_gpu_feat_cell.py (GPU: the cell forms of the K4 kernels, gb_feat(box=Cell) and the fused fit).
NumPy only; the references are tests/cell_ref.py (brick image) and tests/nearest_ref.py (nearest image).

Dyadic construction (checks 2 and 2b): cells ``s * DYADIC_NEAR``, s in {2, 4, 8} -- a = (8s, 0, 0), b = (0, 8s, 0),
c = (4s, 4s, 4s): every entry and every inverse of a diagonal entry is a power of two -- group means on multiples of
1/64, mapped sites on odd multiples of 1/128, lattice shifts with counts in [-2, 2].  Every coordinate, difference,
quotient, integer and fused multiply-add of the brick reduction and of the 27-candidate search is then exact in
float32 and float64, and so is the squared length of the shortest candidate (the others only have to stay longer)."""
import numpy as np

import cell_ref as R
import nearest_ref as NR
from featpbc_cases import BEADS, BONDS, CONS, MOLECULE, N_ATOMS  # noqa: F401  (the molecules of the box tests)

DYADIC_SCALES = (2.0, 4.0, 8.0)
SHAPES = [(7, 20, 3, 4), (7, 75, 2, 10)]  # tests/test_gpu_feat_pbc.py's: (T, G, n_cg, n_basis)


def rows(H, T):
    """(T, 9) float64: the row-major matrix of every frame, a constant cell expanded (``Cell.rows``)."""
    H = np.asarray(H, dtype=np.float64)
    return np.ascontiguousarray(np.broadcast_to(H, (T, 3, 3)).reshape(T, 9))


def frames_of(H, T):
    return np.broadcast_to(np.asarray(H, dtype=np.float64), (T, 3, 3))


def lattice(n, H):
    """n (T, K, 3) integer counts (i, j, k) -> i a + j b + k c per frame, (T, K, 3)."""
    return np.einsum("tkc,tcj->tkj", n.astype(np.float64), frames_of(H, n.shape[0]))


def dyadic_cell(T, per_frame):
    """``2 * DYADIC_NEAR`` (the scale at which most displacements go through the search), or one scale per frame with
    all three present."""
    if not per_frame:
        return DYADIC_SCALES[0] * NR.DYADIC_NEAR
    s = np.array([DYADIC_SCALES[t % 3] for t in range(T)])
    return s[:, None, None] * NR.DYADIC_NEAR[None]


def dyadic_groups(T, G, n_cg, per_frame, seed):
    """Check 2: Pg (T, G, 3) on multiples of 1/64 in [0, 4), cg (T, n_cg, 3) on odd multiples of 1/128 in [0, 4), the
    cell, and Pg with every (frame, group) moved by its own lattice vectors.  Every unmoved displacement has
    components below 4 <= cz / 2 (inside the brick, strictly) and is shorter than sqrt(48) = image_radius of the
    smallest cell: it is its own brick image and its own nearest image."""
    rng = np.random.default_rng(seed)
    Pg = rng.integers(0, 256, size=(T, G, 3)) / 64.0
    cg = (2 * rng.integers(0, 256, size=(T, n_cg, 3)) + 1) / 128.0
    H = dyadic_cell(T, per_frame)
    n = rng.integers(-2, 3, size=(T, G, 3))
    n[:, 0, :] = [2, -2, 1]  # (the extremes are there whatever the draw)
    return Pg, cg, H, Pg + lattice(n, H)


def outside_brick_groups(T, G, n_cg, per_frame, seed):
    """Check 2b: as ``dyadic_groups`` with every unmoved displacement OUTSIDE the brick and inside image_radius:
    |dx|, |dy| <= 1 and |dz| in (cz / 2, cz / 2 + 1].  Sites in [0, 1/2)^3, group means at x, y in [0, 1/2] and z beyond
    half the cell's height on either side."""
    rng = np.random.default_rng(seed)
    H = dyadic_cell(T, per_frame)
    cz = frames_of(H, T)[:, 2, 2][:, None]
    cg = (2 * rng.integers(0, 32, size=(T, n_cg, 3)) + 1) / 128.0            # odd multiples of 1/128 in (0, 1/2)
    Pg = rng.integers(0, 33, size=(T, G, 3)) / 64.0                             # [0, 1/2]
    up = rng.random((T, G)) < 0.5
    up[:, 0], up[:, 1] = True, False
    above = cz / 2 + 0.5 + rng.integers(0, 17, size=(T, G)) / 64.0              # dz in (cz/2, cz/2 + 3/4]
    below = -cz / 2 - rng.integers(1, 33, size=(T, G)) / 64.0                   # dz in [-cz/2 - 1, -cz/2)
    Pg[:, :, 2] = np.where(up, above, below)
    n = rng.integers(-2, 3, size=(T, G, 3))
    n[:, 0, :] = [2, -2, 1]
    return Pg, cg, H, Pg + lattice(n, H)


def displacements(Pg, cg):
    """(T, n_cg, G, 3): Pg[t, g] - cg[t, c]."""
    return Pg[:, None, :, :] - cg[:, :, None, :]


def image(d, H, near):
    """The reference image of d (T, ..., 3) in float64: cell_ref.brick or nearest_ref.nearest."""
    return NR.nearest(d, H)[0] if near else R.wrap(d, H)


def stage_ties(d, H):
    """Per element of d (T, ..., 3): the smallest distance of a quotient of the three brick stages from a half-integer
    (cell_ref.brick's tie distance, not reduced over the elements)."""
    ax, bx, by, cx, cy, cz = R.entries(H, d)
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    qc = d2 / cz
    kc = np.rint(qc)
    d1, d0 = d1 - kc * cy, d0 - kc * cx
    qb = d1 / by
    kb = np.rint(qb)
    d0 = d0 - kb * bx
    qa = d0 / ax
    q = np.stack([qa, qb, qc], axis=-1)
    return np.min(np.abs(q - np.floor(q) - 0.5), axis=-1)


# ------------------------------------------------------------------ check 3: the standard cells, sites over the whole cell
KINDS = ["dodecahedron", "dodecahedron_hex", "octahedron"]
EDGE, OUTER, TIE_STAGE = 12.0, 6.0, 1e-3


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def standard_cell(kind, T, per_frame, seed=0):
    """``nearest_ref.STANDARD[kind](12.0)`` as stored in float32: (3, 3), or (T, 3, 3) breathing by 3 % per frame."""
    H = NR.STANDARD[kind](EDGE)
    if per_frame:
        H = H[None] * (1 + 0.03 * np.random.default_rng(8000 + seed).uniform(-1, 1, T))[:, None, None]
    return f32(H)


def random_groups(kind, T, G, n_cg, per_frame, seed):
    """Group means and mapped sites uniform in the cell (fractional coordinates in [0, 1)), as stored in float32."""
    rng = np.random.default_rng(seed)
    H = standard_cell(kind, T, per_frame, seed)
    Hf = frames_of(H, T)
    Pg = f32(np.einsum("tgk,tkj->tgj", rng.random((T, G, 3)), Hf))
    cg = f32(np.einsum("tgk,tkj->tgj", rng.random((T, n_cg, 3)), Hf))
    return Pg, cg, H


def seed_of(G):
    return 11 if G == 20 else 12


def image_statistics(Pg, cg, H, near):
    """(image (T, n_cg, G, 3), mask of the triples left out, share whose image differs from the raw displacement,
    share with pick != 0): left out are the triples within 1e-3 of a tie in a brick stage and, for the nearest form,
    those whose two shortest candidates are closer than nearest_ref.TIE."""
    d = displacements(Pg, cg)
    out = stage_ties(d, H) < TIE_STAGE
    _, pick, gap = NR.nearest(d, H)
    if near:
        out = out | (gap < NR.TIE)
    img = image(d, H, near)
    return img, out, float(np.any(img != d, axis=-1).mean()), float((pick != 0).mean())


# ------------------------------------------------------------------ check 4: everything within safe_radius
def near_groups(T, G, n_cg, seed):
    """A truncated octahedron of edge 12 (safe_radius 4.9): sites and group means inside a ball of radius 2 (every
    displacement shorter than 4), the group means then moved by their own lattice vectors; float32-valued."""
    rng = np.random.default_rng(seed)
    H = standard_cell("octahedron", T, False)

    def ball(k):
        v = rng.standard_normal((T, k, 3))
        return 2.0 * rng.random((T, k, 1)) ** (1 / 3) * v / np.linalg.norm(v, axis=-1, keepdims=True)

    cg = f32(ball(n_cg) + 5.0)
    Pg = f32(ball(G) + 5.0 + lattice(rng.integers(-2, 3, size=(T, G, 3)), H))
    return Pg, cg, H


# ------------------------------------------------------------------ check 6: molecules
def wrap_into_cell(x, H):
    """Every atom of x (T, N, 3) into the brick-shaped unit cell [0, ax) x [0, by) x [0, cz) by lattice vectors, floors
    stage by stage (c first) -- exact on dyadic inputs."""
    Hf = frames_of(H, x.shape[0])[:, None]
    x = x.copy()
    for k in (2, 1, 0):
        x = x - np.floor(x[..., k] / Hf[..., k, k])[..., None] * Hf[..., k, :]
    return x


def dyadic_molecules(T, H, seed):
    """The molecules of tests/featpbc_cases.py in a dyadic cell: a compact trajectory U (T, 16, 3) on multiples of 1/64,
    molecule m in [-1, 1)^3 + (0, 0, m) -- bonds shorter than sqrt(12) < 4 = safe_radius of the smallest cell, every
    displacement below 5 in z and shorter than sqrt(33) < image_radius --, forces, ``wrapped`` = every ATOM of the moved
    trajectory wrapped into the cell (molecules split over faces) and ``moved`` = every MOLECULE moved as a whole by
    its own lattice vectors per frame."""
    rng = np.random.default_rng(seed)
    U = rng.integers(-64, 64, size=(T, N_ATOMS, 3)) / 64.0
    U[:, :, 2] += MOLECULE
    forces = 25.0 * rng.standard_normal((T, N_ATOMS, 3))
    moved = U + lattice(rng.integers(-2, 3, size=(T, 4, 3)), H)[:, MOLECULE, :]
    return U, forces, moved, wrap_into_cell(moved, H)


# connected pieces of the open tests' 14-atom system (constraint groups and beads joined): what may move together
OPEN_PIECES = [[0, 1, 2], [3], [4, 5, 6, 7], [8, 10, 12, 13], [9], [11]]


def move_pieces(coords, H, seed):
    """coords (T, 14, 3) with every piece of ``OPEN_PIECES`` moved by its own lattice vectors per frame."""
    rng = np.random.default_rng(seed)
    piece = np.zeros(coords.shape[1], dtype=np.int64)
    for k, atoms in enumerate(OPEN_PIECES):
        piece[atoms] = k
    return coords + lattice(rng.integers(-1, 2, size=(coords.shape[0], len(OPEN_PIECES), 3)), H)[:, piece, :]
