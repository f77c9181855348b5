"""Inputs shared by tests/test_feat_pbc_host.py (CPU: the constructions themselves) and tests/test_gpu_feat_pbc.py
(GPU: the box forms of the K4 kernels, gb_feat(box=) and the fused fit).  NumPy only.

Dyadic construction: coordinates are multiples of 1/128 in [0, 4) (group means on multiples of 1/64, mapped sites on
the odd multiples of 1/128 between them, so no distance is zero), box lengths are powers of two >= 8, and a (frame,
group) is moved by its own integer multiples of the box lengths, -2..2 per component.  Every quantity is then exact in
float32 and float64: the shifted coordinate (below 4 + 2 * 64 at a resolution of 1/128 needs 15 bits), the difference d,
d * (1 / L), the integer rint recovers and the fma that takes it out again.  Every component of every unshifted
displacement is below 4 <= L / 2 in magnitude: no tie, and the minimum image IS the unshifted displacement, bit for bit.
"""
import numpy as np

BOX_CHOICES = np.array([8.0, 16.0, 32.0, 64.0])


def dyadic_box(T, per_frame, rng):
    """(3,) with three different lengths, or (T, 3) whose rows differ between frames and components."""
    if not per_frame:
        return np.array([8.0, 32.0, 16.0])
    box = BOX_CHOICES[rng.integers(0, 4, size=(T, 3))]
    box[0] = [8.0, 16.0, 64.0]
    box[1 % T] = [32.0, 8.0, 16.0]
    return box


def dyadic_groups(T, G, n_cg, per_frame, seed):
    """Pg (T, G, 3), cg (T, n_cg, 3), box, and Pg with every (frame, group) moved by its own box vectors; float64
    arrays whose values are exact in float32."""
    rng = np.random.default_rng(seed)
    Pg = rng.integers(0, 256, size=(T, G, 3)) / 64.0
    cg = (2 * rng.integers(0, 256, size=(T, n_cg, 3)) + 1) / 128.0
    box = dyadic_box(T, per_frame, rng)
    n = rng.integers(-2, 3, size=(T, G, 3)).astype(np.float64)
    n[:, 0, :] = [2.0, -2.0, 1.0]  # (the extremes are there whatever the draw)
    rows = box[:, None, :] if per_frame else box[None, None, :]
    return Pg, cg, box, Pg + n * rows


def min_image(d, L, dtype):
    """The kernels' wrap in NumPy arithmetic of ``dtype``: k = rint(d * (1 / L)), d - k L (one rounding each; exact
    on the dyadic inputs, where the fused and the unfused last step agree)."""
    d, L = d.astype(dtype), L.astype(dtype)
    k = np.rint(d * (dtype(1) / L))
    return d - k * L


def random_groups(T, G, n_cg, per_frame, seed):
    """Group means and mapped sites spread over the whole cell, so that many displacements have a nearer image:
    float32-valued float64 arrays Pg, cg and box ((3,) or (T, 3), lengths that differ per component and frame)."""
    rng = np.random.default_rng(seed)
    box = np.array([5.0, 6.5, 8.0]) if not per_frame else np.array([5.0, 6.5, 8.0]) + 1.5 * rng.random((T, 3))
    box = box.astype(np.float32).astype(np.float64)
    rows = box[:, None, :] if per_frame else box[None, None, :]
    Pg = (rng.random((T, G, 3)) * rows).astype(np.float32).astype(np.float64)
    cg = (rng.random((T, n_cg, 3)) * rows).astype(np.float32).astype(np.float64)
    return Pg, cg, box


def image_statistics(Pg, cg, box):
    """(d_mi (T, n_cg, G, 3) float64 minimum-image displacements d - L rint(d / L), share of (frame, site, group)
    triples with a component beyond half a box length, mask of the triples within 1e-3 of a tie in d / L)."""
    rows = box[:, None, None, :] if box.ndim == 2 else box[None, None, None, :]
    d = Pg[:, None, :, :] - cg[:, :, None, :]
    q = d / rows
    d_mi = d - rows * np.rint(q)
    moved = np.any(np.abs(d) > rows / 2, axis=-1)
    near_tie = np.any(np.abs(np.abs(q - np.floor(q)) - 0.5) < 1e-3, axis=-1)
    return d_mi, float(moved.mean()), near_tie


# ---- molecules: 4 molecules of 4 atoms, chains; two-atom constraint groups and two-atom beads inside molecules
N_ATOMS = 16
BONDS = np.array([[4 * m + i, 4 * m + i + 1] for m in range(4) for i in range(3)])
CONS = {frozenset([0, 1]), frozenset([5, 6]), frozenset([10, 11]), frozenset([12, 13])}
BEADS = [[0, 2], [4, 7], [8, 9], [13, 15]]  # (no bead sits on a group mean: r > 0)
MOLECULE = np.repeat(np.arange(4), 4)


def dyadic_molecules(T, per_frame, seed):
    """A compact trajectory U (T, 16, 3) on multiples of 1/64 in [-2, 2) (every displacement below 4 <= L / 2),
    forces, a dyadic box, ``wrapped`` = every ATOM of U wrapped into [0, L) (molecules that straddle the origin are
    split over faces), and ``moved`` = U with every MOLECULE moved as a whole by its own box vectors per frame."""
    rng = np.random.default_rng(seed)
    U = rng.integers(-128, 128, size=(T, N_ATOMS, 3)) / 64.0
    forces = 25.0 * rng.standard_normal((T, N_ATOMS, 3))
    box = dyadic_box(T, per_frame, rng)
    rows = box[:, None, :] if per_frame else box[None, None, :]
    wrapped = U - rows * np.floor(U / rows)
    n = rng.integers(-2, 3, size=(T, 4, 3)).astype(np.float64)
    moved = U + n[:, MOLECULE, :] * rows
    return U, forces, box, wrapped, moved
