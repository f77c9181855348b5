"""NumPy float64 restatement of map validation under periodic boundaries, for tests/test_*mapval_pbc*.py: that of
tests/mapval_ref.py with every displacement r_i - r_j replaced by its image d_ij under the frame's box or cell.

x_ij = |d_ij|^2, g(x) = exp(-((x - o) / w)^2), E_t = sum_{i,j} g(x_ij) (the diagonal is d = 0) and
G_i = (8 / w^2) sum_j (x_ij - o) g(x_ij) d_ij.  ``box`` is what the periodic functions are given, as NumPy: the lengths
of an orthorhombic box, (3,) or (T, 3) -- the minimum image, ``featpbc_cases.min_image`` -- or ``Cell``-like vectors
wrapped in ``Tri``: (3, 3) or (T, 3, 3) -- the brick image, ``cell_ref.brick``.  Every sum returns its L1 scale too, the
unit of the tolerances, as the open restatement does."""
import numpy as np

import cell_ref
import mapval_ref as ref
from featpbc_cases import min_image


class Tri:
    """Marks lattice vectors ((3, 3) or (T, 3, 3)): a raw (T, 3) array is the lengths of a box."""

    def __init__(self, vectors):
        self.vectors = np.asarray(vectors, dtype=np.float64)


def displacements(X, box):
    """(d (T, n, n, 3): the image of r_i - r_j, x = |d|^2, whether the image differs from r_i - r_j (T, n, n))."""
    X = np.asarray(X, dtype=np.float64)
    raw = X[:, :, None, :] - X[:, None, :, :]
    if isinstance(box, Tri):
        d, counts, _ = cell_ref.brick(raw, box.vectors)
        moved = (counts != 0).any(-1)
    else:
        L = np.asarray(box, dtype=np.float64)
        L = np.broadcast_to(L if L.ndim == 1 else L[:, None, None, :], raw.shape)
        d = min_image(raw, L, np.float64)
        moved = (d != raw).any(-1)
    return d, (d * d).sum(-1), moved


def _coef(x, offset, width):
    return (8.0 / width**2) * (x - offset) * np.exp(-(((x - offset) / width) ** 2))


def literal_energies(X, offset, width, box):
    _, x, _ = displacements(X, box)
    return np.exp(-(((x - offset) / width) ** 2)).sum(axis=(1, 2))


def forces(X, offset, width, box, scale=False):
    """Closed-form G (T, n, 3); scale=True also returns the L1 scale sum_j |(8/w^2) (x - o) g d| per entry."""
    d, x, _ = displacements(X, box)
    c = _coef(x, offset, width)
    G = (c[..., None] * d).sum(axis=2)
    return (G, (np.abs(c)[..., None] * np.abs(d)).sum(axis=2)) if scale else G


def proj_terms(X, F, offset, width, box):
    """(sum_t sum_i F . G, L1 scale of the pair terms)."""
    d, x, _ = displacements(X, box)
    t = _coef(x, offset, width) * (d * np.asarray(F, dtype=np.float64)[:, :, None, :]).sum(-1)
    return t.sum(), np.abs(t).sum()


def shift_terms(X, F, offset, width, box):
    """(sum |G|^2 - 2 sum F . G, L1 scale of the terms)."""
    G, S = forces(X, offset, width, box, scale=True)
    ip, l1_ip = proj_terms(X, F, offset, width, box)
    return (G * G).sum() - 2.0 * ip, (S * S).sum() + 2.0 * l1_ip


def random_force_proj(X, F, n_samples, seed, inner, outer, width, box, sq_args=True):
    """(per-sample projections, per-sample L1 scales): the reference loop, the offsets of the open path."""
    offs, w = ref.offsets(seed, n_samples, inner, outer, width, sq_args)
    vals, scales = zip(*(proj_terms(X, F, o, w, box) for o in offs))
    return np.array(vals) / np.shape(X)[0], np.array(scales) / np.shape(X)[0]


def random_residual_shift(X, F, n_samples, seed, inner, outer, width, box, sq_args=True):
    offs, w = ref.offsets(seed, n_samples, inner, outer, width, sq_args)
    vals, scales = zip(*(shift_terms(X, F, o, w, box) for o in offs))
    return np.array(vals) / np.size(F), np.array(scales) / np.size(F)
