"""NumPy float64 restatement of the reference's map validation (jaxmapval.py), for tests/test_*mapval*.py.

Closed form of the squared-distance Gaussian (jaxmapval.py:365-401): with x_ij = |r_i - r_j|^2 and
g(x) = exp(-((x - o) / w)^2),  E_t = sum_{i,j} g(x_ij)  (diagonal included) and
G_i = -dE/dr_i = (8 / w^2) sum_j (x_ij - o) g(x_ij) (r_i - r_j).
The sample loops mirror random_force_proj (266-319) and random_residual_shift (159-237) one draw at a time from
``np.random.default_rng(seed)``; each also returns the L1 scale of the terms it summed (the tolerance unit).
"""
import numpy as np

_CHUNK = 2 ** 21  # frames * n * n per NumPy block


def _blocks(T, n):
    step = max(1, _CHUNK // max(1, n * n))
    for t0 in range(0, T, step):
        yield slice(t0, min(T, t0 + step))


def _pairs(X):
    d = X[:, :, None, :] - X[:, None, :, :]  # r_i - r_j
    return d, (d * d).sum(-1)


def literal_energies(X, offset, width):
    """sum_{i,j} exp(-((x_ij - o) / w)^2) per frame, the reference's expression (clipped_gauss(clip=None))."""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty(X.shape[0])
    for b in _blocks(*X.shape[:2]):
        _, x = _pairs(X[b])
        out[b] = np.exp(-(((x - offset) / width) ** 2)).sum(axis=(1, 2))
    return out


def forces(X, offset, width, scale=False):
    """Closed-form G (T, n, 3); scale=True also returns the L1 scale sum_j |(8/w^2) (x - o) g (r_i - r_j)| per entry."""
    X = np.asarray(X, dtype=np.float64)
    G = np.empty_like(X)
    S = np.empty_like(X)
    for b in _blocks(*X.shape[:2]):
        d, x = _pairs(X[b])
        c = (8.0 / width**2) * (x - offset) * np.exp(-(((x - offset) / width) ** 2))
        G[b] = (c[..., None] * d).sum(axis=2)
        S[b] = (np.abs(c)[..., None] * np.abs(d)).sum(axis=2)
    return (G, S) if scale else G


def proj_terms(X, F, offset, width):
    """(sum_t sum_i F . G, L1 scale of the pair terms)."""
    X = np.asarray(X, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    tot, l1 = 0.0, 0.0
    for b in _blocks(*X.shape[:2]):
        d, x = _pairs(X[b])
        c = (8.0 / width**2) * (x - offset) * np.exp(-(((x - offset) / width) ** 2))
        t = c * (d * F[b][:, :, None, :]).sum(-1)
        tot += t.sum()
        l1 += np.abs(t).sum()
    return tot, l1


def shift_terms(X, F, offset, width):
    """(sum |G|^2 - 2 sum F . G, L1 scale of the terms)."""
    G, S = forces(X, offset, width, scale=True)
    F = np.asarray(F, dtype=np.float64)
    ip, l1_ip = proj_terms(X, F, offset, width)
    return (G * G).sum() - 2.0 * ip, (S * S).sum() + 2.0 * l1_ip


def offsets(seed, n_samples, inner, outer, width, sq_args=True):
    """The reference's offsets: one randg.random() per sample (rsqpg_forces, jaxmapval.py:124-130)."""
    if sq_args:
        inner, outer, width = inner**2, outer**2, width**2
    rg = np.random.default_rng(seed)
    return np.array([rg.random() * (outer - inner) + inner for _ in range(n_samples)]), width


def random_force_proj(X, F, n_samples, seed, inner, outer, width, sq_args=True):
    """(per-sample projections, per-sample L1 scales), the reference loop with rsqpg_forces."""
    offs, w = offsets(seed, n_samples, inner, outer, width, sq_args)
    T = np.shape(X)[0]
    vals, scales = zip(*(proj_terms(X, F, o, w) for o in offs)) if n_samples else ((), ())
    return np.array(vals) / T, np.array(scales) / T


def random_residual_shift(X, F, n_samples, seed, inner, outer, width, sq_args=True):
    """(per-sample shifts force_smoothness(F - G) - force_smoothness(F), per-sample L1 scales)."""
    offs, w = offsets(seed, n_samples, inner, outer, width, sq_args)
    N = np.size(F)
    vals, scales = zip(*(shift_terms(X, F, o, w) for o in offs)) if n_samples else ((), ())
    return np.array(vals) / N, np.array(scales) / N


def uniform_forces_loop(F, n_samples, seed, shape, shift):
    """random_uniform_forces as the method (jaxmapval.py:30-76): per-sample values and L1 scales."""
    rg = np.random.default_rng(seed)
    F = np.asarray(F, dtype=np.float64)
    vals, scales = [], []
    for _ in range(n_samples):
        v = 2 * rg.random(size=3) - 1
        v = v / np.sqrt((v**2).sum())
        G = np.broadcast_to(v, shape)
        if shift:
            vals.append(((G * G).sum() - 2.0 * (F * G).sum()) / F.size)
            scales.append(((G * G).sum() + 2.0 * np.abs(F * G).sum()) / F.size)
        else:
            vals.append((F * G).sum() / shape[0])
            scales.append(np.abs(F * G).sum() / shape[0])
    return np.array(vals), np.array(scales)
