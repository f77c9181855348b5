"""Helpers shared by tests/test_pairlist_host.py and tests/test_gpu_pairlist.py: the list kinds the tests use, a
brute-force build of the incidence tables, float64 NumPy restatements of the K9c / K9d kernels with the per-entry sum
of |terms| their error bounds are stated in, and the two kernels restated in torch for the CPU tests."""
import numpy as np
import torch

import aggforce_amd._kernels as K


def lattice_sites(T, n, seed):
    """Sites on a 1.5-spaced lattice with 0.3 of seeded noise per frame (bench.py's synthetic recipe)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1 / 3)))
    while side**3 < n:
        side += 1
    a = np.arange(n)
    lat = 1.5 * np.stack([a % side, (a // side) % side, a // side**2], axis=1)
    return lat[None] + 0.3 * rng.standard_normal((T, n, 3))


# ------------------------------------------------------------------ list kinds: (P, 2) int64 rows (i, j)
def triangle(n):
    return np.stack(np.triu_indices(n, k=1), axis=1).astype(np.int64)


def chain(n):
    a = np.arange(n - 1, dtype=np.int64)
    return np.stack([a, a + 1], axis=1)


def star(n):
    a = np.arange(1, n, dtype=np.int64)
    return np.stack([np.zeros_like(a), a], axis=1)


def random_list(P, m, n, seed, self_form=True):
    """P random pairs with repeats, (in the self form) pairs i == j, and the last site of each side in no pair."""
    rng = np.random.default_rng(seed)
    pairs = np.stack([rng.integers(0, max(m - 1, 1), P), rng.integers(0, max(n - 1, 1), P)], axis=1).astype(np.int64)
    if P >= 3:
        pairs[P // 2] = pairs[0]  # a repeat
        if self_form:
            pairs[P - 1, 1] = pairs[P - 1, 0]  # a self pair
    return pairs


def brute_tables(pairs, n_rows, n_sites):
    """(ptr, idx) by j and by i, built site by site."""
    out = []
    for col, count in ((1, n_sites), (0, n_rows)):
        ptr, idx = [0], []
        for s in range(count):
            idx += [p for p in range(len(pairs)) if pairs[p, col] == s]
            ptr.append(len(idx))
        out.append((np.array(ptr), np.array(idx, dtype=np.int64)))
    return out


# ------------------------------------------------------------------ float64 NumPy references (inputs as stored)
def list_disp(x, c, pairs):
    """u[t,p] = x[t,j_p] - c[t,i_p]."""
    return x[:, pairs[:, 1]] - c[:, pairs[:, 0]]


def pull_reference(w, u, pairs, m, n):
    """(A, B, bound of A, bound of B): the two sums and the sums of |terms|."""
    T = u.shape[0]
    q = w[..., None] * u
    aq = np.abs(w)[..., None] * np.abs(u)
    A, B, Ab, Bb = (np.zeros((T, k, 3)) for k in (n, m, n, m))
    for t in range(T):
        np.add.at(A[t], pairs[:, 1], q[t])
        np.add.at(B[t], pairs[:, 0], -q[t])
        np.add.at(Ab[t], pairs[:, 1], aq[t])
        np.add.at(Bb[t], pairs[:, 0], aq[t])
    return A, B, Ab, Bb


# ------------------------------------------------------------------ the two kernels in torch (CPU tests)
def fake_pair_list_dist(x, c, tab, mode=K.PAIR_DIST, v=None, y=None):
    assert x.dtype == c.dtype and x.is_contiguous() and c.is_contiguous()
    i, j = tab.pairs[:, 0].long(), tab.pairs[:, 1].long()
    u = x[:, j] - c[:, i]
    if mode == K.PAIR_DOT:
        assert v.dtype == x.dtype == y.dtype
        return ((v[:, j] - y[:, i]) * u).sum(-1)
    s = (u * u).sum(-1)
    return s if mode == K.PAIR_SQDIST else s.sqrt()


def fake_pair_list_pull(w, x, c, tab, dv=None, want_a=True, want_b=True, out_dtype=None):
    assert w.dtype == x.dtype == c.dtype and (dv is None or dv.dtype == w.dtype)
    out_dtype = out_dtype or x.dtype
    assert not (x.dtype == torch.float32 and out_dtype == torch.float64)
    i, j = tab.pairs[:, 0].long(), tab.pairs[:, 1].long()
    if dv is not None:
        w = torch.where(dv > 0, w / dv, torch.zeros_like(w))
    q = w[..., None] * (x[:, j] - c[:, i])
    a = torch.zeros_like(x).index_add_(1, j, q).to(out_dtype) if want_a else None
    b = torch.zeros_like(c).index_add_(1, i, -q).to(out_dtype) if want_b else None
    return a, b
