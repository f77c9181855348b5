"""Helpers shared by tests/test_cell_host.py and tests/test_gpu_cell.py: the test cells, float64 / long double
restatements in NumPy (and one in torch) of the brick reduction of a displacement under a triclinic cell, the
brute-force minimum image that validates it, the magnitudes the error bounds are stated in, tie-free inputs, and a
tree-walking reference of ``make_whole`` under a cell.

A cell H is (3, 3) or (T, 3, 3): rows a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz).  Brick reduction, each line on
the updated d::

    kc = rint(dz / cz);  d -= kc c        kb = rint(dy / by);  d -= kb b        ka = rint(dx / ax);  d -= ka a

Near a tie -- a stage whose quotient lies within a margin of a half-integer -- both images are legitimate: the device
rounds d * (1 / L) in the operands' precision and reduces with fmas, the reference divides in float64.  The inputs of
the tests are built free of ties (``tie_free_sites``) with the margins of tests/pbc_ref.py, and every test asserts
``tie_distance`` of what it compares, so float32 kernels and the float64 reference pick the same integers."""
import numpy as np
import torch

from pbc_ref import MARGIN  # {float32: 1e-5, float64: 1e-11}: the rounding of a quotient at three cell lengths, with room

D = 4.3  # the edge of the dodecahedron and of the octahedron's cube


def rhombic_dodecahedron(d=D):
    return np.array([[d, 0, 0], [0, d, 0], [d / 2, d / 2, d * np.sqrt(2) / 2]])


def truncated_octahedron(d=D):
    return np.array([[d, 0, 0], [d / 3, 2 * np.sqrt(2) * d / 3, 0], [-d / 3, np.sqrt(2) * d / 3, np.sqrt(6) * d / 3]])


SKEW = np.array([[4.1, 0, 0], [-1.3, 4.7, 0], [1.7, -2.1, 5.0]])  # generic, negative off-diagonals
DIAG_LENGTHS = np.array([4.1, 4.7, 5.3])
DIAG = np.diag(DIAG_LENGTHS)


def frame_cells(T, seed=0):
    """(T, 3, 3): SKEW with every off-diagonal entry scaled by its own factor in [-1, 1] per frame (the skew changes
    sign and size from frame to frame) and the diagonal varied by a few percent."""
    rng = np.random.default_rng(7000 + seed)
    H = np.tile(SKEW, (T, 1, 1))
    for r, c in ((1, 0), (2, 0), (2, 1)):
        H[:, r, c] *= rng.uniform(-1, 1, T)
    for k in range(3):
        H[:, k, k] *= 1 + 0.03 * rng.uniform(-1, 1, T)
    return H


KINDS = ["dodecahedron", "octahedron", "skew", "frames", "diag"]


def cell_of(kind, T, seed=0):
    """The test cell ``kind``: (3, 3), or (T, 3, 3) for "frames"."""
    return {"dodecahedron": rhombic_dodecahedron, "octahedron": truncated_octahedron, "skew": lambda: SKEW,
            "diag": lambda: DIAG, "frames": lambda: frame_cells(T, seed)}[kind]()


def safe_radius(H):
    return float(np.min(np.diagonal(np.asarray(H), axis1=-2, axis2=-1))) / 2


def entries(H, d):
    """(ax, bx, by, cx, cy, cz) of H ((3, 3) or (T, 3, 3)) shaped to broadcast against the components of d (T, ..., 3)."""
    H = np.asarray(H, dtype=d.dtype if d.dtype == np.longdouble else np.float64)
    if H.ndim == 3:
        H = H.reshape((H.shape[0],) + (1,) * (d.ndim - 2) + (3, 3))
    return H[..., 0, 0], H[..., 1, 0], H[..., 1, 1], H[..., 2, 0], H[..., 2, 1], H[..., 2, 2]


# ------------------------------------------------------------------ NumPy references (inputs as stored)
def brick(d, H):
    """(image, counts, tie distance): the brick image of d (T, ..., 3) in d's dtype (float64 or long double), the counts
    (ka, kb, kc) as integers (..., 3), and the smallest |frac(q) - 1/2| over the quotients of all three stages."""
    ax, bx, by, cx, cy, cz = entries(H, d)
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    qc = d2 / cz
    kc = np.rint(qc)
    d2, d1, d0 = d2 - kc * cz, d1 - kc * cy, d0 - kc * cx
    qb = d1 / by
    kb = np.rint(qb)
    d1, d0 = d1 - kb * by, d0 - kb * bx
    qa = d0 / ax
    ka = np.rint(qa)
    d0 = d0 - ka * ax
    q = np.stack([qa, qb, qc], axis=-1)
    tie = float(np.min(np.abs(q - np.floor(q) - 0.5))) if q.size else 0.5
    return np.stack([d0, d1, d2], axis=-1), np.stack([ka, kb, kc], axis=-1).astype(np.int64), tie


def wrap(d, H):
    return brick(d, H)[0]


def tie_distance(d, H):
    return brick(d, H)[2]


def comp_bound(d, H):
    """Per component, |d| + |kc| |c| + |kb| |b| + |ka| |a|: the magnitudes the brick image is formed from."""
    ax, bx, by, cx, cy, cz = entries(H, d)
    k = np.abs(brick(d, H)[1]).astype(np.float64)
    ka, kb, kc = k[..., 0], k[..., 1], k[..., 2]
    a = np.abs(d)
    return np.stack([a[..., 0] + kc * np.abs(cx) + kb * np.abs(bx) + ka * ax, a[..., 1] + kc * np.abs(cy) + kb * by,
                     a[..., 2] + kc * cz], axis=-1)


def brute_min(d, H, reach=4):
    """The minimum image of d (M, 3) under one cell H (3, 3) by brute force over the lattice shifts in
    [-reach, reach]^3: (image (M, 3), its length (M,))."""
    r = np.arange(-reach, reach + 1)
    shifts = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3) @ np.asarray(H, dtype=np.float64)
    best, length = d.copy(), np.full(len(d), np.inf)
    for s in shifts:  # (729 passes over M displacements)
        cand = d - s
        n = np.linalg.norm(cand, axis=-1)
        better = n < length
        best[better], length[better] = cand[better], n[better]
    return best, length


def wrap_positions(x, H):
    """Positions x (T, n, 3) wrapped into the cell: fractional coordinates in [0, 1)."""
    H = np.broadcast_to(np.asarray(H, dtype=np.float64), (x.shape[0], 3, 3)) if np.ndim(H) == 2 else np.asarray(H)
    s = np.einsum("tnk,tkj->tnj", x, np.linalg.inv(H))
    return np.einsum("tnk,tkj->tnj", s - np.floor(s), H)


def tie_free_sites(make, pairs_disp, H, dtype, tries=200, margin=None):
    """The first of make(0), make(1), ... -- arrays as stored in ``dtype`` -- whose displacements ``pairs_disp(sites)``
    lie further than ``margin`` (default: twice MARGIN[dtype]) from a tie in all three stages.  Returns (sites as
    float64, tie distance)."""
    margin = 2 * MARGIN[dtype] if margin is None else margin
    for k in range(tries):
        sites = make(k)
        sites = tuple(np.asarray(torch.as_tensor(s).to(dtype).double().numpy()) for s in sites)
        tie = tie_distance(pairs_disp(*sites), H)
        if tie > margin:
            return sites, tie
    raise AssertionError("no tie-free input found")


# ------------------------------------------------------------------ the same in torch (autograd references on the CPU)
def torch_wrap(d, H):
    """Brick image of d (T, ..., 3) under H ((3, 3) or (T, 3, 3) tensor), differentiable in d (rint: no gradient)."""
    H = torch.as_tensor(H, dtype=d.dtype)
    if H.dim() == 3:
        H = H.reshape((H.shape[0],) + (1,) * (d.dim() - 2) + (3, 3))
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    kc = torch.round(d2 / H[..., 2, 2]).detach()
    d2, d1, d0 = d2 - kc * H[..., 2, 2], d1 - kc * H[..., 2, 1], d0 - kc * H[..., 2, 0]
    kb = torch.round(d1 / H[..., 1, 1]).detach()
    d1, d0 = d1 - kb * H[..., 1, 1], d0 - kb * H[..., 1, 0]
    ka = torch.round(d0 / H[..., 0, 0]).detach()
    return torch.stack([d0 - ka * H[..., 0, 0], d1, d2], dim=-1)


# ------------------------------------------------------------------ make_whole under a cell, walked along the tree
TREES = {
    "chain": lambda n: np.arange(-1, n - 1),                                     # depth n - 1
    "forest": lambda n: np.where(np.arange(n) % 7 == 0, -1, np.arange(n) - 1),   # several roots
    "backward": lambda n: np.where(np.arange(n) == n - 1, -1, np.arange(n) + 1),  # every parent follows its child
}


def molecule(tree, T, N, H, dtype, seed):
    """A random walk with steps well below the safe radius along ``tree``, wrapped into the cell, as stored in dtype."""
    par = TREES[tree](N)
    rng = np.random.default_rng(seed)
    step = 0.45 * safe_radius(H) * rng.uniform(-1, 1, (T, N, 3)) / np.sqrt(3) * 1.7
    x = np.zeros((T, N, 3))
    done = par < 0
    x[:, done] = rng.uniform(0, 4, (T, int(done.sum()), 3))
    while not done.all():
        ready = ~done & done[np.maximum(par, 0)]
        x[:, ready] = x[:, par[ready]] + step[:, ready]
        done |= ready
    w = wrap_positions(x, H)
    return torch.from_numpy(w).to(dtype).double().numpy(), par


def whole_reference(x, H, parent):
    """(u, k, tie, bound): x (T, N, 3) float64 (the inputs as stored) made whole under H along ``parent``, atom by atom
    from the roots down: n_i the counts of brick(x_i - x_parent(i)), k_i = n_i + k_parent(i) (T, N, 3; a, b, c),
    u = x - kc c - kb b - ka a evaluated in long double; the tie distance of the edge displacements; and per component
    |x| + |ka| ax + |kb| |b| + |kc| |c|, the magnitudes the bound of the coordinates is stated in."""
    T, N = x.shape[:2]
    parent = np.asarray(parent)
    has = parent >= 0
    d = x - x[:, np.maximum(parent, 0)]
    _, n, tie = brick(d[:, has], H)
    edge = np.zeros((T, N, 3), dtype=np.int64)
    edge[:, has] = n
    k = np.zeros_like(edge)
    done = ~has
    k[:, done] = 0
    while not done.all():
        ready = ~done & done[np.maximum(parent, 0)]
        assert ready.any(), "a cycle"
        k[:, ready] = edge[:, ready] + k[:, parent[ready]]
        done |= ready
    Hl = np.asarray(H, dtype=np.longdouble)
    Hl = Hl.reshape((1, 1, 3, 3)) if Hl.ndim == 2 else Hl.reshape((T, 1, 3, 3))
    kl = k.astype(np.longdouble)
    u = x.astype(np.longdouble) - np.einsum("tnk,tnkj->tnj", kl, np.broadcast_to(Hl, (T, N, 3, 3)))
    bound = np.abs(x) + np.einsum("tnk,tnkj->tnj", np.abs(k).astype(np.float64),
                                  np.abs(np.broadcast_to(Hl, (T, N, 3, 3)).astype(np.float64)))
    return u, k, tie, bound


def assert_whole(got, u, bound, dtype, what):
    """|got - u| <= 3 eps bound per component: the three roundings of the nested fmas."""
    eps = float(np.finfo(np.float32 if dtype in (torch.float32, "float32", np.float32) else np.float64).eps)
    err = np.abs(got.astype(np.longdouble) - u).astype(np.float64)
    worst = float(np.max(err / (3 * eps * bound + 1e-300))) if err.size else 0.0
    print(f"{what}: error {worst:.3g} x the 3 eps (|x| + |k| |H|) bound")
    assert worst <= 1.0, f"{what}: error {worst:.3g} x the bound"
