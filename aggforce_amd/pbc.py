"""Whole molecules under a periodic box (not in the reference).

A trajectory that is wrapped into an orthorhombic cell splits every molecule that straddles a face: its atoms sit a
box length apart, and whatever averages them -- a centre-of-mass ``coord_map``, the group means and mapped sites of
``gb_feat`` -- is off by a box length in those frames.  ``make_whole`` undoes that the standard way (``gmx trjconv -pbc
whole``): along a spanning forest of the bond graph every atom is put at the minimum image of its parent, so each
molecule comes out in one piece around its root, which does not move.  ``project_forces(..., box=, bonds=)`` applies it
once to the coordinates before anything else sees them.

Per frame and Cartesian component, in the coordinates' dtype (the roundings of the minimum image of the pair kernels)::

    n_i = 0 for a root, else (int) rint((x_i - x_parent(i)) / L)      from the input alone
    k_i = n_i + the n of all ancestors of i                          an exact integer sum
    u_i = x_i - k_i L

The sums along the root paths are formed by pointer jumping over ``MoleculeTree.jumps`` (``jumps[r][i]``: the 2^r-th
ancestor of i), ``n_rounds`` rounds for any tree: GPU tensors run on the K11 kernels (``csrc/aggf_whole.hip``), CPU
tensors and NumPy arrays on a NumPy body with the same arithmetic (NumPy has no fma: ``x - k L`` is formed in the next
wider type and narrowed, which can differ from the kernel's single rounding in the last bit; the image counts are the
same integers).

Bonds must be shorter than half the box in every component for the minimum image to be the bonded image; that is
not checked.  Distances BETWEEN molecules are the featuriser's part: ``gb_feat(..., box=)`` measures minimum-image
distances from a mapped site to the (whole) constraint groups, and takes its box through its own binding::

    project_forces(coords, forces, cmap, box=B, bonds=bonds, method=qp_feat_linear_map,
                   featurizer=Multifeaturize([id_feat, Curry(gb_feat, outer=..., box=B)]), ...)

Its group means and mapped sites are plain averages: they are right because ``bonds=`` made the groups and beads whole.
Triclinic cells: ``box=Cell(vectors)`` (``Cell``, below and ``_cell.py``: three lattice vectors a, b, c as the rows of
a lower-triangular matrix).  Every function that takes the lengths of a box here takes a ``Cell`` -- ``make_whole``,
``jaxutil.pair_distances`` / ``distances_in_box`` / ``min_distances``, ``PairList.from_cutoff``,
``guess_pairwise_constraints``, ``project_forces(..., box=, bonds=)`` and ``project_forces_grid_cv`` -- on the triclinic
forms of the same kernels.  The image of a displacement is its brick reduction (``_cell``): the true minimum image up to
``Cell.safe_radius = min(ax, by, cz) / 2``, a periodic image that is never shorter than it beyond.  For ``make_whole``::

    n_i = (ka, kb, kc), the three counts of the brick reduction of x_i - x_parent(i)   (0 for a root)
    k_i = n_i + the n of all ancestors of i                                            integer triples sum exactly
    u_i = x_i - kc c - kb b - ka a                                                     nested fmas in that order

and the image counts (T, N, 3) are those of a, b, c in that order.  Bonds must be shorter than ``safe_radius``.

``Cell(vectors, images="nearest")``: the pair-distance, cutoff-list and map-validation functions then take the shortest
of the brick image's 27 translates -- for a reduced cell the true minimum image up to ``Cell.image_radius``, half the
shortest lattice vector (0.5 d in a rhombic dodecahedron or truncated octahedron of image distance d, where
``safe_radius`` is 0.354 d to 0.408 d): ``_cell``.  ``make_whole``, ``guess_pairwise_constraints``,
``project_forces(..., box=, bonds=)`` and ``project_forces_grid_cv`` accept such a cell and run their brick forms: they
measure bonds and rigid pairs, which must be shorter than ``safe_radius`` anyway, and there the two images coincide.

Map validation (``jaxmapval``) under a box: ``random_force_proj(..., box=B)`` and ``random_residual_shift(..., box=B)``
take the fused periodic path; the single-field functions that take a box are here, ``sq_gaussian_energies``,
``sq_gaussian_forces`` and ``rsqpg_forces`` (``jaxmapval`` keeps the reference's signatures, which have no box).

Out of scope: unwrapping across time (jumps between frames), minimum-image group means, ``aggforce_amd.stream`` for
host trajectories (it takes no box); under a ``Cell`` also ``gb_feat`` (refused) and ``comm=`` (refused).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _kernels as K
from . import mapval as _mv
from ._cell import Cell, cell_good, is_cell_rows, is_nearest  # noqa: F401  (Cell: part of this module's surface)
from .jaxutil import PairList, _as_box

MAX_DEPTH = 1 << 16  # a forest this deep is refused: the int32 image counts of K11 cannot overflow below it
_MAX_EDGE = 1 << 15  # |n_i| is clamped to this before summing


def _ranges(starts: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """The concatenation of arange(s, s + c) over the rows of (starts, counts)."""
    total = int(counts.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    ends = np.cumsum(counts)
    return np.arange(total, dtype=np.int64) - np.repeat(ends - counts, counts) + np.repeat(starts, counts)


class MoleculeTree:
    """A spanning forest over ``n_sites`` atoms, validated on the host once: ``parent`` (n_sites,) integers in
    [-1, n_sites), -1 marking a root; a parent may have a larger index than its children.  Refused: an index out of
    range, a cycle, a depth of 2^16 or more (``ValueError``).

    ``depth``: the longest root path in edges (0 for a forest of roots); ``n_rounds``: the smallest R with
    2^R >= depth; ``jumps`` (R, n_sites) int32: ``jumps[r][i]`` the 2^r-th ancestor of i or -1; ``pairs``: the
    (child, parent) edges as a ``PairList``.  The device tables are built on first use, once per device."""

    def __init__(self, parent):
        if isinstance(parent, torch.Tensor):
            if parent.dtype.is_floating_point or parent.dtype.is_complex or parent.dtype == torch.bool:
                raise ValueError(f"parent must hold integers; got {parent.dtype}")
            arr = parent.detach().cpu().numpy()
        else:
            arr = np.asarray(parent)
            if arr.size == 0:
                arr = arr.astype(np.int64)
        if arr.dtype.kind not in "iu":
            raise ValueError(f"parent must hold integers; got {arr.dtype}")
        if arr.ndim != 1:
            raise ValueError(f"parent must have shape (n_sites,); got {arr.shape}")
        n = int(arr.shape[0])
        if n > np.iinfo(np.int32).max:
            raise ValueError("a molecule tree is limited to 2^31 - 1 sites")
        if arr.dtype == np.uint64 and arr.size and int(arr.max()) > np.iinfo(np.int64).max:
            raise ValueError("parent holds an index beyond the int64 range")
        par = np.array(arr, dtype=np.int64)
        bad = (par < -1) | (par >= n)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"parent[{i}] = {par[i]} is out of range: a parent is in [-1, {n})")
        # levels from the roots down: whatever they do not reach hangs on a cycle
        order = np.argsort(par, kind="stable")
        first = np.searchsorted(par[order], np.arange(n + 1))  # children of p: order[first[p]:first[p + 1]]
        level = np.full(n, -1, dtype=np.int64)
        frontier = np.flatnonzero(par == -1)
        depth = 0
        while frontier.size:
            level[frontier] = depth
            frontier = order[_ranges(first[frontier], first[frontier + 1] - first[frontier])]
            if frontier.size:
                depth += 1
                if depth >= MAX_DEPTH:
                    raise ValueError(f"the forest is {MAX_DEPTH} or more bonds deep: beyond what make_whole sums")
        if (level < 0).any():
            i = int(np.argmax(level < 0))
            raise ValueError(f"parent holds a cycle: site {i} (parent {par[i]}) has no root")
        self.n_sites = n
        self.depth = depth
        self.n_rounds = 0 if depth <= 1 else int(depth - 1).bit_length()
        par.setflags(write=False)
        self._parent = par
        level.setflags(write=False)
        self._level = level
        jumps = np.empty((self.n_rounds, n), dtype=np.int32)
        anc = par
        for r in range(self.n_rounds):
            jumps[r] = anc
            anc = np.where(anc >= 0, anc[np.maximum(anc, 0)], -1)
        jumps.setflags(write=False)
        self._jumps = jumps
        self._pairs = None
        self._devices: dict = {}

    @classmethod
    def from_bonds(cls, n_sites: int, bonds) -> "MoleculeTree":
        """The spanning forest of a bond graph: breadth first from the lowest index of every connected component
        (that site is the root; neighbours are visited in ascending index).  ``bonds``: a (k, 2) integer array or a
        ``PairList`` over ``n_sites`` sites.  Ring-closing and repeated bonds are dropped, sites without bonds are
        roots; a bond of a site to itself or an index outside [0, n_sites) raises ``ValueError`` naming the row."""
        n = int(n_sites)
        if n < 0:
            raise ValueError(f"negative number of sites: {n_sites}")
        if isinstance(bonds, PairList):
            if bonds.n_cross is not None or bonds.n_sites != n:
                raise ValueError(f"bonds: a pair list over {bonds.n_sites} sites (n_cross {bonds.n_cross}) for "
                                 f"{n} sites")
            b = bonds.pairs
        else:
            arr = bonds.detach().cpu().numpy() if isinstance(bonds, torch.Tensor) else np.asarray(bonds)
            if arr.size == 0:
                arr = np.zeros((0, 2), dtype=np.int64)
            if arr.dtype.kind not in "iu":
                raise ValueError(f"bonds must be integers; got {arr.dtype}")
            if arr.ndim != 2 or arr.shape[1] != 2:
                raise ValueError(f"bonds must have shape (n_bonds, 2); got {arr.shape}")
            b = arr.astype(np.int64)
        bad = (b < 0).any(axis=1) | (b >= n).any(axis=1)
        if bad.any():
            row = int(np.argmax(bad))
            raise ValueError(f"bonds row {row} = ({b[row, 0]}, {b[row, 1]}) is out of range: sites are in [0, {n})")
        selfb = b[:, 0] == b[:, 1]
        if selfb.any():
            row = int(np.argmax(selfb))
            raise ValueError(f"bonds row {row} = ({b[row, 0]}, {b[row, 1]}) bonds a site to itself")
        # adjacency (both directions), neighbours ascending
        src = np.concatenate([b[:, 0], b[:, 1]])
        dst = np.concatenate([b[:, 1], b[:, 0]])
        order = np.lexsort((dst, src))
        nbr = dst[order]
        first = np.searchsorted(src[order], np.arange(n + 1))
        parent = np.full(n, -1, dtype=np.int64)
        seen = np.zeros(n, dtype=bool)
        for root in np.flatnonzero(first[1:] > first[:-1]):  # (a site without bonds stays a root)
            if seen[root]:
                continue
            seen[root] = True
            frontier = np.array([root], dtype=np.int64)
            while frontier.size:
                counts = first[frontier + 1] - first[frontier]
                cand = nbr[_ranges(first[frontier], counts)]
                via = np.repeat(frontier, counts)
                fresh = ~seen[cand]
                cand, via = cand[fresh], via[fresh]
                cand, idx = np.unique(cand, return_index=True)  # (a site reached twice in a level: its first finder)
                parent[cand] = via[idx]
                seen[cand] = True
                frontier = cand
        return cls(parent)

    @property
    def parent(self) -> np.ndarray:
        return self._parent

    @property
    def jumps(self) -> np.ndarray:
        return self._jumps

    @property
    def level(self) -> np.ndarray:
        """(n_sites,) the number of bonds between each site and its root."""
        return self._level

    @property
    def pairs(self) -> PairList:
        if self._pairs is None:
            child = np.flatnonzero(self._parent >= 0)
            self._pairs = PairList(np.stack([child, self._parent[child]], axis=1), self.n_sites)
        return self._pairs

    def on(self, device) -> "K.TreeTables":
        """The forest on ``device`` (cached): see ``_kernels.TreeTables``."""
        device = torch.device(device)
        if device not in self._devices:
            put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            self._devices[device] = K.TreeTables(put(self._parent.astype(np.int32)), put(self._jumps))
        return self._devices[device]


def as_tree(bonds, n_sites: int) -> MoleculeTree:
    """``bonds`` as a ``MoleculeTree`` over ``n_sites`` sites: a tree as it is, a ``PairList`` or a (k, 2) integer
    array through ``MoleculeTree.from_bonds``."""
    tree = bonds if isinstance(bonds, MoleculeTree) else MoleculeTree.from_bonds(n_sites, bonds)
    if tree.n_sites != int(n_sites):
        raise ValueError(f"a molecule tree over {tree.n_sites} sites for coordinates of {n_sites} sites")
    return tree


def _host_whole(x: np.ndarray, box: np.ndarray, tree: MoleculeTree):
    """The NumPy body: (u, k) for x (T, N, 3) float32/float64 and box (3,) or (T, 3) in x's dtype."""
    dt = x.dtype.type
    T, N = x.shape[0], x.shape[1]
    L = np.broadcast_to(box.reshape(-1, 1, 3), (box.reshape(-1, 3).shape[0], 1, 3)).astype(x.dtype)
    with np.errstate(all="ignore"):
        good = (L > 0) & np.isfinite(L)
        L = np.where(good, L, dt(np.nan))
        invL = dt(1) / L
        par = tree.parent
        has = par >= 0
        q = (x - x[:, np.maximum(par, 0)]) * invL
        r = np.clip(np.rint(q), -_MAX_EDGE, _MAX_EDGE)
        n = np.where(np.isfinite(q) & has[None, :, None], r, 0).astype(np.int32)
        k = n
        for jr in tree.jumps:
            k = k + np.where((jr >= 0)[None, :, None], k[:, np.maximum(jr, 0)], 0)
        # x - k L rounded once, as the kernel's fma does: the product and difference in a wider type
        wide = np.float64 if x.dtype == np.float32 else np.longdouble
        u = (x.astype(wide) - k.astype(x.dtype).astype(wide) * L.astype(wide)).astype(x.dtype)
    return u.reshape(T, N, 3), np.ascontiguousarray(k, dtype=np.int32).reshape(T, N, 3)


def _host_whole_cell(x: np.ndarray, rows: np.ndarray, tree: MoleculeTree):
    """The NumPy body under a triclinic cell: (u, k) for x (T, N, 3) float32/float64 and rows (T, 9) in x's dtype, with
    the arithmetic of K11's triclinic form (each fma as a product and sum in the next wider type, narrowed once)."""
    dt = x.dtype.type
    T, N = x.shape[0], x.shape[1]
    wide = np.float64 if x.dtype == np.float32 else np.longdouble
    with np.errstate(all="ignore"):
        good = cell_good(torch.from_numpy(np.ascontiguousarray(rows))).numpy()
        h = np.where(good[:, None], rows, dt(np.nan)).astype(x.dtype).reshape(T, 1, 9)
        ax, bx, by, cx, cy, cz = (h[..., k] for k in (0, 3, 4, 6, 7, 8))
        iax, iby, icz = dt(1) / ax, dt(1) / by, dt(1) / cz
        par = tree.parent
        has = par >= 0
        d = x - x[:, np.maximum(par, 0)]

        def count(q):
            r = np.clip(np.rint(q), -_MAX_EDGE, _MAX_EDGE)
            return np.where(np.isfinite(q), r, 0).astype(x.dtype)

        def fnma(k, c, v):  # fma(-k, c, v), rounded once
            return (v.astype(wide) - k.astype(wide) * c.astype(wide)).astype(x.dtype)

        d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
        kc = count(d2 * icz)
        d1, d0 = fnma(kc, cy, d1), fnma(kc, cx, d0)
        kb = count(d1 * iby)
        d0 = fnma(kb, bx, d0)
        ka = count(d0 * iax)
        n = np.where(has[None, :, None], np.stack([ka, kb, kc], axis=-1), 0).astype(np.int32)
        k = n
        for jr in tree.jumps:
            k = k + np.where((jr >= 0)[None, :, None], k[:, np.maximum(jr, 0)], 0)
        fa, fb, fc = (k[..., c].astype(x.dtype) for c in range(3))
        u0 = fnma(fa, ax, fnma(fb, bx, fnma(fc, cx, x[..., 0])))
        u1 = fnma(fb, by, fnma(fc, cy, x[..., 1]))
        u2 = fnma(fc, cz, x[..., 2])
        u = np.stack([u0, u1, u2], axis=-1)
    return u.reshape(T, N, 3), np.ascontiguousarray(k, dtype=np.int32).reshape(T, N, 3)


def make_whole(xyz, box, tree, *, inplace: bool = False, return_images: bool = False):
    """``xyz`` (n_steps, n_sites, 3) with every molecule of ``tree`` made whole under ``box``: each atom at the
    minimum image of its parent in the forest, roots where they are (see the module's text for the arithmetic).

    ``box``: the lengths of an orthorhombic cell, (3,) or (n_steps, 3), as everywhere (``jaxutil``): a box on the host
    is checked, a box on a GPU is not -- a length that is not positive and finite makes its frame's coordinates NaN
    (image counts 0) and no other frame's.  A ``Cell`` (with either setting of ``images``: bonds must be shorter than
    ``safe_radius``, where the nearest image is the brick image): a triclinic cell -- every atom at the brick image of its
    parent, the image counts those of a, b, c in that order (the module's text), a bad frame NaN in every
    component.  ``tree``: a ``MoleculeTree`` (or bonds: a ``PairList`` / (k, 2) array,
    turned into one).  A non-finite coordinate stays where it is and moves nothing else.

    NumPy in gives NumPy out, a tensor gives a tensor on its device, in the input's dtype (float32 / float64; anything
    else is computed and returned in float64).  GPU tensors run on K11; one that requires a gradient goes through
    ``_autograd.MakeWhole``, whose backward is the identity (the shift is piecewise constant).  ``inplace``: write into
    ``xyz`` itself (a contiguous float32 / float64 array that does not require a gradient) and return it.
    ``return_images``: return ``(whole, images)``, images (n_steps, n_sites, 3) int32: the box lengths each atom was
    moved back by."""
    shape = tuple(xyz.shape) if hasattr(xyz, "shape") else np.shape(xyz)
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"xyz must have shape (n_steps, n_sites, 3); got {shape}")
    tree = as_tree(tree, shape[1])
    box = _as_box(box, shape[0])
    is_tensor = isinstance(xyz, torch.Tensor)
    if is_tensor and xyz.requires_grad and inplace:
        raise ValueError("make_whole: inplace=True with a tensor that requires a gradient")
    if is_tensor and xyz.is_cuda:
        x = xyz if xyz.dtype in (torch.float32, torch.float64) else xyz.to(torch.float64)
        if inplace and (x is not xyz or not xyz.is_contiguous()):
            raise ValueError("make_whole: inplace=True needs a contiguous float32 or float64 tensor")
        K.lib()
        b = box.to(device=x.device, dtype=x.dtype).contiguous()
        if x.requires_grad and torch.is_grad_enabled():
            from ._autograd import MakeWhole

            images = torch.empty(shape, dtype=torch.int32, device=x.device) if return_images else None
            out = MakeWhole.apply(x, b, tree, K.WHOLE_AUTO, images)
            return (out, images) if return_images else out
        xc = x.detach().contiguous()
        images = torch.empty(shape, dtype=torch.int32, device=x.device) if return_images else None
        out = K.make_whole(xc, b, tree.on(x.device), out=xc if inplace else None, images=images)
        out = xyz if inplace else out
        return (out, images) if return_images else out
    # the host body
    if is_tensor:
        x = xyz.detach()
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        arr = x.numpy()
    else:
        arr = np.asarray(xyz)
        if arr.dtype not in (np.float32, np.float64):
            arr = arr.astype(np.float64)
    if inplace and not _float_array(xyz):
        raise ValueError("make_whole: inplace=True needs a float32 or float64 array")
    host = _host_whole_cell if is_cell_rows(box) else _host_whole
    u, k = host(arr, box.detach().cpu().numpy().astype(arr.dtype), tree)
    if is_tensor:
        images = torch.from_numpy(k)
        if inplace:
            out = xyz.copy_(torch.from_numpy(u))
        elif xyz.requires_grad and torch.is_grad_enabled():
            out = _HostWhole.apply(xyz, torch.from_numpy(u))
        else:
            out = torch.from_numpy(u)
    else:
        images = k
        if inplace:
            xyz[...] = u
        out = xyz if inplace else u
    return (out, images) if return_images else out


def _float_array(a) -> bool:
    """A float32 or float64 NumPy array or tensor (what ``inplace`` can write into)."""
    if isinstance(a, torch.Tensor):
        return a.dtype in (torch.float32, torch.float64)
    return isinstance(a, np.ndarray) and a.dtype in (np.float32, np.float64)


class _HostWhole(torch.autograd.Function):
    """The host body's result with the identity backward of ``_autograd.MakeWhole`` (CPU tensors)."""

    @staticmethod
    def forward(ctx, x, whole):
        return whole.view_as(whole)

    @staticmethod
    def backward(ctx, H):
        return H, None


# ------------------------------------------------------------------ map validation under a box (mapval.py, K7)
def _mapval_inputs(positions, width, box, outer=None, sq_args: bool = True):
    """(coordinates on the device, the ``box`` / ``near`` keywords of the K7 calls), every argument checked before any
    device work."""
    n_frames = _mv._check_trajectory(positions, "positions")[0]
    _mv._check_width(width)
    near = is_nearest(box)
    box = _mv._host_box(box, n_frames, outer, sq_args)
    X = K.as_device(positions)
    return X, ({"box": _mv._device_box(box, X), "near": True} if near else {"box": _mv._device_box(box, X)})


def sq_gaussian_energies(positions, offset: float, width: float, box):
    """``jaxmapval.sq_gaussian_energies`` under a periodic box: ``E_t = sum_{i,j} exp(-((|d_ij|^2 - offset) / width)^2)``
    with ``d_ij`` the image of ``r_i - r_j`` under ``box`` -- the lengths of an orthorhombic box, (3,) or
    (n_frames, 3) (minimum image), or a ``Cell`` (brick image, or the nearest image with ``images="nearest"``) -- diagonal
    included (``d = 0``).  Shape (n_frames,),
    in the container and dtype of ``positions``.  A box on a GPU is not checked: a frame whose box is bad is NaN."""
    X, b = _mapval_inputs(positions, width, box)
    _, E = K.gauss_pair_forces(X, offset, width, want_forces=False, want_energies=True, **b)
    return K.like_input(E, positions)


def sq_gaussian_forces(positions, offset: float, width: float, box):
    """``jaxmapval.sq_gaussian_forces`` under a periodic box: ``G_i = (8 / width^2) sum_j (x_ij - offset) g(x_ij) d_ij``,
    ``x_ij = |d_ij|^2``, ``d_ij`` the image of ``r_i - r_j`` under ``box`` (as ``sq_gaussian_energies``) -- the forces
    of that energy wherever no pair sits where its image switches."""
    X, b = _mapval_inputs(positions, width, box)
    G, _ = K.gauss_pair_forces(X, offset, width, **b)
    return K.like_input(G, positions)


def rsqpg_forces(positions, inner: float, outer: float, width: float, randg=None, sq_args: bool = True, box=None):
    """``jaxmapval.rsqpg_forces`` with ``box=``: the forces of one random squared-distance Gaussian field of image
    distances (the same draw from ``randg``).  As ``method`` of ``random_force_proj`` / ``random_residual_shift`` it
    takes their fused path.  ``outer`` (a distance if ``sq_args``, else a squared one) must not exceed half the
    smallest box length, ``Cell.safe_radius`` for a cell, ``Cell.image_radius`` for one with ``images="nearest"``:
    ``ValueError`` for a box on the host, not checked for a box on a GPU.  The Gaussian's tail past ``outer`` is the caller's concern."""
    _mv._check_trajectory(positions, "positions")
    lo, interval_width, w = _mv._sq_params(inner, outer, width, sq_args)
    X, b = _mapval_inputs(positions, w, box, outer, sq_args)
    if randg is None:
        randg = np.random.default_rng()
    offset = randg.random() * interval_width + lo
    G, _ = K.gauss_pair_forces(X, offset, w, **b)
    return K.like_input(G, positions)
