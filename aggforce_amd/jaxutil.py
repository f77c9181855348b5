"""Differentiable array helpers at the reference's module path (reference: jaxutil.py).

The reference differentiates these through JAX; here the array type is the torch tensor and ``trjdot`` runs on the
HIP kernels through the autograd Functions of ``_autograd`` (K3 / K3c forward, K8 backward), differentiable in both
arguments to any order.  ``distances`` of GPU tensors runs on K9 through ``PairDist`` / ``PairPull`` / ``PairDot``:
no (T, m, n, 3) displacement array is formed, forward or backward, and a zero distance (the diagonal of a self-distance
matrix, coincident sites) has gradient 0 at every order -- plain torch returns NaN from the second order on.  Its
other forms (``return_displacements``, CPU tensors, NumPy inputs, other dtypes) and ``abatch`` are plain torch code:
autograd handles them.

``pair_distances`` is the same over a static list of pairs (``PairList``: bonded pairs, non-bonded pairs with
exclusions, site-to-atom lists) on K9c / K9d through ``PairListDist`` / ``PairListPull`` / ``PairListDot``: every array
is (T, n_pairs), forward and backward.  The upper triangles of ``distances(x, return_matrix=False)`` are the list
``PairList.upper_triangle(n)``, so they never form the (T, n, n) matrix.

Periodic boundaries (not in the reference): ``pair_distances(..., box=)`` and ``distances_in_box`` take the lengths of
an orthorhombic cell, one box or one per frame, and return minimum-image distances on the box forms of K9c / K9d.
``min_distances`` reduces a trajectory to the smallest distance each pair reaches (K9e), and
``PairList.from_cutoff`` builds the static list of the pairs that come within a cutoff from it.
"""
from typing import Callable, Union

import numpy as np
import torch

from . import _kernels as K
from ._cell import Cell, is_cell_rows, is_nearest, nearest_of

_FACTOR_MSG = "Factor matrix is an incompatible shape."


def _check_trjdot_shapes(points, factor) -> int:
    """Rank and shape checks of trjdot (before any device work); returns the factor's rank."""
    fshape = tuple(factor.shape) if hasattr(factor, "shape") else np.shape(factor)
    pshape = tuple(points.shape) if hasattr(points, "shape") else np.shape(points)
    if len(fshape) not in (2, 3):
        raise ValueError(_FACTOR_MSG)
    if len(pshape) != 3 or pshape[2] != 3:
        raise ValueError(f"points must have shape (n_steps, n_sites, 3); got {pshape}")
    if len(fshape) == 2 and fshape[1] != pshape[1]:
        raise ValueError(f"factor of shape {fshape} cannot map points of shape {pshape}")
    if len(fshape) == 3 and (fshape[0] != pshape[0] or fshape[2] != pshape[1]):
        raise ValueError(f"factor of shape {fshape} cannot map points of shape {pshape}")
    return len(fshape)


def _float_tensor(x, device) -> torch.Tensor:
    """A float32/float64 tensor on ``device``; torch inputs keep their autograd history."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.to(device)


def trjdot(points, factor):
    """out[t,c,d] = sum_f factor[c,f] points[t,f,d] (2-D factor (n_cg, n_sites)), or with a per-frame factor
    (n_steps, n_cg, n_sites) sum_f factor[t,c,f] points[t,f,d] (reference jaxutil.py:10-57).

    NumPy arguments give a NumPy result (the same kernels as ``util.trjdot``).  If either argument is a torch tensor
    the result is a tensor, on the device of ``points`` (GPU tensors) and differentiable in both arguments."""
    from .util import trjdot as np_trjdot

    fdim = _check_trjdot_shapes(points, factor)
    if not (isinstance(points, torch.Tensor) or isinstance(factor, torch.Tensor)):
        return np_trjdot(points, factor)
    from ._autograd import Apply, ApplyFrames

    K.lib()
    home = points if isinstance(points, torch.Tensor) else factor
    dev = home.device if home.is_cuda else K.default_device()
    p, f = _float_tensor(points, dev), _float_tensor(factor, dev)
    out = Apply.apply(p, f) if fdim == 2 else ApplyFrames.apply(p, f)
    return out if home.is_cuda else out.to(home.device)


def abatch(
    func: Callable[..., torch.Tensor],
    arr: torch.Tensor,
    chunk_size: Union[None, int],
    *args,
    **kwargs,
) -> torch.Tensor:
    """func(arr, *args, **kwargs) evaluated on chunks of ``arr`` along its first axis and concatenated
    (reference jaxutil.py:60-100; ``torch.cat`` in place of ``jnp.vstack``)."""
    if chunk_size is None or chunk_size >= arr.shape[0]:
        return func(arr, *args, **kwargs)
    n_chunks = int(np.ceil(len(arr) / chunk_size))
    # (np.array_split's chunk sizes: the first len % n_chunks chunks are one longer)
    base, extra = divmod(len(arr), n_chunks)
    sizes = [base + 1] * extra + [base] * (n_chunks - extra)
    chunks = torch.split(arr, sizes) if isinstance(arr, torch.Tensor) else np.array_split(arr, n_chunks)
    results = [func(sub, *args, **kwargs) for sub in chunks]
    if all(isinstance(r, torch.Tensor) for r in results):
        return torch.cat([r if r.dim() > 1 else r.reshape(1, -1) for r in results])
    return np.vstack(results)


def _on_kernels(x, like=None) -> bool:
    """A (T, n, 3) float32/float64 GPU tensor (with ``like``: on its device, with its number of frames)."""
    ok = (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.dim() == 3
          and x.shape[2] == 3)
    return ok and (like is None or (x.device == like.device and x.shape[0] == like.shape[0]))


def _upper_triangles(dist: torch.Tensor) -> torch.Tensor:
    n_sites = dist.shape[-1]
    i0, i1 = torch.triu_indices(n_sites, n_sites, offset=1, device=dist.device)
    return dist[:, i0, i1]


def _incidence(sites: np.ndarray, n: int):
    """CSR table of the pairs at each of ``n`` sites: (ptr (n + 1,), pair index (P,)) int32, a site's pairs in
    ascending pair index (a stable sort of the pairs by site), and the longest run."""
    idx = np.argsort(sites, kind="stable").astype(np.int32)
    counts = np.bincount(sites, minlength=n) if sites.size else np.zeros(n, dtype=np.int64)
    ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(counts, out=ptr[1:])
    return ptr, idx, int(counts.max()) if n else 0


def _as_box(box, n_steps: int) -> torch.Tensor:
    """``box`` as a tensor of shape (3,) or (n_steps, 3): the lengths of an orthorhombic cell, one for all frames or
    one per frame.  A box on the host (a sequence, a NumPy array, a CPU tensor) is checked here -- positive, finite --
    and comes out as float64; a box on a GPU is taken as it is (no synchronisation: the kernels turn a frame whose
    box is bad into NaN).  The box is a constant: one that requires a gradient is refused.

    A ``pbc.Cell`` (a triclinic cell, checked when it was made) comes out as its (n_steps, 9) rows -- the row-major
    matrix of every frame, a constant cell expanded -- which no raw array can be: (n_steps, 9) is refused like every
    other raw shape."""
    if isinstance(box, Cell):
        return box.rows(n_steps).contiguous()
    if isinstance(box, torch.Tensor):
        if box.requires_grad:
            raise ValueError("box is a constant: gradients with respect to box lengths are not built")
        if not box.dtype.is_floating_point:
            box = box.double()
    else:
        try:
            box = torch.as_tensor(np.asarray(box, dtype=np.float64))
        except (TypeError, ValueError) as exc:
            raise ValueError(f"box must hold numbers: {exc}") from None
    if tuple(box.shape) not in ((3,), (n_steps, 3)):
        raise ValueError(f"box must have shape (3,) or (n_steps, 3) = ({n_steps}, 3); got {tuple(box.shape)}")
    if not box.is_cuda:
        box = box.double()
        if not bool((torch.isfinite(box) & (box > 0)).all()):
            raise ValueError("box lengths must be positive and finite")
    return box


def _wrap(disp: torch.Tensor, box: torch.Tensor, near: bool = False) -> torch.Tensor:
    """The minimum image of displacements (T, ..., 3) in plain torch: d - L rint(d / L), rint to nearest even.  Under
    the (T, 9) rows of a ``Cell``: its brick reduction (``_cell``) in the same plain operations, stage by stage on
    the updated displacement -- with zero off-diagonal entries the box form's numbers bit for bit (d - 0 k == d).
    ``near`` (with the rows of a cell): then the shortest of the brick image's 27 translates (``_cell.nearest_of``)."""
    L = box.to(device=disp.device, dtype=disp.dtype if disp.dtype.is_floating_point else torch.float64)
    if is_cell_rows(L):
        h = L.reshape((L.shape[0],) + (1,) * (disp.dim() - 2) + (9,))
        ax, bx, by, cx, cy, cz = (h[..., k] for k in (0, 3, 4, 6, 7, 8))
        d0, d1, d2 = disp[..., 0], disp[..., 1], disp[..., 2]
        kc = torch.round(d2 / cz)
        d2, d1, d0 = d2 - cz * kc, d1 - cy * kc, d0 - cx * kc
        kb = torch.round(d1 / by)
        d1, d0 = d1 - by * kb, d0 - bx * kb
        ka = torch.round(d0 / ax)
        d0 = d0 - ax * ka
        if near:
            d0, d1, d2 = nearest_of(d0, d1, d2, ax, bx, by, cx, cy, cz)
        return torch.stack([d0, d1, d2], dim=-1)
    if L.dim() == 2:
        L = L.reshape((L.shape[0],) + (1,) * (disp.dim() - 2) + (3,))
    return disp - L * torch.round(disp / L)


class PairList:
    """A static list of site pairs shared by all frames, validated on the host once: ``pairs`` (P, 2) integers (a
    list, a NumPy array or a torch tensor on any device), row p = (i_p, j_p) with ``0 <= j_p < n_sites`` and
    ``0 <= i_p < n_cross`` (``n_cross`` None: the self form, both sites among the same ``n_sites``).  The order
    (i, j) = (other, self) is that of the (T, other, self) result of ``distances``.  Repeated pairs are allowed (each
    is its own column), so are i == j in the self form (distance 0, gradient weight 0) and an empty list.

    The device side -- the int32 index array and the two incidence tables (the pairs of every j and of every i, in
    ascending pair index) that the backward kernel sums over -- is built on first use, once per device."""

    _triangles: dict = {}
    _all: dict = {}

    def __init__(self, pairs, n_sites: int, n_cross: Union[int, None] = None):
        if isinstance(pairs, torch.Tensor):
            if pairs.dtype.is_floating_point or pairs.dtype.is_complex or pairs.dtype == torch.bool:
                raise ValueError(f"pairs must be integers; got {pairs.dtype}")
            arr = pairs.detach().cpu().numpy()
        else:
            arr = np.asarray(pairs)
            if arr.size == 0 and arr.dtype.kind == "f":  # ([] and [[]] come out as float64)
                arr = arr.astype(np.int64)
        if arr.dtype.kind not in "iu":
            raise ValueError(f"pairs must be integers; got {arr.dtype}")
        if arr.ndim == 1 and arr.size == 0:
            arr = arr.reshape(0, 2)
        if arr.ndim != 2 or arr.shape[1] != 2:
            raise ValueError(f"pairs must have shape (n_pairs, 2); got {arr.shape}")
        if arr.dtype == np.uint64 and arr.size and int(arr.max()) > np.iinfo(np.int64).max:
            raise ValueError("pairs holds an index beyond the int64 range")
        self.n_sites = int(n_sites)
        self.n_cross = None if n_cross is None else int(n_cross)
        if self.n_sites < 0 or (self.n_cross is not None and self.n_cross < 0):
            raise ValueError(f"negative number of sites: n_sites {n_sites}, n_cross {n_cross}")
        self.pairs = np.array(arr, dtype=np.int64)  # (a copy: the list is a constant from here on)
        self.pairs.setflags(write=False)
        self.n_pairs = int(self.pairs.shape[0])
        m = self.n_rows
        if max(m, self.n_sites, self.n_pairs) > np.iinfo(np.int32).max:
            raise ValueError("a pair list is limited to 2^31 - 1 pairs and sites")
        bad = (self.pairs[:, 0] < 0) | (self.pairs[:, 0] >= m) | (self.pairs[:, 1] < 0) | (self.pairs[:, 1] >= self.n_sites)
        if bad.any():
            row = int(np.argmax(bad))
            raise ValueError(f"pairs row {row} = ({self.pairs[row, 0]}, {self.pairs[row, 1]}) is out of range: "
                             f"i must be in [0, {m}) and j in [0, {self.n_sites})")
        self._host = None
        self._devices: dict = {}

    @property
    def n_rows(self) -> int:
        """The number of sites i runs over: ``n_cross``, or ``n_sites`` in the self form."""
        return self.n_sites if self.n_cross is None else self.n_cross

    @classmethod
    def upper_triangle(cls, n_sites: int) -> "PairList":
        """The pairs i < j of ``n_sites`` sites in the order of ``torch.triu_indices(n, n, offset=1)`` (what
        ``distances(x, return_matrix=False)`` returns); one object per ``n_sites``, kept."""
        n_sites = int(n_sites)
        if n_sites not in cls._triangles:
            if len(cls._triangles) >= 8:  # (a handful of system sizes per process; the tables are O(n^2))
                cls._triangles.pop(next(iter(cls._triangles)))
            cls._triangles[n_sites] = cls(np.stack(np.triu_indices(n_sites, k=1), axis=1), n_sites)
        return cls._triangles[n_sites]

    @classmethod
    def all_pairs(cls, n_sites: int, n_cross: Union[int, None] = None) -> "PairList":
        """Every pair (i, j), i over ``n_cross`` sites (None: the self form, i over ``n_sites``, i == j included), in
        row-major order of (i, j): a (T, P) array over this list is the (T, other, self) matrix of ``distances``
        reshaped.  One object per shape, kept."""
        key = (int(n_sites), None if n_cross is None else int(n_cross))
        if key not in cls._all:
            if len(cls._all) >= 8:
                cls._all.pop(next(iter(cls._all)))
            n, m = key[0], key[0] if key[1] is None else key[1]
            i, j = np.divmod(np.arange(m * n, dtype=np.int64), max(n, 1))
            cls._all[key] = cls(np.stack([i, j], axis=1), n, key[1])
        return cls._all[key]

    @classmethod
    def from_cutoff(cls, xyz, cutoff: float, cross_xyz=None, box=None, exclude=None) -> "PairList":
        """The static list of the pairs that come within ``cutoff`` of each other in any frame:
        ``min_distances(xyz, cross_xyz, box=box) <= cutoff`` (a NaN minimum is never kept).  The self form keeps i < j
        in the order of ``upper_triangle``; the cross form keeps all (i, j) in row-major order.  ``exclude`` (a
        ``PairList`` or a (k, 2) integer array): pairs to leave out, e.g. bonded ones; in the self form (i, j) and
        (j, i) are the same pair.  Under a box the minimum image is only the nearest image up to half a box length:
        a cutoff beyond half the smallest length of any frame raises ``ValueError``.  Under a ``pbc.Cell`` the list
        is exact for ``cutoff <= cell.image_radius`` (``safe_radius`` for brick images, half the shortest lattice
        vector for ``images="nearest"``): a host cell with a larger cutoff raises ``ValueError``; with a cell on a GPU
        (not read back) that condition is the caller's part."""
        cutoff = float(cutoff)
        if not cutoff >= 0 or not np.isfinite(cutoff):
            raise ValueError(f"cutoff must be a non-negative finite number; got {cutoff}")
        dmin = min_distances(xyz, cross_xyz, box=box)
        if isinstance(box, Cell):
            if box.nearest and not box.is_cuda and not cutoff <= box.image_radius:
                raise ValueError(f"cutoff {cutoff} is beyond the cell's image radius, half its shortest lattice "
                                 f"vector = {box.image_radius}: the nearest of 27 images is not the minimum image there")
            if not box.nearest and not box.is_cuda and not cutoff <= box.safe_radius:
                raise ValueError(f"cutoff {cutoff} is beyond the cell's safe radius min(ax, by, cz) / 2 = "
                                 f"{box.safe_radius}: the brick image is not the nearest image there")
        elif box is not None:
            lengths = _as_box(box, int(xyz.shape[0]) if hasattr(xyz, "shape") else len(xyz)).detach().cpu().double()
            if lengths.numel() and not cutoff <= 0.5 * float(lengths.min()):
                raise ValueError(f"cutoff {cutoff} is beyond half the smallest box length {float(lengths.min())}: the "
                                 "minimum image is not the nearest image there")
        keep = (dmin <= cutoff).cpu().numpy()
        m, n = keep.shape
        if cross_xyz is None:
            keep &= np.triu(np.ones((n, n), dtype=bool), k=1)
        if exclude is not None:
            ex = exclude.pairs if isinstance(exclude, PairList) else cls(exclude, n, None if cross_xyz is None else m).pairs
            keep[ex[:, 0], ex[:, 1]] = False
            if cross_xyz is None:
                keep[ex[:, 1], ex[:, 0]] = False
        return cls(np.argwhere(keep), n, None if cross_xyz is None else m)

    def tables(self):
        """The incidence tables on the host: ``(by_j, by_i)``, each ``(ptr, pair index, longest run)``."""
        if self._host is None:
            self._host = (_incidence(self.pairs[:, 1], self.n_sites), _incidence(self.pairs[:, 0], self.n_rows))
        return self._host

    def on(self, device) -> "K.PairTables":
        """The list on ``device`` (cached): see ``_kernels.PairTables``."""
        device = torch.device(device)
        if device not in self._devices:
            (a_ptr, a_idx, a_deg), (b_ptr, b_idx, b_deg) = self.tables()
            put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            self._devices[device] = K.PairTables(put(self.pairs.astype(np.int32)), put(a_ptr), put(a_idx), put(b_ptr),
                                                 put(b_idx), a_deg, b_deg, self.n_rows, self.n_sites)
        return self._devices[device]


def pair_distances(xyz, pairs, cross_xyz=None, square: bool = False, box=None) -> torch.Tensor:
    """Differentiable distances over a list of pairs: (n_steps, n_pairs),
    ``out[t, p] = |xyz[t, j_p] - (cross_xyz if given else xyz)[t, i_p]|`` (squared with ``square``), for ``pairs`` a
    ``PairList`` or any (n_pairs, 2) integer array of rows (i_p, j_p) -- the index order of the (T, other, self) result
    of ``distances``: with the pairs of ``torch.triu_indices`` this is ``distances(xyz)[:, i, j]``.

    float32/float64 GPU tensors run on the K9c / K9d kernels (``PairListDist``): nothing of the size of the distance
    matrix is formed, forward or backward, the result is differentiable in both arrays to any order, and a zero
    distance has gradient 0.  CPU tensors, NumPy inputs and other dtypes take plain torch operations.

    ``box``: the lengths of an orthorhombic periodic cell, (3,) or (n_steps, 3) (a sequence, an array or a tensor; a
    constant).  Every displacement is then its minimum image, d - L rint(d / L) per component -- the nearest image
    for distances up to half a box length -- on the box forms of the same kernels.  A ``pbc.Cell`` (a triclinic
    cell): every displacement is its brick image -- the nearest image for distances up to ``cell.safe_radius``, a
    periodic image that is never shorter than it beyond -- on the triclinic forms of the same kernels, with every
    convention of the box forms (inputs, dtypes, gradients of any order, NaN for a bad frame).  A cell with
    ``images="nearest"``: the shortest of the brick image's 27 translates -- the nearest image for distances up to
    ``cell.image_radius`` -- on the nearest-image forms of the same kernels; the backward kernels choose the same image."""
    def shape_of(a):
        return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)

    shapes = [shape_of(xyz)] + ([] if cross_xyz is None else [shape_of(cross_xyz)])
    for s in shapes:
        if len(s) != 3 or s[2] != 3:
            raise ValueError(f"sites must have shape (n_steps, n_sites, 3); got {s}")
    if len(shapes) == 2 and shapes[0][0] != shapes[1][0]:
        raise ValueError(f"xyz {shapes[0]} and cross_xyz {shapes[1]} differ in their number of frames")
    n_sites, n_cross = shapes[0][1], (None if cross_xyz is None else shapes[1][1])
    plist = pairs if isinstance(pairs, PairList) else PairList(pairs, n_sites, n_cross)
    if (plist.n_sites, plist.n_cross) != (n_sites, n_cross):
        raise ValueError(f"a pair list for n_sites {plist.n_sites}, n_cross {plist.n_cross} with xyz {shapes[0]}"
                         + ("" if cross_xyz is None else f" and cross_xyz {shapes[1]}"))
    near = is_nearest(box)
    if box is not None:
        box = _as_box(box, shapes[0][0])
    if _on_kernels(xyz) and (cross_xyz is None or _on_kernels(cross_xyz, xyz)):
        from ._autograd import PairListDist

        K.lib()
        if box is None:
            return PairListDist.apply(xyz, xyz if cross_xyz is None else cross_xyz, plist, bool(square))
        if near:
            return PairListDist.apply(xyz, xyz if cross_xyz is None else cross_xyz, plist, bool(square),
                                      box.to(xyz.device), True)
        return PairListDist.apply(xyz, xyz if cross_xyz is None else cross_xyz, plist, bool(square),
                                  box.to(xyz.device))
    xyz = xyz if isinstance(xyz, torch.Tensor) else torch.as_tensor(np.asarray(xyz))
    if cross_xyz is None:
        other = xyz
    else:
        other = cross_xyz if isinstance(cross_xyz, torch.Tensor) else torch.as_tensor(np.asarray(cross_xyz))
    i = torch.from_numpy(plist.pairs[:, 0].copy()).to(other.device)
    j = torch.from_numpy(plist.pairs[:, 1].copy()).to(xyz.device)
    disp = xyz[:, j] - other[:, i]
    if box is not None:
        disp = _wrap(disp, box, near)
    return (disp**2).sum(dim=-1) if square else torch.linalg.vector_norm(disp, dim=-1)


def min_distances(xyz, cross_xyz=None, square: bool = False, box=None) -> torch.Tensor:
    """The smallest distance each pair of sites reaches over the trajectory: (other_n_sites, n_sites),
    ``out[i, j] = min_t |xyz[t, j] - (cross_xyz if given else xyz)[t, i]|`` (squared with ``square``; the minimum
    image under ``box``, as in ``pair_distances``).  Detached: it is the input of a list builder
    (``PairList.from_cutoff``), not of a loss.  A NaN coordinate makes every pair of its site NaN; without frames
    every minimum is +inf.

    float32/float64 GPU tensors run on K9e (``aggf_pair_min``), which reads the coordinates alone: nothing of the size
    (n_steps, other, self) is formed.  Everything else is ``amin`` over plain torch."""
    for a in (xyz,) if cross_xyz is None else (xyz, cross_xyz):
        shape = tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
        if len(shape) != 3 or shape[2] != 3:
            raise ValueError(f"sites must have shape (n_steps, n_sites, 3); got {shape}")
    n_steps = int(xyz.shape[0]) if hasattr(xyz, "shape") else len(xyz)
    given = box
    if box is not None:
        box = _as_box(box, n_steps)
    if _on_kernels(xyz) and (cross_xyz is None or _on_kernels(cross_xyz, xyz)):
        x = xyz.detach()
        c = x if cross_xyz is None else cross_xyz.detach()
        ct = torch.promote_types(x.dtype, c.dtype)
        x, c = x.to(ct).contiguous(), c.to(ct).contiguous()
        return K.pair_min(x, c, bool(square), None if box is None else box.to(device=x.device, dtype=ct).contiguous(),
                          near=is_nearest(given))
    with torch.no_grad():
        d = _distances(xyz, cross_xyz, True, False, square, given)
        if d.shape[0] == 0:
            return torch.full(tuple(d.shape[1:]), float("inf"), dtype=d.dtype, device=d.device)
        return d.amin(dim=0)


def distances(
    xyz: torch.Tensor,
    cross_xyz: Union[torch.Tensor, None] = None,
    return_matrix: bool = True,
    return_displacements: bool = False,
    square: bool = False,
) -> torch.Tensor:
    """Differentiable per-frame distances (reference jaxutil.py:103-187): (n_steps, n_sites, n_sites) matrices, or
    (n_steps, other_n_sites, n_sites) with ``cross_xyz``, or the flattened upper triangles (``return_matrix=False``);
    displacements (one more trailing axis) with ``return_displacements``; squared distances with ``square``.  The
    signature is the reference's; under a periodic box use ``distances_in_box``."""
    return _distances(xyz, cross_xyz, return_matrix, return_displacements, square, None)


def distances_in_box(
    xyz: torch.Tensor,
    box,
    cross_xyz: Union[torch.Tensor, None] = None,
    return_matrix: bool = True,
    return_displacements: bool = False,
    square: bool = False,
) -> torch.Tensor:
    """``distances`` under an orthorhombic periodic cell (not in the reference): minimum-image distances and
    displacements for ``box`` as in ``pair_distances`` (the lengths of a box, or a ``pbc.Cell``).  On GPU tensors both
    forms run on the pair-list kernels -- the matrix over ``PairList.all_pairs``, reshaped -- since the matrix kernels
    K9a / K9b have no box form."""
    if box is None:
        raise ValueError("distances_in_box needs a box; without one it is distances")
    return _distances(xyz, cross_xyz, return_matrix, return_displacements, square, box)


def _distances(xyz, cross_xyz, return_matrix, return_displacements, square, box) -> torch.Tensor:
    if cross_xyz is not None and not return_matrix:
        raise ValueError("Cross distances only supported when return_matrix is truthy.")
    if return_displacements and not return_matrix:
        raise ValueError("Displacements only supported when return_matrix is truthy.")
    if not return_displacements and _on_kernels(xyz) and (cross_xyz is None or _on_kernels(cross_xyz, xyz)):
        if not return_matrix:  # the pairs i < j as a list: no (T, n, n) array, forward or backward
            return pair_distances(xyz, PairList.upper_triangle(xyz.shape[1]), square=square, box=box)
        if box is not None:
            n_cross = None if cross_xyz is None else cross_xyz.shape[1]
            flat = pair_distances(xyz, PairList.all_pairs(xyz.shape[1], n_cross), cross_xyz, square=square, box=box)
            return flat.reshape(xyz.shape[0], xyz.shape[1] if n_cross is None else n_cross, xyz.shape[1])
        from ._autograd import PairDist

        K.lib()
        return PairDist.apply(xyz, xyz if cross_xyz is None else cross_xyz, bool(square))
    xyz = xyz if isinstance(xyz, torch.Tensor) else torch.as_tensor(np.asarray(xyz))
    if cross_xyz is None:
        disp = xyz[:, None, :, :] - xyz[:, :, None, :]
    else:
        cross_xyz = cross_xyz if isinstance(cross_xyz, torch.Tensor) else torch.as_tensor(np.asarray(cross_xyz))
        disp = xyz[:, None, :, :] - cross_xyz[:, :, None, :]
    if box is not None:
        disp = _wrap(disp, _as_box(box, xyz.shape[0]), is_nearest(box))
    if return_displacements:
        return disp
    if square:
        dist = (disp**2).sum(dim=-1)
    else:
        dist = torch.linalg.vector_norm(disp, dim=-1)
    return dist if return_matrix else _upper_triangles(dist)
