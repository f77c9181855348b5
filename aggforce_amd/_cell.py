"""Triclinic periodic cells (not in the reference): the ``Cell`` that every ``box=`` of the pair-distance, cutoff-list,
whole-molecule, constraint-guess, map-validation and featuriser functions takes beside the lengths of an orthorhombic
box (``pbc.Cell``).

A cell is three lattice vectors as the rows ``a, b, c`` of a lower-triangular matrix (the GROMACS / MDTraj
convention)::

    a = (ax, 0, 0)      b = (bx, by, 0)      c = (cx, cy, cz)          ax, by, cz > 0

The image of a displacement ``d`` is obtained by BRICK REDUCTION, each line on the updated ``d``::

    kc = rint(dz / cz);  d -= kc c
    kb = rint(dy / by);  d -= kb b
    ka = rint(dx / ax);  d -= ka a

(``rint`` to nearest even; the kernels multiply by inverses formed once per frame and subtract with fused
multiply-adds: ``csrc/aggf_common.h``, ``brick_image``).  For a cell without off-diagonal entries this is the
orthorhombic minimum image component by component, bit for bit.  What it guarantees:

* the result is the unique lattice translate of ``d`` inside the brick ``|dx| <= ax/2, |dy| <= by/2, |dz| <= cz/2``,
  for any lower-triangular cell (no "reduced" condition on the skews);
* it is the true minimum image whenever that is shorter than ``safe_radius = min(ax, by, cz) / 2``;
* beyond ``safe_radius`` it is still a periodic image, never shorter than the minimum: a cutoff list with
  ``cutoff <= safe_radius`` is exact.

This is what OpenMM and GROMACS do inside their cutoffs, and the "shorter than half the cell" condition that
``make_whole`` documents for bonds.

THE NEAREST IMAGE, ``Cell(vectors, images="nearest")``.  In the cells solvated systems are run in, ``safe_radius`` is
well short of where the minimum image is well defined (half the shortest lattice vector); in float64, for cells of
image distance d and 2e5 random displacements each:

    cell                                    safe_radius   half the shortest      true minimum image below d/2
                                                          lattice vector         where the brick image is not it
    rhombic dodecahedron, square form         0.354 d        0.5 d                   11.7 %
    rhombic dodecahedron, hexagonal form      0.408 d        0.5 d                    7.3 %
    truncated octahedron                      0.408 d        0.5 d                    5.1 %

The nearest form starts from the brick image and takes the shortest of its 27 translates ``d + i a + j b + k c``,
``i, j, k`` in {-1, 0, 1}, by squared length.  The candidates are visited in one fixed order -- (0, 0, 0) first, then
k = -1, 0, 1 outermost, j inside it, i innermost -- and a candidate replaces the best so far only if it is strictly
shorter: a tie keeps the earlier one (the brick image before all others), and the choice is deterministic.  A brick
image no longer than ``safe_radius`` is the answer already and the search is skipped, with the same bits
(``csrc/aggf_common.h``, ``nearest_image``).  What it guarantees:

* for a REDUCED cell -- ``|bx| <= ax/2``, ``|cx| <= ax/2``, ``|cy| <= by/2``, the GROMACS condition; equality allowed --
  the result is the true minimum image whenever that image is shorter than ``image_radius``, half the length of the
  shortest of the 26 lattice vectors ``i a + j b + k c``;
* beyond ``image_radius`` it is a periodic image, never longer than the brick image;
* with zero off-diagonal entries it is the orthorhombic minimum image bit for bit, and wherever the brick image is
  within ``safe_radius`` it is the brick image bit for bit.

The image is a locally constant choice, so gradients are those of the brick form with that image, to any order.  It
is used by ``pair_distances``, ``distances_in_box``, ``min_distances``, ``PairList.from_cutoff``, the map-validation
functions and the featuriser (below); ``guess_pairwise_constraints`` and ``make_whole`` accept such a cell and run
their brick forms (they measure bonds and rigid pairs, which must be shorter than ``safe_radius``, where the two
images coincide).

THE FEATURISER.  ``gb_feat(box=Cell)`` -- with the fused fit, the one-pass cross-validation and the fitted map's
application behind it -- and ``qp.jaxfeat.gb_subfeat`` / ``gb_subfeat_jac`` measure the distance from a mapped site to
a group mean as the length of the cell's image, brick or nearest (cell forms of the K4 kernels).  A feature is a
function of the TRUE minimum-image distance only up to ``image_radius``, so a cell on the host whose ``image_radius``
is less than the featuriser's ``outer`` is refused (``check_reach``); an orthorhombic box needs no such rule, its wrap
is the minimum image at any distance.  A cell on a GPU is not read on the host.

Not built under a cell: ``comm=`` (frames sharded over ranks), gradients with respect to the cell; minimum-image group
means; an exact minimum image beyond ``image_radius``; the nearest image of a cell that is not reduced.
"""
from __future__ import annotations

import numpy as np
import torch


REDUCED_SLACK = 1e-6  # relative: the roundings of a float32 cell on the conditions of a reduced cell


class Cell:
    """A triclinic periodic cell, one for all frames or one per frame: ``Cell(vectors)`` with ``vectors`` (3, 3) or
    (n_steps, 3, 3), rows ``a, b, c``, as a sequence, a NumPy array or a tensor.

    A cell on the host is checked here -- ``ValueError`` for a wrong shape, non-numbers, a nonzero upper-triangular
    entry, a diagonal entry that is not positive and finite, any non-finite entry -- and kept as float64.  A cell on a
    GPU is taken as it is, with no synchronisation: the kernels read its six lower-triangular entries, and a frame
    whose diagonal entry is not positive and finite, or whose lower off-diagonal entry is not finite, comes out NaN
    (image counts 0) and no other frame.  The cell is a constant: one that requires a gradient is refused.

    ``images``: ``"brick"`` (the default: every displacement is its brick image) or ``"nearest"`` (the shortest of the
    brick image's 27 translates: the module's text).  A host cell with ``images="nearest"`` must be reduced,
    ``|bx| <= ax/2``, ``|cx| <= ax/2``, ``|cy| <= by/2`` (``ValueError``; equality is allowed, with a relative slack of
    1e-6 for a cell that was stored in float32 or converted from angles); a cell on a GPU is taken as it is.

    A class, not a raw array, because a raw (3, 3) array given as ``box=`` to three frames already means one
    orthorhombic box per frame."""

    def __init__(self, vectors, images: str = "brick"):
        if images not in ("brick", "nearest"):
            raise ValueError(f'Cell: images must be "brick" or "nearest"; got {images!r}')
        self._images = images
        if isinstance(vectors, Cell):
            vectors = vectors.vectors
        if isinstance(vectors, torch.Tensor):
            if vectors.requires_grad:
                raise ValueError("Cell: the cell is a constant: gradients with respect to the cell are not built")
            if vectors.dtype.is_complex or vectors.dtype == torch.bool:
                raise ValueError(f"Cell: vectors must hold numbers; got {vectors.dtype}")
            v = vectors if vectors.dtype.is_floating_point else vectors.double()
        else:
            try:
                v = torch.as_tensor(np.asarray(vectors, dtype=np.float64))
            except (TypeError, ValueError) as exc:
                raise ValueError(f"Cell: vectors must hold numbers: {exc}") from None
        if v.dim() not in (2, 3) or tuple(v.shape[-2:]) != (3, 3):
            raise ValueError(f"Cell: vectors must have shape (3, 3) or (n_steps, 3, 3); got {tuple(v.shape)}")
        if not v.is_cuda:
            v = v.double()
            if not bool(torch.isfinite(v).all()):
                raise ValueError("Cell: every entry must be finite")
            if bool((torch.triu(v, diagonal=1) != 0).any()):
                raise ValueError("Cell: the vectors must form a lower-triangular matrix a = (ax, 0, 0), "
                                 "b = (bx, by, 0), c = (cx, cy, cz); an upper-triangular entry is not zero")
            if not bool((torch.diagonal(v, dim1=-2, dim2=-1) > 0).all()):
                raise ValueError("Cell: the diagonal entries ax, by, cz must be positive and finite")
            if images == "nearest":
                # (equality is the rule in the standard cells -- the dodecahedron has cx = ax/2 -- and a cell that
                # went through float32 or through lengths and angles misses it by a rounding: REDUCED_SLACK)
                ax, by = v[..., 0, 0] * (1 + REDUCED_SLACK), v[..., 1, 1] * (1 + REDUCED_SLACK)
                if not bool(((v[..., 1, 0].abs() <= ax / 2) & (v[..., 2, 0].abs() <= ax / 2)
                             & (v[..., 2, 1].abs() <= by / 2)).all()):
                    raise ValueError('Cell: images="nearest" needs a reduced cell: |bx| <= ax/2, |cx| <= ax/2 and '
                                     "|cy| <= by/2 (add multiples of a to b, and of a and b to c, until they hold)")
        self._v = v.detach()

    @classmethod
    def from_lengths_angles(cls, lengths, angles_deg, images: str = "brick") -> "Cell":
        """The cell of edge lengths (A, B, C) and angles (alpha, beta, gamma) in degrees, (3,) or (n_steps, 3) each
        (alpha between b and c, beta between a and c, gamma between a and b), by the standard conversion in float64:
        a = (A, 0, 0), b = (B cos gamma, B sin gamma, 0), cx = C cos beta, cy = C (cos alpha - cos beta cos gamma) /
        sin gamma, cz = sqrt(C^2 - cx^2 - cy^2).  An angle of exactly 90 degrees gives an exact zero.  ``images``: as in
        ``Cell``."""
        try:
            L = np.asarray(lengths.detach().cpu() if isinstance(lengths, torch.Tensor) else lengths, dtype=np.float64)
            A = np.asarray(angles_deg.detach().cpu() if isinstance(angles_deg, torch.Tensor) else angles_deg,
                           dtype=np.float64)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"Cell.from_lengths_angles: lengths and angles must hold numbers: {exc}") from None
        if L.shape != A.shape or L.ndim not in (1, 2) or L.shape[-1] != 3:
            raise ValueError("Cell.from_lengths_angles: lengths and angles must both have shape (3,) or (n_steps, 3); "
                             f"got {L.shape} and {A.shape}")
        rad = np.deg2rad(A)
        cos = np.where(A == 90.0, 0.0, np.cos(rad))
        sin = np.where(A == 90.0, 1.0, np.sin(rad))
        ca, cb, cg, sg = cos[..., 0], cos[..., 1], cos[..., 2], sin[..., 2]
        v = np.zeros(L.shape[:-1] + (3, 3), dtype=np.float64)
        with np.errstate(all="ignore"):
            v[..., 0, 0] = L[..., 0]
            v[..., 1, 0] = L[..., 1] * cg
            v[..., 1, 1] = L[..., 1] * sg
            v[..., 2, 0] = L[..., 2] * cb
            v[..., 2, 1] = L[..., 2] * (ca - cb * cg) / sg
            v[..., 2, 2] = np.sqrt(L[..., 2] ** 2 - v[..., 2, 0] ** 2 - v[..., 2, 1] ** 2)
        return cls(v, images=images)

    @property
    def vectors(self) -> torch.Tensor:
        """The (3, 3) or (n_steps, 3, 3) tensor of lattice vectors (rows a, b, c)."""
        return self._v

    @property
    def is_per_frame(self) -> bool:
        return self._v.dim() == 3

    @property
    def is_cuda(self) -> bool:
        return self._v.is_cuda

    @property
    def safe_radius(self):
        """``min(ax, by, cz) / 2`` over all frames: up to this length the brick image is the true minimum image.  A
        float for a host cell, a 0-d tensor for a cell on a GPU (no synchronisation)."""
        d = torch.diagonal(self._v, dim1=-2, dim2=-1)
        if d.numel() == 0:
            return float("inf") if not self._v.is_cuda else torch.full((), float("inf"), device=self._v.device)
        r = d.min() / 2
        return r if self._v.is_cuda else float(r)

    @property
    def images(self) -> str:
        """``"brick"`` or ``"nearest"``: the image this cell gives a displacement."""
        return self._images

    @property
    def nearest(self) -> bool:
        return self._images == "nearest"

    @property
    def image_radius(self):
        """Up to this length the cell's image is the true minimum image: ``safe_radius`` for ``"brick"``; for
        ``"nearest"`` half the length of the shortest of the 26 lattice vectors ``i a + j b + k c``, ``i, j, k`` in
        {-1, 0, 1}, over all frames.  A float for a host cell, a 0-d tensor for a cell on a GPU (no synchronisation)."""
        if not self.nearest:
            return self.safe_radius
        if self._v.numel() == 0:
            return float("inf") if not self._v.is_cuda else torch.full((), float("inf"), device=self._v.device)
        idx = torch.arange(27, device=self._v.device)
        ijk = torch.stack([idx % 3 - 1, idx // 3 % 3 - 1, idx // 9 - 1], dim=1).to(self._v.dtype)
        lengths = torch.linalg.vector_norm(ijk @ self._v, dim=-1)  # (the combination (0, 0, 0) has length 0: left out)
        r = torch.where(lengths > 0, lengths, torch.full_like(lengths, float("inf"))).min() / 2
        return r if self._v.is_cuda else float(r)

    def take(self, frames) -> "Cell":
        """The cell of the frames ``frames`` (an index array): itself unless it is per frame."""
        if not self.is_per_frame:
            return self
        return Cell(self._v[torch.as_tensor(np.asarray(frames), device=self._v.device)], images=self._images)

    def rows(self, n_steps: int) -> torch.Tensor:
        """(n_steps, 9): the row-major matrix of every frame -- the form the kernels and host bodies take (a constant
        cell is expanded: 72 bytes per frame beside the frame's 24 n_sites bytes of coordinates).  ``ValueError`` if a
        per-frame cell has another number of frames."""
        n_steps = int(n_steps)
        if self.is_per_frame:
            if self._v.shape[0] != n_steps:
                raise ValueError(f"a per-frame Cell of {self._v.shape[0]} frames for {n_steps} frames")
            return self._v.reshape(n_steps, 9)
        return self._v.reshape(1, 9).expand(n_steps, 9)

    def __repr__(self) -> str:
        return (f"Cell({'per frame, ' if self.is_per_frame else ''}"
                f"vectors={self._v.tolist() if self._v.numel() <= 9 else '...'}"
                f"{', images=' + repr(self._images) if self.nearest else ''})")


def is_cell_rows(box) -> bool:
    """Whether a normalised box (``jaxutil._as_box``) is the (n_steps, 9) form of a ``Cell``."""
    return box is not None and box.dim() == 2 and box.shape[1] == 9


def is_nearest(box) -> bool:
    """Whether ``box`` as a caller gave it is a ``Cell`` with ``images="nearest"``."""
    return isinstance(box, Cell) and box.nearest


def nearest_of(d0, d1, d2, ax, bx, by, cx, cy, cz):
    """The nearest image of the BRICK image (d0, d1, d2) in plain torch (the host bodies): the shortest of its 27
    translates by squared length, (0, 0, 0) first, then k outermost, j, i innermost from -1 to 1, replaced only by a
    strictly shorter one -- the search of ``nearest_image`` (csrc/aggf_common.h), unpruned (pruning changes no bit).
    The choice is made on detached values; the result is the chosen translate of the given tensors."""
    with torch.no_grad():
        best = d0 * d0 + d1 * d1 + d2 * d2
        pick = torch.zeros(best.shape + (3,), dtype=best.dtype, device=best.device)
        for k in (-1, 0, 1):
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    if i == j == k == 0:
                        continue
                    x, y, z = d0 + k * cx + j * bx + i * ax, d1 + k * cy + j * by, d2 + k * cz
                    q = x * x + y * y + z * z
                    shorter = q < best
                    best = torch.where(shorter, q, best)
                    pick = torch.where(shorter.unsqueeze(-1), torch.tensor([i, j, k], dtype=best.dtype, device=best.device), pick)
        i, j, k = pick[..., 0], pick[..., 1], pick[..., 2]
    return d0 + k * cx + j * bx + i * ax, d1 + k * cy + j * by, d2 + k * cz


def refuse_cell(box, who: str) -> None:
    """``ValueError`` if ``box`` is a ``Cell``: ``who`` names a function under which triclinic cells are not built."""
    if isinstance(box, Cell):
        raise ValueError(f"{who}: triclinic cells are not built here; it takes the lengths of an orthorhombic box, "
                         "(3,) or (n_steps, 3)")


def check_reach(box, outer, who: str) -> None:
    """``ValueError`` if ``box`` is a ``Cell`` on the host whose image is not the minimum image all the way to
    ``outer``: ``outer`` must not exceed ``image_radius`` (``safe_radius`` for brick images, half the shortest lattice
    vector for ``images="nearest"``).  Lengths of an orthorhombic box, a cell on a GPU (not read here) and an ``outer``
    of None pass."""
    if not isinstance(box, Cell) or box.is_cuda or outer is None or box.vectors.numel() == 0:
        return
    radius = box.image_radius
    if float(outer) > radius:
        raise ValueError(f"{who}: outer={float(outer):g} reaches beyond image_radius={radius:g} of the triclinic cell "
                         f"(images={box.images!r}): past it the cell's image is not the minimum image and the feature "
                         "would be that of a wrong image"
                         + ("" if box.nearest else '; Cell(..., images="nearest") reaches half the shortest lattice vector'))


def cell_good(rows: torch.Tensor) -> torch.Tensor:
    """(n_steps,) bool: the frames of an (n_steps, 9) cell that are good by the kernels' rule (the six lower-triangular
    entries alone: diagonal positive and finite, off-diagonal finite)."""
    diag, low = rows[:, [0, 4, 8]], rows[:, [3, 6, 7]]
    return (torch.isfinite(diag) & (diag > 0)).all(dim=1) & torch.isfinite(low).all(dim=1)
