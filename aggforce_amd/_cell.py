"""Triclinic periodic cells (not in the reference): the ``Cell`` that every ``box=`` of the pair-distance, cutoff-list,
whole-molecule and constraint-guess functions takes beside the lengths of an orthorhombic box (``pbc.Cell``).

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
  ``cutoff <= safe_radius`` is exact.  An exact minimum image beyond that radius is not built.

This is what OpenMM and GROMACS do inside their cutoffs, and the "shorter than half the cell" condition that
``make_whole`` documents for bonds.  Not built under a cell: ``gb_feat`` / ``qp.jaxfeat.gb_subfeat`` (K4), ``comm=``
(frames sharded over ranks), gradients with respect to the cell.
"""
from __future__ import annotations

import numpy as np
import torch


class Cell:
    """A triclinic periodic cell, one for all frames or one per frame: ``Cell(vectors)`` with ``vectors`` (3, 3) or
    (n_steps, 3, 3), rows ``a, b, c``, as a sequence, a NumPy array or a tensor.

    A cell on the host is checked here -- ``ValueError`` for a wrong shape, non-numbers, a nonzero upper-triangular
    entry, a diagonal entry that is not positive and finite, any non-finite entry -- and kept as float64.  A cell on a
    GPU is taken as it is, with no synchronisation: the kernels read its six lower-triangular entries, and a frame
    whose diagonal entry is not positive and finite, or whose lower off-diagonal entry is not finite, comes out NaN
    (image counts 0) and no other frame.  The cell is a constant: one that requires a gradient is refused.

    A class, not a raw array, because a raw (3, 3) array given as ``box=`` to three frames already means one
    orthorhombic box per frame."""

    def __init__(self, vectors):
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
        self._v = v.detach()

    @classmethod
    def from_lengths_angles(cls, lengths, angles_deg) -> "Cell":
        """The cell of edge lengths (A, B, C) and angles (alpha, beta, gamma) in degrees, (3,) or (n_steps, 3) each
        (alpha between b and c, beta between a and c, gamma between a and b), by the standard conversion in float64:
        a = (A, 0, 0), b = (B cos gamma, B sin gamma, 0), cx = C cos beta, cy = C (cos alpha - cos beta cos gamma) /
        sin gamma, cz = sqrt(C^2 - cx^2 - cy^2).  An angle of exactly 90 degrees gives an exact zero."""
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
        return cls(v)

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

    def take(self, frames) -> "Cell":
        """The cell of the frames ``frames`` (an index array): itself unless it is per frame."""
        if not self.is_per_frame:
            return self
        return Cell(self._v[torch.as_tensor(np.asarray(frames), device=self._v.device)])

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
        return f"Cell({'per frame, ' if self.is_per_frame else ''}vectors={self._v.tolist() if self._v.numel() <= 9 else '...'})"


def is_cell_rows(box) -> bool:
    """Whether a normalised box (``jaxutil._as_box``) is the (n_steps, 9) form of a ``Cell``."""
    return box is not None and box.dim() == 2 and box.shape[1] == 9


def refuse_cell(box, who: str) -> None:
    """``ValueError`` if ``box`` is a ``Cell``: ``who`` names a function under which triclinic cells are not built."""
    if isinstance(box, Cell):
        raise ValueError(f"{who}: triclinic cells are not built here; it takes the lengths of an orthorhombic box, "
                         "(3,) or (n_steps, 3)")


def cell_good(rows: torch.Tensor) -> torch.Tensor:
    """(n_steps,) bool: the frames of an (n_steps, 9) cell that are good by the kernels' rule (the six lower-triangular
    entries alone: diagonal positive and finite, off-diagonal finite)."""
    diag, low = rows[:, [0, 4, 8]], rows[:, [3, 6, 7]]
    return (torch.isfinite(diag) & (diag > 0)).all(dim=1) & torch.isfinite(low).all(dim=1)
