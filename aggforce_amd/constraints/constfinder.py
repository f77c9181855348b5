"""Guess constrained bonds from coordinate fluctuations (reference: constraints/constfinder.py:14-57).

Pairs of sites whose distance has a standard deviation over the trajectory below ``threshold`` are
taken to be constrained.  The reference materialises all (n_steps, n_sites, n_sites) distances; here
the per-pair variance comes from one streaming GPU pass (K6, ``aggf_pair_dist_var``), so the default
``project_forces(constrained_inds="auto")`` also works on full-size trajectories.  With ``cross_xyz``
(two different systems; not on the force-map path) the small host computation is kept.  With ``box`` the
distances are minimum-image distances under an orthorhombic periodic cell (the box form of K6,
``aggf_pair_dist_var_pbc``): the guess then also holds on trajectories wrapped into their cell.
"""
from typing import Union

import numpy as np

from ..util import distances
from .hints import Constraints


def _host_lengths(lengths) -> np.ndarray:
    """The checked box of ``jaxutil._as_box`` as a float64 NumPy array that broadcasts against (T, m, n, 3)."""
    L = lengths.detach().cpu().double().numpy()
    return L if L.ndim == 1 else L.reshape((L.shape[0], 1, 1, 3))


def guess_pairwise_constraints(xyz, cross_xyz: Union[None, np.ndarray] = None, threshold: float = 1e-3,
                               comm=None, box=None) -> Constraints:
    """Pairs of sites whose distance fluctuates by less than ``threshold`` (standard deviation).

    Returns a set of frozensets {i, j}; with ``cross_xyz`` a set of ordered tuples (i, j) with i
    indexing ``cross_xyz`` and j indexing ``xyz`` (as the reference).  ``comm`` (extra): ``xyz`` is this
    rank's shard of a frame-sharded trajectory; the per-rank means and variances are combined exactly
    (two all-reduces of (N, N)), so every rank gets the set the whole trajectory gives.

    ``box`` (extra): the lengths of an orthorhombic periodic cell, (3,) or (n_steps, 3) -- a sequence, an
    array or a tensor (with ``comm``: this rank's rows).  Every distance is then that of the minimum image
    (``d - L rint(d / L)`` per component, in float64), so a rigid pair that a wrapped trajectory splits across
    a face in some frames is still found; without it such a pair's distance jumps by a box length and the
    pair is silently dropped.  Shape and host values are checked before any device work; a box on a GPU is
    checked there.  Lengths that are not positive and finite raise ValueError.

    ``box`` may be a ``pbc.Cell`` (a triclinic cell): every distance is then that of the brick image (``pbc``), in
    float64 on the triclinic form of K6 -- the minimum-image distance for pairs closer than ``cell.safe_radius``,
    which every rigid pair of a molecule is.  A cell with a bad frame raises ValueError, as bad lengths do; with
    ``comm`` a ``Cell`` is refused (not built).  A cell with ``images="nearest"`` is accepted and measured in the
    same brick form: a rigid pair is shorter than ``safe_radius``, where the two images coincide.
    """
    lengths = None
    if box is not None:
        from .._cell import Cell, cell_good, is_cell_rows
        from ..jaxutil import _as_box, _wrap

        if isinstance(box, Cell) and comm is not None:
            raise ValueError("guess_pairwise_constraints: triclinic cells are not built with comm= (frames sharded "
                             "over ranks); guess on one rank")

        lengths = _as_box(box, int(xyz.shape[0]) if hasattr(xyz, "shape") else len(xyz))
    if cross_xyz is not None:
        x = xyz.detach().cpu().numpy() if hasattr(xyz, "detach") else np.asarray(xyz)
        c = cross_xyz.detach().cpu().numpy() if hasattr(cross_xyz, "detach") else np.asarray(cross_xyz)
        if lengths is None:
            dist = distances(x, cross_xyz=c)
        else:
            disp = distances(x, cross_xyz=c, return_displacements=True).astype(np.float64)
            if is_cell_rows(lengths):
                import torch

                rows = lengths.detach().cpu().double()
                if not bool(cell_good(rows).all()):  # (a cell that came from a GPU)
                    raise ValueError("the cell's diagonal must be positive and finite, its lower triangle finite")
                disp = _wrap(torch.from_numpy(disp), rows).numpy()
            else:
                L = _host_lengths(lengths)
                if not (np.isfinite(L) & (L > 0)).all():  # (a box that came from a GPU)
                    raise ValueError("box lengths must be positive and finite")
                disp = disp - L * np.rint(disp / L)
            dist = np.sqrt(np.sum(disp * disp, axis=-1))
        spread = np.std(dist, axis=0)
        first, second = np.nonzero(spread < threshold)
        return {(int(i), int(j)) for i, j in zip(first, second)}
    import torch
    from .. import _kernels as K

    from ..distributed import all_reduce_sum_, world_size

    x = K.as_device(xyz)
    if lengths is not None:
        on_device = lengths.is_cuda
        lengths = lengths.to(device=x.device, dtype=x.dtype).contiguous()
        # (a box that was on the host is checked already; this function synchronises for its result anyway)
        if on_device and is_cell_rows(lengths):
            if not bool(cell_good(lengths).all()):
                raise ValueError("the cell's diagonal must be positive and finite, its lower triangle finite")
        elif on_device and not bool((torch.isfinite(lengths) & (lengths > 0)).all()):
            raise ValueError("box lengths must be positive and finite")
    if world_size(comm) > 1:
        # exact pooling of the per-rank (n_r, mean_r, var_r):  var = sum_r (n_r / n) (var_r + (mean_r - mean)^2)
        mean_r, var_r = K.pair_dist_moments(x, box=lengths)
        n = torch.full((1,), float(x.shape[0]), dtype=torch.float64, device=x.device)
        all_reduce_sum_(n, comm)
        weight = float(x.shape[0]) / float(n.item())
        mean = K.axpby(weight, mean_r, 0.0, mean_r)
        all_reduce_sum_(mean, comm)
        var = K.pair_pool_term(var_r, mean_r, mean, weight)
        all_reduce_sum_(var, comm)
    else:
        var = K.pair_dist_var(x, box=lengths)
    close = var < float(threshold) * float(threshold)  # std < threshold
    close.fill_diagonal_(False)
    idx = torch.nonzero(torch.triu(close, diagonal=1)).cpu().numpy()
    return {frozenset((int(i), int(j))) for i, j in idx}
