"""Differentiable array helpers at the reference's module path (reference: jaxutil.py).

The reference differentiates these through JAX; here the array type is the torch tensor and ``trjdot`` runs on the
HIP kernels through the autograd Functions of ``_autograd`` (K3 / K3c forward, K8 backward), differentiable in both
arguments to any order.  ``distances`` of GPU tensors runs on K9 through ``PairDist`` / ``PairPull`` / ``PairDot``:
no (T, m, n, 3) displacement array is formed, forward or backward, and a zero distance (the diagonal of a self-distance
matrix, coincident sites) has gradient 0 at every order -- plain torch returns NaN from the second order on.  Its
other forms (``return_displacements``, CPU tensors, NumPy inputs, other dtypes) and ``abatch`` are plain torch code:
autograd handles them.
"""
from typing import Callable, Union

import numpy as np
import torch

from . import _kernels as K

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


def distances(
    xyz: torch.Tensor,
    cross_xyz: Union[torch.Tensor, None] = None,
    return_matrix: bool = True,
    return_displacements: bool = False,
    square: bool = False,
) -> torch.Tensor:
    """Differentiable per-frame distances (reference jaxutil.py:103-187): (n_steps, n_sites, n_sites) matrices, or
    (n_steps, other_n_sites, n_sites) with ``cross_xyz``, or the flattened upper triangles (``return_matrix=False``);
    displacements (one more trailing axis) with ``return_displacements``; squared distances with ``square``."""
    if cross_xyz is not None and not return_matrix:
        raise ValueError("Cross distances only supported when return_matrix is truthy.")
    if return_displacements and not return_matrix:
        raise ValueError("Displacements only supported when return_matrix is truthy.")
    if not return_displacements and _on_kernels(xyz) and (cross_xyz is None or _on_kernels(cross_xyz, xyz)):
        from ._autograd import PairDist

        K.lib()
        dist = PairDist.apply(xyz, xyz if cross_xyz is None else cross_xyz, bool(square))
        return dist if return_matrix else _upper_triangles(dist)
    xyz = xyz if isinstance(xyz, torch.Tensor) else torch.as_tensor(np.asarray(xyz))
    if cross_xyz is None:
        disp = xyz[:, None, :, :] - xyz[:, :, None, :]
    else:
        cross_xyz = cross_xyz if isinstance(cross_xyz, torch.Tensor) else torch.as_tensor(np.asarray(cross_xyz))
        disp = xyz[:, None, :, :] - cross_xyz[:, :, None, :]
    if return_displacements:
        return disp
    if square:
        dist = (disp**2).sum(dim=-1)
    else:
        dist = torch.linalg.vector_norm(disp, dim=-1)
    return dist if return_matrix else _upper_triangles(dist)
