"""Module path of the reference's JAX featuriser (qp/jaxfeat.py): ``gb_feat`` is the HIP one (``gbfeat``), and the
array functions it is made of -- ``clipped_gauss``, ``gaussian_dist_basis``, ``channel_allocate``, ``gb_subfeat``,
``gb_subfeat_jac`` -- take tensors and return tensors, as ``jaxutil`` does.

float32 / float64 GPU tensors run on the K10 kernels through the autograd Functions ``Basis`` / ``BasisDot`` of
``_autograd`` and are differentiable to any order (the q-th derivative of a clipped Gaussian is a Hermite polynomial
times the Gaussian; the kernels take q at run time).  ``gb_subfeat`` never forms the one-hot array of its collapsed
form, and writes the channelised form once, zeros included.  CPU tensors and NumPy arrays run the same expressions in
plain torch; the smear step goes through ``jaxutil.trjdot`` and needs the device, as ``trjdot`` does.

Two conventions differ from JAX on sets of measure zero.  At a zero distance the direction (r - cg) / |r - cg| has
weight 0 (``PairDist``'s convention; JAX gives NaN), and at the tie exp(-z^2) == clip the derivative is 0 (JAX's
``maximum`` gives half of it).  Centres, width and clip are constants, as in the reference, where they are Python
floats under ``jit``.

``box=`` (a keyword of ``gb_subfeat`` / ``gb_subfeat_jac``; not in the reference): the lengths of an orthorhombic box,
or a ``pbc.Cell`` -- the distances are then those of the cell's image, brick or nearest (``jaxutil.distances_in_box``:
K9c on the GPU), and a host cell whose ``image_radius`` is less than ``outer`` is refused, as in ``gb_feat``.
"""
from functools import lru_cache
from typing import Optional, Tuple, Union

import numpy as np
import torch

from .. import _kernels as K
from .._cell import check_reach, is_nearest
from ..jaxutil import _as_box, _wrap, distances, distances_in_box, trjdot
from .gbfeat import gb_centers, gb_feat

__all__ = ["gb_feat", "clipped_gauss", "gaussian_dist_basis", "channel_allocate", "gb_subfeat", "gb_subfeat_jac"]

DIVMETHOD_REORDER = "reorder"
DIVMETHOD_BASIC = "basic"

_NP_OF = {torch.float32: np.float32, torch.float64: np.float64}


def _tensor(x, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A float32 / float64 tensor (on the device of ``like``); torch inputs keep their autograd history."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dtype not in _NP_OF:
        t = t.to(torch.float64)
    return t if like is None or t.device == like.device else t.to(like.device)


def _on_kernels(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype in _NP_OF


@lru_cache(maxsize=64)
def _spec(device: str, dtype: torch.dtype, centers: Tuple[float, ...], width: float, clip: Optional[float],
          channels: Optional[Tuple[int, ...]], n_slots: Optional[int]) -> "K.BasisSpec":
    cen = torch.tensor(centers, dtype=torch.float64).to(dtype).to(device)
    return K.BasisSpec(cen, width, clip, channels, n_slots)


def _grid(dtype: torch.dtype, outer, inner, n_basis, dist_power) -> Tuple[float, ...]:
    """The centres as ``gb_centers`` computes them in ``dtype`` (exact as Python floats)."""
    return tuple(float(c) for c in gb_centers(float(outer), float(inner), int(n_basis), float(dist_power), _NP_OF[dtype]))


def _basis_spec(d: torch.Tensor, centers: Tuple[float, ...], width, clip, channels=None, n_slots=None) -> "K.BasisSpec":
    K.lib()
    ch = None if channels is None else tuple(int(c) for c in channels)
    return _spec(str(d.device), d.dtype, centers, float(width), None if clip is None else float(clip), ch,
                 None if n_slots is None else int(n_slots))


def _plain_basis(d: torch.Tensor, centers: Tuple[float, ...], width, clip, q: int = 0) -> torch.Tensor:
    """The value (q = 0) or first derivative (q = 1) of the clipped Gaussians in plain torch, d.shape + (n_basis,)."""
    cen = torch.tensor(centers, dtype=torch.float64).to(d.dtype).to(d.device)
    z = (d[..., None] - cen) / width
    gauss = torch.exp(-(z**2))
    floor = 0.0 if clip is None else float(clip)
    if q == 0:
        return gauss if clip is None else torch.clamp(gauss, min=floor) - floor
    return torch.where(gauss > floor, (-2.0 / width) * z * gauss, torch.zeros_like(gauss))


def clipped_gauss(inp, center, width=1.0, clip=1e-3):
    """max(exp(-((inp - center) / width)**2), clip) - clip, in the shape of ``inp`` (reference jaxfeat.py:244-276);
    ``clip=None``: the Gaussian itself."""
    t = _tensor(inp)
    centers = (float(np.asarray(center, dtype=_NP_OF[t.dtype])),)
    if _on_kernels(t):
        from .._autograd import Basis

        return Basis.apply(None, t, 0, _basis_spec(t, centers, width, clip), False)[..., 0]
    return _plain_basis(t, centers, width, clip)[..., 0]


def gaussian_dist_basis(dists, outer, inner=0, n_basis=10, width=1.0, dist_power=0.5, clip=1e-3):
    """Distances of any shape -> ``dists.shape + (n_basis,)`` clipped Gaussians (reference jaxfeat.py:188-240).  The
    centres are ``linspace(inner**p, outer**p, n_basis) ** (1/p)`` with p = ``dist_power``, in the dtype of ``dists``.
    Distances outside [inner, outer] are not clipped.  GPU tensors: one kernel, differentiable to any order."""
    t = _tensor(dists)
    centers = _grid(t.dtype, outer, inner, n_basis, dist_power)
    if _on_kernels(t):
        from .._autograd import Basis

        return Basis.apply(None, t, 0, _basis_spec(t, centers, width, clip), False)
    return _plain_basis(t, centers, width, clip)


def _kept(channels, max_channels: int):
    """(sites, their channels) of the sites whose channel has a block in a row of ``max_channels`` blocks."""
    ch = np.asarray(channels, dtype=np.int64).reshape(-1)
    sites = np.flatnonzero((ch >= 0) & (ch < int(max_channels)))
    return sites, ch[sites]


def channel_allocate(feats, channels, max_channels, jac_shape=False):
    """Per-site features -> their one-hot-like form (reference jaxfeat.py:282-368): site ``a`` with channel ``ch(a)``
    puts its ``n_feats`` values at ``[n_feats * ch, n_feats * (ch + 1))`` of a row of ``n_feats * max_channels`` zeros.
    A channel ``>= max_channels`` gets nothing (the reference's out-of-range slice).

    ``feats`` (n_frames, n_sites, n_feats) -> (n_frames, n_sites, n_feats * max_channels); with ``jac_shape``
    (n_feats, n_frames, n_sites, n_dim) -> (n_feats * max_channels, n_frames, n_sites, n_dim).  Index arithmetic in
    torch on the device of ``feats``; ``gb_subfeat`` does not come through here on the GPU (K10a writes this layout)."""
    t = _tensor(feats)
    mc = int(max_channels)
    sites, ch = _kept(channels, mc)
    sites_t = torch.from_numpy(sites).to(t.device)
    ch_t = torch.from_numpy(ch).to(t.device)
    if jac_shape:
        n_feats, n_frames, n_sites, n_dim = t.shape
        out = t.new_zeros((mc, n_feats, n_frames, n_sites, n_dim))
        if len(sites):
            out[ch_t, :, :, sites_t] = t[:, :, sites_t, :].permute(2, 0, 1, 3)
        return out.reshape(mc * n_feats, n_frames, n_sites, n_dim)
    n_frames, n_sites, n_feats = t.shape
    out = t.new_zeros((n_frames, n_sites, mc, n_feats))
    if len(sites):
        out[:, sites_t, ch_t] = t[:, sites_t, :]
    return out.reshape(n_frames, n_sites, mc * n_feats)


def _basis_kwargs(outer, inner=0, n_basis=10, width=1.0, dist_power=0.5, clip=1e-3):
    return outer, inner, n_basis, width, dist_power, clip


def _site_distances(points, cg_points, smear_mat, box=None):
    """(smeared points, first cg site (T, 1, 3), their distances (T, N)); under ``box`` the minimum-image distances."""
    if smear_mat is not None:
        if isinstance(points, torch.Tensor) and not isinstance(smear_mat, torch.Tensor):
            smear_mat = _tensor(smear_mat, points).to(_tensor(points).dtype)  # (a NumPy constant takes the tensor's dtype)
        points = trjdot(points, smear_mat)
    p = _tensor(points)
    cg = _tensor(cg_points, p)[:, :1, :]
    if box is not None:
        return p, cg, distances_in_box(p, box, cross_xyz=cg)[:, 0, :]
    return p, cg, distances(xyz=p, cross_xyz=cg)[:, 0, :]


def gb_subfeat(points, cg_points, channels, max_channels, smear_mat, collapse=False, channelize=True, **kwargs):
    """Gaussian-bin features of the distances of the (smeared) sites to the FIRST site of ``cg_points`` (reference
    jaxfeat.py:383-464): ``trjdot(points, smear_mat)`` (skipped for None), ``distances``, ``gaussian_dist_basis(**kwargs)``,
    ``channel_allocate`` unless ``channelize=False``, the sum over frames and sites if ``collapse``.

    (n_frames, n_sites, n_features), (n_features,) collapsed; 2-D ``points`` get and lose a dummy frame axis.  GPU
    tensors are differentiable to any order in ``points``, ``cg_points`` and ``smear_mat``; the channelised form is
    written by one kernel and the collapsed one summed by one, without the one-hot array.

    ``box`` (a keyword among ``kwargs``, so that the signature stays the reference's; not in the reference; (3,) or
    (n_frames, 3), a constant; default None): the distances are minimum-image distances under
    that orthorhombic cell (``jaxutil.distances_in_box``), as ``gb_feat(box=)`` measures them.  A ``pbc.Cell``: the
    image distances of that triclinic cell, brick or nearest; a host cell with ``outer`` beyond its ``image_radius`` is
    refused (``ValueError``), as in ``gb_feat``."""
    box = kwargs.pop("box", None)
    outer, inner, n_basis, width, dist_power, clip = _basis_kwargs(**kwargs)
    check_reach(box, outer, "gb_subfeat")
    dummy_axis = len(points.shape) == 2
    if dummy_axis:
        points = points[None, ...]
    _, _, r = _site_distances(points, cg_points, smear_mat, box)
    centers = _grid(r.dtype, outer, inner, n_basis, dist_power)
    if _on_kernels(r):
        from .._autograd import Basis

        slots = (channels, max_channels) if channelize else (None, None)
        if channelize and int(max_channels) < 1:
            out = r.new_zeros((0,) if collapse else tuple(r.shape) + (0,))
        else:
            out = Basis.apply(None, r, 0, _basis_spec(r, centers, width, clip, *slots), bool(collapse))
        out = out.reshape(-1) if collapse else out
    else:
        out = _plain_basis(r, centers, width, clip)
        if channelize:
            out = channel_allocate(out, channels, max_channels)
        if collapse:
            out = out.sum(dim=(0, 1))
    return out[0, ...] if dummy_axis and not collapse else out


def gb_subfeat_jac(points, cg_points, channels, max_channels, smear_mat=None, method=DIVMETHOD_REORDER, **kwargs):
    """Per-frame divergences of ``gb_subfeat``, (n_frames, n_features, 3) (reference jaxfeat.py:467-567, where they
    are Jacobians of the collapsed features summed over the sites).  Here in closed form: with S = ``smear_mat``
    (identity for None), p = S points, u = p - cg, r = |u| and W[t,a',k,:] = g'_k(r[t,a']) u[t,a',:] / r[t,a'],

        ``method="reorder"``  div[t,(ch,k),:] = sum_a' (sum_{a: ch(a) = ch} S[a',a]) W[t,a',k,:]
        ``method="basic"``    div[t,(ch,k),:] = sum_{a': ch(a') = ch} (sum_a S[a',a]) W[t,a',k,:]

    over the channels below ``max_channels``.  At r = 0 the weight is 0 (the reference gives NaN).  Differentiable as
    ``gb_subfeat`` is.  ``box`` (a keyword among ``kwargs``, as in ``gb_subfeat``): u is the minimum-image displacement u - L rint(u / L) and r its
    length; under a ``pbc.Cell`` u is the cell's image of the displacement, brick or nearest (``_cell.nearest_of``), with
    the rule on ``outer`` of ``gb_subfeat``."""
    if method not in (DIVMETHOD_BASIC, DIVMETHOD_REORDER):
        raise ValueError("Unknown method for jacobian calculation.")
    box = kwargs.pop("box", None)
    outer, inner, n_basis, width, dist_power, clip = _basis_kwargs(**kwargs)
    check_reach(box, outer, "gb_subfeat_jac")
    p, cg, r = _site_distances(points, cg_points, smear_mat, box)
    centers = _grid(r.dtype, outer, inner, n_basis, dist_power)
    if _on_kernels(r):
        from .._autograd import Basis

        slope = Basis.apply(None, r, 1, _basis_spec(r, centers, width, clip), False)
    else:
        slope = _plain_basis(r, centers, width, clip, q=1)
    pos = r > 0
    disp = p - cg if box is None else _wrap(p - cg, _as_box(box, p.shape[0]), is_nearest(box))  # (the image is locally constant)
    unit = torch.where(pos[..., None], disp / torch.where(pos, r, torch.ones_like(r))[..., None],
                       torch.zeros_like(p))
    weights = slope[..., None] * unit[:, :, None, :]                            # (T, N, n_basis, 3)
    n_frames, n_sites, nb = slope.shape
    mc = int(max_channels)
    sites, ch = _kept(channels, mc)
    onehot = torch.zeros((mc, n_sites), dtype=r.dtype, device=r.device)
    onehot[torch.from_numpy(ch).to(r.device), torch.from_numpy(sites).to(r.device)] = 1
    if smear_mat is None:
        factor = onehot
    else:
        smear = _tensor(smear_mat, r).to(r.dtype)
        factor = onehot @ smear.t() if method == DIVMETHOD_REORDER else onehot * smear.sum(dim=1)[None, :]
    stacked = weights.permute(2, 0, 1, 3).reshape(nb * n_frames, n_sites, 3)
    if mc == 0 or n_frames == 0:
        return r.new_zeros((n_frames, mc * nb, 3))
    if stacked.is_cuda:
        mapped = trjdot(stacked, factor)                                          # (n_basis T, mc, 3)
    else:
        mapped = torch.einsum("tfd,cf->tcd", stacked, factor)
    return mapped.reshape(nb, n_frames, mc, 3).permute(1, 2, 0, 3).reshape(n_frames, mc * nb, 3)
