"""Differentiable map application: five ``torch.autograd.Function``s over the HIP contractions.

Each Function is one kernel launch; the backward of each calls only these same Functions, so the set is closed under
differentiation (``gradgradcheck``, force-matching double backward).  Shapes: points (T, N, 3), a 2-D map (n_cg, N),
a per-frame factor (T, n_cg, N), mapped arrays (T, n_cg, 3).

==============  ==========================================  =================================================
Function        forward                                     backward (upstream gradient H)
==============  ==========================================  =================================================
Apply(P, M)     out[t,c,d] = sum_a M[c,a] P[t,a,d]   (K3)   dP = Apply(H, M'),      dM = Cross(H, P)
Cross(G, P)     out[c,a] = sum_{t,d} G[t,c,d] P[t,a,d] K8a  dG = Apply(P, H),       dP = Apply(G, H')
ApplyFrames     out[t,c,d] = sum_a F[t,c,a] P[t,a,d] (K3c)  dP = FramesT(H, F),     dF = Outer(H, P)
FramesT(G, F)   out[t,a,d] = sum_c F[t,c,a] G[t,c,d] (K8b)  dG = ApplyFrames(H, F), dF = Outer(G, H)
Outer(G, P)     out[t,c,a] = sum_d G[t,c,d] P[t,a,d] (K8c)  dG = ApplyFrames(P, H), dP = FramesT(G, H)
==============  ==========================================  =================================================

Forward outputs have NumPy's promoted dtype; every gradient is returned in its input's dtype (the K8 kernels narrow in
their epilogue, K3 and K3c results are cast).  A gradient autograd does not ask for is not computed: a constant map
never launches K8a.  All launches go to the current stream.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _kernels as K


def _promote(a: torch.Tensor, b: torch.Tensor, out_dtype: Optional[torch.dtype] = None) -> torch.dtype:
    ct = torch.promote_types(a.dtype, b.dtype)
    return ct if out_dtype is None else torch.promote_types(ct, out_dtype)


def _widened(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return x.to(dtype).contiguous()


def _as(x: Optional[torch.Tensor], dtype: torch.dtype) -> Optional[torch.Tensor]:
    return x if x is None or x.dtype == dtype else x.to(dtype)


class Apply(torch.autograd.Function):
    """out[t,c,d] = sum_a M[c,a] P[t,a,d] on K3 (``aggf_linearmap_apply``).  ``MT``: a contiguous M' in the output
    dtype for the transposed apply of the backward (a cached constant; ignored when M itself is differentiated).
    ``probe``: a zeroed int32 flag from ``_kernels.take_flag`` that K3 sets when it meets a NaN."""

    @staticmethod
    def forward(ctx, P, M, MT=None, probe=None):
        out_t = _promote(P, M)
        y = K.linearmap_apply(P.contiguous(), _widened(M, out_t), nan_probe=probe)
        ctx.save_for_backward(P, M, MT)
        return y

    @staticmethod
    def backward(ctx, H):
        P, M, MT = ctx.saved_tensors
        dP = dM = None
        if ctx.needs_input_grad[0]:
            # (the cached transpose is a constant: not when the backward itself is differentiated in M)
            const_m = not (M.requires_grad and torch.is_grad_enabled())
            mt = MT if MT is not None and MT.dtype == _promote(H, M) and const_m else M.t()
            dP = _as(Apply.apply(H, mt), P.dtype)
        if ctx.needs_input_grad[1]:
            dM = Cross.apply(H, P, M.dtype)
        return dP, dM, None, None


class Cross(torch.autograd.Function):
    """out[c,a] = sum_{t,d} G[t,c,d] P[t,a,d] on K8a (``aggf_trjdot_cross``), in ``out_dtype`` (default: promoted)."""

    @staticmethod
    def forward(ctx, G, P, out_dtype=None):
        ct = _promote(G, P)
        y = K.trjdot_cross(_widened(G, ct), _widened(P, ct), out_dtype or ct)
        ctx.save_for_backward(G, P)
        return y

    @staticmethod
    def backward(ctx, H):
        G, P = ctx.saved_tensors
        dG = dP = None
        if ctx.needs_input_grad[0]:
            dG = _as(Apply.apply(P, H), G.dtype)
        if ctx.needs_input_grad[1]:
            dP = _as(Apply.apply(G, H.t()), P.dtype)
        return dG, dP, None


class ApplyFrames(torch.autograd.Function):
    """out[t,c,d] = sum_a F[t,c,a] P[t,a,d] on K3c (``aggf_trjdot_frames``)."""

    @staticmethod
    def forward(ctx, P, F):
        y = K.trjdot_frames(P.contiguous(), F.contiguous())
        ctx.save_for_backward(P, F)
        return y

    @staticmethod
    def backward(ctx, H):
        P, F = ctx.saved_tensors
        dP = dF = None
        if ctx.needs_input_grad[0]:
            dP = FramesT.apply(H, F, P.dtype)
        if ctx.needs_input_grad[1]:
            dF = Outer.apply(H, P, F.dtype)
        return dP, dF


class FramesT(torch.autograd.Function):
    """out[t,a,d] = sum_c F[t,c,a] G[t,c,d] on K8b (``aggf_trjdot_frames_t``), in ``out_dtype`` (default: promoted)."""

    @staticmethod
    def forward(ctx, G, F, out_dtype=None):
        ct = _promote(G, F, out_dtype)  # (the kernels narrow, never widen)
        y = K.trjdot_frames_t(_widened(G, ct), _widened(F, ct), out_dtype or ct)
        ctx.save_for_backward(G, F)
        return y

    @staticmethod
    def backward(ctx, H):
        G, F = ctx.saved_tensors
        dG = dF = None
        if ctx.needs_input_grad[0]:
            dG = _as(ApplyFrames.apply(H, F), G.dtype)
        if ctx.needs_input_grad[1]:
            dF = Outer.apply(G, H, F.dtype)
        return dG, dF, None


class Outer(torch.autograd.Function):
    """out[t,c,a] = sum_d G[t,c,d] P[t,a,d] on K8c (``aggf_trjdot_frames_outer``), in ``out_dtype`` (default:
    promoted)."""

    @staticmethod
    def forward(ctx, G, P, out_dtype=None):
        ct = _promote(G, P, out_dtype)
        y = K.trjdot_frames_outer(_widened(G, ct), _widened(P, ct), out_dtype or ct)
        ctx.save_for_backward(G, P)
        return y

    @staticmethod
    def backward(ctx, H):
        G, P = ctx.saved_tensors
        dG = dP = None
        if ctx.needs_input_grad[0]:
            dG = _as(ApplyFrames.apply(P, H), G.dtype)
        if ctx.needs_input_grad[1]:
            dP = FramesT.apply(G, H, P.dtype)
        return dG, dP, None
