"""Differentiable map application, pair distances, radial basis and the unwrap: fourteen ``torch.autograd.Function``s
over the HIP kernels.

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

Pair distances (``jaxutil.distances``): sites X (T, n, 3) and C (T, m, 3) (C is X for the self-distance matrix),
u[t,i,j] = X[t,j] - C[t,i], pair arrays (T, m, n).  No (T, m, n, 3) array is formed by any of them.

==========================  ===============================================  ==========================================
Function                    forward                                          backward (upstream H, or GA and GB)
==========================  ===============================================  ==========================================
PairDist(X, C, square)      D[t,i,j] = |u| or u.u                     (K9a)  (dX, dC) = PairPull(W, X, C), W = 2 H or
                                                                             where(D > 0, H / D, 0)
PairPull(W, X, C) -> A, B   A[t,j] = sum_i W_ij u_ij, B[t,i] = -sum_j (K9b)  dW = PairDot(GA, GB, X, C),
                                                                             (dX, dC) = PairPull(W, GA, GB)
PairDot(V, Y, X, C)         out[t,i,j] = (V[t,j] - Y[t,i]).u          (K9a)  (dV, dY) = PairPull(H, X, C),
                                                                             (dX, dC) = PairPull(H, V, Y)
==========================  ===============================================  ==========================================

The same three over a static list of P pairs (i_p, j_p) shared by all frames (``jaxutil.pair_distances``; the upper
triangles of ``jaxutil.distances`` are the list ``triu_indices``): u[t,p] = X[t,j_p] - C[t,i_p], pair arrays (T, P),
``plist`` a ``jaxutil.PairList`` (a constant).  Nothing of size T m n is formed, forward or backward.

==========================  ===============================================  ==========================================
PairListDist(X, C, plist,   D[t,p] = |u| or u.u                       (K9c)  as PairDist, through PairListPull
  square)
PairListPull(W, X, C,       A[t,j] = sum_{p: j_p = j} W_p u_p,               dW = PairListDot(GA, GB, X, C),
  plist) -> A, B            B[t,i] = -sum_{p: i_p = i} W_p u_p        (K9d)  (dX, dC) = PairListPull(W, GA, GB)
PairListDot(V, Y, X, C,     out[t,p] = (V[t,j_p] - Y[t,i_p]).u        (K9c)  (dV, dY) = PairListPull(H, X, C),
  plist)                                                                     (dX, dC) = PairListPull(H, V, Y)
==========================  ===============================================  ==========================================

The Gaussian radial basis (``qp.jaxfeat``): distances D of any shape, g_k^(q) the q-th derivative of the clipped
Gaussian of centre k (q = 0: the value; q at run time, by the Hermite recurrence), col0(e) = 0, or with channel slots
slot(site of e) * n_basis in a row of n_slots * n_basis values.  ``collapse``: the sum over all elements of a slot.

==========================  ===============================================  ==========================================
Function                    forward                                          backward (upstream H, or G)
==========================  ===============================================  ==========================================
Basis(S, D, q)              out[e, col0 + k] = S[e] g_k^(q)(D[e])    (K10a)  dS = BasisDot(H, D, q),
                            collapse: out[slot, k] = sum_e of that   (K10c)  dD = S * BasisDot(H, D, q + 1)
BasisDot(H, D, q)           out[e] = sum_k H[., k] g_k^(q)(D[e])     (K10b)  dH = Basis(G, D, q),
                            H per element, slotted row or slot table         dD = G * BasisDot(H, D, q + 1)
==========================  ===============================================  ==========================================

MakeWhole(X, box, tree) (``pbc.make_whole``): out = X - k L on K11, k the integer image counts along the bond forest.
The shift is piecewise constant in X, so the backward is the identity (dX = H) and needs no kernel; box is a constant.

A zero distance has weight 0: torch's own first-order value at |0|, and what keeps every higher order finite (the
diagonal of a self-distance matrix does not depend on X at all).  A first-order backward of a distance (grad mode off)
hands H and D to K9b, which divides as it reads: no W array exists.  With grad mode on W is built by torch ops on the
saved D, which is connected to the graph.  PairPull is linear in (X, C), so the squared form's W = 2 H is taken as
PairPull(H, 2 X, 2 C): no (T, m, n) product.

Forward outputs have NumPy's promoted dtype; every gradient is returned in its input's dtype (the K8 kernels narrow in
their epilogue, K9b does the same, K3, K3c and K9a results are cast).  A gradient autograd does not ask for is not
computed: a constant map never launches K8a, and K9b skips the sum whose pointer is null.  All launches go to the current stream.
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


# ------------------------------------------------------------------ pair distances (K9)
def _pair_dtype(*arrays) -> torch.dtype:
    ct = arrays[0].dtype
    for a in arrays[1:]:
        ct = torch.promote_types(ct, a.dtype)
    return ct


def _pull_dtype(ct: torch.dtype, x: torch.Tensor, c: torch.Tensor, want_x: bool, want_c: bool) -> torch.dtype:
    """The one output dtype of a K9b call whose A goes to x and whose B goes to c: theirs if the wanted ones agree."""
    wanted = {t.dtype for t, w in ((x, want_x), (c, want_c)) if w}
    return wanted.pop() if len(wanted) == 1 else ct


def _zeros_if_none(g: Optional[torch.Tensor], like: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return torch.zeros(like.shape, dtype=dtype, device=like.device) if g is None else g


class PairDist(torch.autograd.Function):
    """D[t,i,j] = |X[t,j] - C[t,i]| (``square``: squared) on K9a (``aggf_pair_dist``), in the promoted dtype."""

    @staticmethod
    def forward(ctx, X, C, square=False):
        ct = _pair_dtype(X, C)
        D = K.pair_dist(_widened(X, ct), _widened(C, ct), K.PAIR_SQDIST if square else K.PAIR_DIST)
        ctx.square = bool(square)
        ctx.save_for_backward(X, C, D)
        return D

    @staticmethod
    def backward(ctx, H):
        X, C, D = ctx.saved_tensors
        want_x, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_c):
            return None, None, None
        if ctx.square:
            dX, dC = PairPull.apply(H, 2 * X, 2 * C, want_x, want_c, _pull_dtype(D.dtype, X, C, want_x, want_c))
        elif torch.is_grad_enabled():
            pos = D > 0
            W = torch.where(pos, H / torch.where(pos, D, torch.ones_like(D)), torch.zeros_like(D))
            dX, dC = PairPull.apply(W, X, C, want_x, want_c, _pull_dtype(D.dtype, X, C, want_x, want_c))
        else:
            ct = _pair_dtype(H, D)
            dX, dC = K.pair_pull(_widened(H, ct), _widened(X, ct), _widened(C, ct), dv=_widened(D, ct),
                                 want_a=want_x, want_b=want_c, out_dtype=_pull_dtype(ct, X, C, want_x, want_c))
        return _as(dX, X.dtype), _as(dC, C.dtype), None


class PairPull(torch.autograd.Function):
    """(A, B), A[t,j,:] = sum_i W[t,i,j] u[t,i,j] and B[t,i,:] = -sum_j W[t,i,j] u[t,i,j], on K9b
    (``aggf_pair_pull``), in ``out_dtype`` (default: promoted).  ``want_a`` / ``want_b`` False: that output is None."""

    @staticmethod
    def forward(ctx, W, X, C, want_a=True, want_b=True, out_dtype=None):
        ct = _pair_dtype(W, X, C) if out_dtype is None else torch.promote_types(_pair_dtype(W, X, C), out_dtype)
        A, B = K.pair_pull(_widened(W, ct), _widened(X, ct), _widened(C, ct), want_a=want_a, want_b=want_b,
                           out_dtype=out_dtype or ct)
        ctx.save_for_backward(W, X, C)
        return A, B

    @staticmethod
    def backward(ctx, GA, GB):
        W, X, C = ctx.saved_tensors
        dW = dX = dC = None
        if GA is None and GB is None:
            return None, None, None, None, None, None
        ct = _pair_dtype(W, X, C, *(g for g in (GA, GB) if g is not None))
        GA, GB = _zeros_if_none(GA, X, ct), _zeros_if_none(GB, C, ct)
        if ctx.needs_input_grad[0]:
            dW = _as(PairDot.apply(GA, GB, X, C), W.dtype)
        want_x, want_c = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if want_x or want_c:
            dX, dC = PairPull.apply(W, GA, GB, want_x, want_c, _pull_dtype(ct, X, C, want_x, want_c))
        return dW, _as(dX, X.dtype), _as(dC, C.dtype), None, None, None


class PairDot(torch.autograd.Function):
    """out[t,i,j] = (V[t,j] - Y[t,i]) . (X[t,j] - C[t,i]) on K9a (``aggf_pair_dist``, DOT), in the promoted dtype."""

    @staticmethod
    def forward(ctx, V, Y, X, C):
        ct = _pair_dtype(V, Y, X, C)
        out = K.pair_dist(_widened(X, ct), _widened(C, ct), K.PAIR_DOT, _widened(V, ct), _widened(Y, ct))
        ctx.save_for_backward(V, Y, X, C)
        return out

    @staticmethod
    def backward(ctx, H):
        V, Y, X, C = ctx.saved_tensors
        need = ctx.needs_input_grad
        dV = dY = dX = dC = None
        ct = _pair_dtype(H, V, Y, X, C)
        if need[0] or need[1]:
            dV, dY = PairPull.apply(H, X, C, need[0], need[1], _pull_dtype(ct, V, Y, need[0], need[1]))
        if need[2] or need[3]:
            dX, dC = PairPull.apply(H, V, Y, need[2], need[3], _pull_dtype(ct, X, C, need[2], need[3]))
        return _as(dV, V.dtype), _as(dY, Y.dtype), _as(dX, X.dtype), _as(dC, C.dtype)


# ------------------------------------------------------------------ pair lists (K9c / K9d)
def _tables(plist, like: torch.Tensor) -> "K.PairTables":
    """The device tables of ``plist`` (a ``jaxutil.PairList``, or its ``_kernels.PairTables`` already)."""
    return plist.on(like.device) if hasattr(plist, "on") else plist


def _box_kw(box, ct: torch.dtype, near: bool = False) -> dict:
    """The ``box`` keyword of a kernel call in the call's dtype; with no box, no keyword (the open call as it was).
    ``near``: the nearest-image form of a cell's rows (``pbc.Cell(..., images="nearest")``)."""
    if box is None:
        return {}
    if box.requires_grad:
        raise ValueError("box is a constant: gradients with respect to box lengths are not built")
    return {"box": _widened(box, ct), "near": True} if near else {"box": _widened(box, ct)}


class PairListDist(torch.autograd.Function):
    """D[t,p] = |X[t,j_p] - C[t,i_p]| (``square``: squared) over the pairs of ``plist`` on K9c
    (``aggf_pair_list_dist``), in the promoted dtype.  The backward is PairDist's with the list forms.

    ``box`` ((3,) or (T, 3) tensor on the operands' device, a constant): every displacement of coordinates is its
    minimum image under that box (the box forms of K9c / K9d).  The wrap is locally constant, so a derivative differs
    from the open one only in the displacement it multiplies: the box goes to every call that forms a displacement of
    coordinates, and the pulls whose "sites" are tangents (``PairListPull`` / ``PairListDot`` backward) stay open --
    differences of tangents are not displacements and are never wrapped.  ``near`` (with the (T, 9) rows of a cell): the
    nearest image instead of the brick image, in the forward and -- the backward kernels recompute the displacement --
    in every derivative, which therefore multiply the image the forward chose."""

    @staticmethod
    def forward(ctx, X, C, plist, square=False, box=None, near=False):
        ct = _pair_dtype(X, C)
        D = K.pair_list_dist(_widened(X, ct), _widened(C, ct), _tables(plist, X), K.PAIR_SQDIST if square else K.PAIR_DIST,
                             **_box_kw(box, ct, near))
        ctx.square, ctx.plist, ctx.box, ctx.near = bool(square), plist, box, bool(near)
        ctx.save_for_backward(X, C, D)
        return D

    @staticmethod
    def backward(ctx, H):
        X, C, D = ctx.saved_tensors
        plist, box, near = ctx.plist, ctx.box, ctx.near
        want_x, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_x or want_c):
            return None, None, None, None, None, None
        if ctx.square and box is not None:  # (2 u, not the image of 2 X - 2 C)
            dX, dC = PairListPull.apply(2 * H, X, C, plist, want_x, want_c, _pull_dtype(D.dtype, X, C, want_x, want_c),
                                        box, near)
        elif ctx.square:
            dX, dC = PairListPull.apply(H, 2 * X, 2 * C, plist, want_x, want_c,
                                        _pull_dtype(D.dtype, X, C, want_x, want_c))
        elif torch.is_grad_enabled():
            pos = D > 0
            W = torch.where(pos, H / torch.where(pos, D, torch.ones_like(D)), torch.zeros_like(D))
            dX, dC = PairListPull.apply(W, X, C, plist, want_x, want_c, _pull_dtype(D.dtype, X, C, want_x, want_c),
                                        box, near)
        else:
            ct = _pair_dtype(H, D)
            dX, dC = K.pair_list_pull(_widened(H, ct), _widened(X, ct), _widened(C, ct), _tables(plist, X),
                                      dv=_widened(D, ct), want_a=want_x, want_b=want_c,
                                      out_dtype=_pull_dtype(ct, X, C, want_x, want_c), **_box_kw(box, ct, near))
        return _as(dX, X.dtype), _as(dC, C.dtype), None, None, None, None


class PairListPull(torch.autograd.Function):
    """(A, B), A[t,j,:] = sum_{p: j_p = j} W[t,p] u[t,p] and B[t,i,:] = -sum_{p: i_p = i} W[t,p] u[t,p], on K9d
    (``aggf_pair_list_pull``), in ``out_dtype`` (default: promoted).  ``want_a`` / ``want_b`` False: that output is
    None.  ``box``: u is the minimum image of X[t,j_p] - C[t,i_p] (see ``PairListDist``)."""

    @staticmethod
    def forward(ctx, W, X, C, plist, want_a=True, want_b=True, out_dtype=None, box=None, near=False):
        ct = _pair_dtype(W, X, C) if out_dtype is None else torch.promote_types(_pair_dtype(W, X, C), out_dtype)
        A, B = K.pair_list_pull(_widened(W, ct), _widened(X, ct), _widened(C, ct), _tables(plist, X), want_a=want_a,
                                want_b=want_b, out_dtype=out_dtype or ct, **_box_kw(box, ct, near))
        ctx.plist, ctx.box, ctx.near = plist, box, bool(near)
        ctx.save_for_backward(W, X, C)
        return A, B

    @staticmethod
    def backward(ctx, GA, GB):
        W, X, C = ctx.saved_tensors
        plist, box, near = ctx.plist, ctx.box, ctx.near
        dW = dX = dC = None
        if GA is None and GB is None:
            return None, None, None, None, None, None, None, None, None
        ct = _pair_dtype(W, X, C, *(g for g in (GA, GB) if g is not None))
        GA, GB = _zeros_if_none(GA, X, ct), _zeros_if_none(GB, C, ct)
        if ctx.needs_input_grad[0]:
            dW = _as(PairListDot.apply(GA, GB, X, C, plist, box, near), W.dtype)
        want_x, want_c = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if want_x or want_c:  # (sums of W (GA_j - GB_i): tangents, open under any box)
            dX, dC = PairListPull.apply(W, GA, GB, plist, want_x, want_c, _pull_dtype(ct, X, C, want_x, want_c))
        return dW, _as(dX, X.dtype), _as(dC, C.dtype), None, None, None, None, None, None


class PairListDot(torch.autograd.Function):
    """out[t,p] = (V[t,j_p] - Y[t,i_p]) . (X[t,j_p] - C[t,i_p]) on K9c (``aggf_pair_list_dist``, DOT), in the promoted
    dtype.  ``box``: the second factor is its minimum image; V - Y is never wrapped (see ``PairListDist``)."""

    @staticmethod
    def forward(ctx, V, Y, X, C, plist, box=None, near=False):
        ct = _pair_dtype(V, Y, X, C)
        out = K.pair_list_dist(_widened(X, ct), _widened(C, ct), _tables(plist, X), K.PAIR_DOT, _widened(V, ct),
                               _widened(Y, ct), **_box_kw(box, ct, near))
        ctx.plist, ctx.box, ctx.near = plist, box, bool(near)
        ctx.save_for_backward(V, Y, X, C)
        return out

    @staticmethod
    def backward(ctx, H):
        V, Y, X, C = ctx.saved_tensors
        plist, box, near = ctx.plist, ctx.box, ctx.near
        need = ctx.needs_input_grad
        dV = dY = dX = dC = None
        ct = _pair_dtype(H, V, Y, X, C)
        if need[0] or need[1]:
            dV, dY = PairListPull.apply(H, X, C, plist, need[0], need[1], _pull_dtype(ct, V, Y, need[0], need[1]),
                                        box, near)
        if need[2] or need[3]:  # (sums of H (V_j - Y_i): tangents, open under any box)
            dX, dC = PairListPull.apply(H, V, Y, plist, need[2], need[3], _pull_dtype(ct, X, C, need[2], need[3]))
        return _as(dV, V.dtype), _as(dY, Y.dtype), _as(dX, X.dtype), _as(dC, C.dtype), None, None, None


# ------------------------------------------------------------------ Gaussian radial basis (K10)
def _basis_form(spec: "K.BasisSpec", collapse: bool) -> int:
    return K.GB_H_SLOT if collapse else (K.GB_H_ROW if spec.slot is not None else K.GB_H_ELEM)


class Basis(torch.autograd.Function):
    """out[e, col0(e) + k] = S[e] g_k^(q)(D[e]) on K10a (``aggf_gbasis_expand``), D.shape + (row,); ``collapse``:
    summed over the elements of each slot on K10c (``aggf_gbasis_sum``), (n_slots, n_basis).  ``S`` None: 1.  ``spec``:
    a ``_kernels.BasisSpec`` in the dtype and on the device of D (centres, width, clip, slots: constants)."""

    @staticmethod
    def forward(ctx, S, D, q, spec, collapse=False):
        d = D.contiguous()
        s = None if S is None else _widened(S, D.dtype)
        ctx.q, ctx.spec, ctx.collapse = int(q), spec, bool(collapse)
        ctx.save_for_backward(S, D)
        return K.gbasis_sum(d, spec, q, s) if collapse else K.gbasis_expand(d, spec, q, s)

    @staticmethod
    def backward(ctx, H):
        S, D = ctx.saved_tensors
        dS = dD = None
        if S is not None and ctx.needs_input_grad[0]:
            dS = _as(BasisDot.apply(H, D, ctx.q, ctx.spec, ctx.collapse), S.dtype)
        if ctx.needs_input_grad[1]:
            dD = BasisDot.apply(H, D, ctx.q + 1, ctx.spec, ctx.collapse)
            if S is not None:
                dD = S * dD
            dD = _as(dD, D.dtype)
        return dS, dD, None, None, None


class BasisDot(torch.autograd.Function):
    """out[e] = sum_k H[., k] g_k^(q)(D[e]) on K10b (``aggf_gbasis_contract``), D.shape; H in the layout of the
    ``Basis`` output of the same ``spec`` / ``collapse``: per element, per slotted row, or the (n_slots, n_basis) table."""

    @staticmethod
    def forward(ctx, H, D, q, spec, collapse=False):
        ctx.q, ctx.spec, ctx.collapse = int(q), spec, bool(collapse)
        ctx.save_for_backward(H, D)
        return K.gbasis_contract(_widened(H, D.dtype), D.contiguous(), spec, q, _basis_form(spec, collapse))

    @staticmethod
    def backward(ctx, G):
        H, D = ctx.saved_tensors
        dH = dD = None
        if ctx.needs_input_grad[0]:
            dH = _as(Basis.apply(G, D, ctx.q, ctx.spec, ctx.collapse), H.dtype)
        if ctx.needs_input_grad[1]:
            dD = _as(G * BasisDot.apply(H, D, ctx.q + 1, ctx.spec, ctx.collapse), D.dtype)
        return dH, dD, None, None, None


class MakeWhole(torch.autograd.Function):
    """X (T, N, 3) with the molecules of ``tree`` (a ``pbc.MoleculeTree``, or its ``_kernels.TreeTables``) made whole
    under ``box`` ((3,) or (T, 3) tensor on X's device, a constant) on K11 (``aggf_make_whole``), in X's dtype.  Every
    atom moves by a whole number of box lengths, a piecewise constant function of X: the backward is the identity.
    ``form``: ``_kernels.WHOLE_*`` (tests); ``images``: a (T, N, 3) int32 tensor that receives the image counts."""

    @staticmethod
    def forward(ctx, X, box, tree, form=K.WHOLE_AUTO, images=None):
        tab = tree.on(X.device) if hasattr(tree, "on") else tree
        return K.make_whole(X.contiguous(), _box_kw(box, X.dtype)["box"], tab, images=images, _form=form)

    @staticmethod
    def backward(ctx, H):
        return H, None, None, None, None
