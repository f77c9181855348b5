"""Helpers shared by tests/test_pbc_host.py and tests/test_gpu_pbc.py: float64 restatements, in NumPy and torch, of the
minimum-image convention under an orthorhombic box (d - L rint(d / L) per component, rint to nearest even), the
per-component magnitude b = |d| + |rint(d / L)| L that the error bounds of the box kernels are stated in, the mask of
elements near a tie, and stand-ins in torch for the three ``_kernels`` functions that take a ``box``.

Near a tie -- a component with d / L within ``margin`` of a half-integer -- both images are legitimate answers: the
device rounds d * (1 / L) in the operands' precision, the reference d / L in float64, and they may land on different
sides.  MARGIN is the size of that rounding at the largest |d| / L the test inputs span (three box lengths: 3 x 2^-24
x 2 roundings = 4e-7 in float32, 7e-16 in float64), with room.  Such elements are left out of value comparisons and
carry zero weight in the pull tests; no case may mask more than MAX_MASKED of its elements."""
import numpy as np
import torch

import aggforce_amd._kernels as K

BOX = np.array([4.1, 5.3, 6.7])
MARGIN = {torch.float32: 1e-5, torch.float64: 1e-11}
MAX_MASKED = 1e-3


def frame_boxes(T, seed, spread=0.03):
    """A (T, 3) box that varies by a few percent from frame to frame."""
    return BOX * (1 + spread * np.random.default_rng(seed).uniform(-1, 1, (T, 3)))


def over(L, d):
    """``L`` ((3,) or (T, 3)) shaped to broadcast against displacements ``d`` (T, ..., 3)."""
    L = np.asarray(L, dtype=np.float64)
    return L if L.ndim == 1 else L.reshape((L.shape[0],) + (1,) * (d.ndim - 2) + (3,))


# ------------------------------------------------------------------ float64 NumPy references (inputs as stored)
def wrap(d, L):
    """The minimum image of displacements d (T, ..., 3) under L ((3,) or (T, 3))."""
    L = over(L, d)
    return d - L * np.rint(d / L)


def comp_bound(d, L):
    """b = |d| + |rint(d / L)| L per component: the magnitudes the wrapped component is formed from."""
    L = over(L, d)
    return np.abs(d) + np.abs(np.rint(d / L)) * L


def tie_mask(d, L, margin):
    """Elements (T, ...) with a component whose d / L lies within ``margin`` of a half-integer."""
    q = d / over(L, d)
    return (np.abs(q - np.floor(q) - 0.5) < margin).any(axis=-1)


def tie_distance(d, L):
    """The smallest |frac(d / L) - 1/2| over all components."""
    q = d / over(L, d)
    return float(np.min(np.abs(q - np.floor(q) - 0.5)))


# ------------------------------------------------------------------ the same in torch, and the kernels' stand-ins
def torch_wrap(d, box):
    if box is None:
        return d
    L = box.to(d.dtype)
    if L.dim() == 2:
        L = L.reshape((L.shape[0],) + (1,) * (d.dim() - 2) + (3,))
    return d - L * torch.round(d / L)


def _check_box(box, x):
    assert box is None or (box.dtype == x.dtype and tuple(box.shape) in ((3,), (x.shape[0], 3)) and box.is_contiguous())


def fake_pair_list_dist(x, c, tab, mode=K.PAIR_DIST, v=None, y=None, box=None):
    assert x.dtype == c.dtype and x.is_contiguous() and c.is_contiguous()
    _check_box(box, x)
    i, j = tab.pairs[:, 0].long(), tab.pairs[:, 1].long()
    u = torch_wrap(x[:, j] - c[:, i], box)
    if mode == K.PAIR_DOT:
        assert v.dtype == x.dtype == y.dtype
        return ((v[:, j] - y[:, i]) * u).sum(-1)
    s = (u * u).sum(-1)
    return s if mode == K.PAIR_SQDIST else s.sqrt()


def fake_pair_list_pull(w, x, c, tab, dv=None, want_a=True, want_b=True, out_dtype=None, box=None):
    assert w.dtype == x.dtype == c.dtype and (dv is None or dv.dtype == w.dtype)
    _check_box(box, x)
    out_dtype = out_dtype or x.dtype
    assert not (x.dtype == torch.float32 and out_dtype == torch.float64)
    i, j = tab.pairs[:, 0].long(), tab.pairs[:, 1].long()
    if dv is not None:
        w = torch.where(dv > 0, w / dv, torch.zeros_like(w))
    q = w[..., None] * torch_wrap(x[:, j] - c[:, i], box)
    a = torch.zeros_like(x).index_add_(1, j, q).to(out_dtype) if want_a else None
    b = torch.zeros_like(c).index_add_(1, i, -q).to(out_dtype) if want_b else None
    return a, b


def fake_pair_min(x, c, square=False, box=None):
    assert x.dtype == c.dtype
    _check_box(box, x)
    u = torch_wrap(x[:, None, :, :] - c[:, :, None, :], box)
    s = (u * u).sum(-1).amin(0)
    return s if square else s.sqrt()
