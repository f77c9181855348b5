"""jaxify_linearmap (reference: map/jaxtools.py): a LinearMap as a differentiable callable on torch tensors."""
from typing import Callable

from ..jaxutil import trjdot
from .core import LinearMap


def jaxify_linearmap(
    lm: LinearMap,
    flattened: bool = True,
    n_dim: float = 3,
) -> Callable:
    """Callable ``wrapped(mat, perframe=False)`` applying ``lm``'s matrix through ``jaxutil.trjdot``.

    ``flattened``: ``mat`` is (n_frames, n_fg_sites * n_dim) and so is the result's layout (n_cg_sites * n_dim);
    otherwise (n_frames, n_fg_sites, n_dim).  ``perframe=True``: ``mat`` lacks the leading frame axis (one frame).
    The matrix is a constant (no gradient); the result is differentiable in ``mat``."""
    import torch

    matrix = lm.standard_matrix
    on_device: dict = {}

    def wrapped(mat, perframe: bool = False):
        factor = matrix
        if isinstance(mat, torch.Tensor) and mat.is_cuda:
            key = str(mat.device)
            if key not in on_device:
                on_device[key] = torch.as_tensor(matrix).to(mat.device)
            factor = on_device[key]
        if perframe:
            mat = mat[None, ...]
        if flattened:
            mat = mat.reshape((mat.shape[0], mat.shape[1] // n_dim, n_dim))
        result = trjdot(points=mat, factor=factor)
        if flattened:
            result = result.reshape((result.shape[0], result.shape[1] * result.shape[2]))
        if perframe:
            result = result[0]
        return result

    return wrapped
