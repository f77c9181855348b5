"""JLinearMap: a LinearMap whose application is differentiable (reference: map/jaxlinearmap.py).

The reference maps JAX arrays; here the differentiable array is the torch tensor.  A tensor in gives a tensor out on the
same device, differentiable in ``points`` through the autograd Functions of ``_autograd`` (K3 forward, K3 on the cached
transpose and K8a backward); a NumPy array in gives a NumPy array out.  The NaN policy is the reference's own
(jaxlinearmap.py:15-39,104-116), not LinearMap's: the result is the product with NaN read as 0; unless
``bypass_nan_check`` is set, a ValueError is raised when it differs from the NaN -> 1 product; the gradient at a NaN
input is 0 (as through ``jnp.nan_to_num``).  Those extra products are formed only when the NaN probe fused into K3
fires.
"""
import numpy as np

from .. import _kernels as K
from .core import LinearMap

_NAN_MSG = (
    "NaN handling is on and multiplication tried to use "
    "a NaN value. Check the input array and "
    "standard_matrix."
)


class JLinearMap(LinearMap):
    """Extends LinearMap to differentiable (torch) application."""

    def __init__(self, *args, bypass_nan_check: bool = False, **kwargs) -> None:
        """As LinearMap; ``bypass_nan_check``: skip the NaN -> 1 comparison of the reference's NaN policy."""
        super().__init__(*args, **kwargs)
        self.bypass_nan_check = bypass_nan_check

    def _matrix_dtype(self):
        dt = self._standard_matrix.dtype
        return K.torch_dtype(dt if dt in (np.float32, np.float64) else np.float64)

    @property
    def jax_standard_matrix(self):
        """standard_matrix as a (cached, constant) device tensor."""
        return self._device_matrix(self._matrix_dtype(), K.default_device())

    def _device_matrix_t(self, tdtype, device):
        """Contiguous transpose of the device matrix (the backward's K3 operand), cached beside it."""
        m = self._device_matrix(tdtype, device)
        key = ("T", tdtype, str(device))
        hit = self._dev_cache.get(key)
        if hit is None or hit[0] is not self._standard_matrix:
            hit = (self._standard_matrix, m.t().contiguous())
            self._dev_cache[key] = hit
        return hit[1]

    def __call__(self, points):
        """Map (n_steps, n_fg_sites, 3) points; the container type (and device) of ``points`` is kept."""
        shape = tuple(points.shape)
        if len(shape) != 3 or shape[2] != self.n_dim or shape[1] != self.n_fg_sites:
            raise ValueError(
                f"points of shape {shape} cannot be mapped by a ({self.n_cg_sites},{self.n_fg_sites}) JLinearMap"
            )
        import torch

        from .._autograd import Apply

        out_t = K.torch_dtype(self._out_dtype(points))
        p = K.as_device(points)
        m = self._device_matrix(out_t, p.device)
        mt = self._device_matrix_t(out_t, p.device)
        if not self.handle_nans:
            return K.like_input(Apply.apply(p, m, mt), points)
        probe = K.take_flag(p.device)
        out = Apply.apply(p, m, mt, probe)
        # (the probe is conservative -- an infinity meeting a zero coefficient sets it too -- so it is confirmed on
        # the input before the reference's two products are formed)
        if K.read_flag(probe) and K.has_nan(p.detach()):
            p0 = torch.where(torch.isnan(p), torch.zeros((), dtype=p.dtype, device=p.device), p)
            out = Apply.apply(p0, m, mt)
            if not self.bypass_nan_check:
                pushed = K.linearmap_apply(p.detach(), m, nan_fill=1.0)
                if not K.allclose(out.detach(), pushed, rtol=1e-5, atol=self.nan_check_threshold):
                    raise ValueError(_NAN_MSG)
        return K.like_input(out, points)

    def flat_call(self, flattened):
        """Apply to (n_frames, n_fg_sites*3) and return (n_frames, n_cg_sites*3)."""
        shape = tuple(flattened.shape)
        if len(shape) == 3:
            raise ValueError(f"Expected array of rank 2; got array with shape {shape}.")
        if flattened.shape[1] % self.n_dim != 0:
            raise ValueError(f"Array of shape {shape} can't be reshaped with dim of f{self.n_dim}.")
        reshaped = flattened.reshape((flattened.shape[0], flattened.shape[1] // self.n_dim, self.n_dim))
        transformed = self(reshaped)
        return transformed.reshape((transformed.shape[0], transformed.shape[1] * transformed.shape[2]))

    # ------------------------------------------------------------------ algebra (T, @, __rmul__, __add__, astype)
    def _derive(self, matrix: np.ndarray) -> "JLinearMap":
        return JLinearMap(
            mapping=matrix,
            bypass_nan_check=self.bypass_nan_check,
            handle_nans=self.handle_nans,
            nan_check_threshold=self.nan_check_threshold,
        )

    @classmethod
    def from_linearmap(cls, lm: LinearMap, /, bypass_nan_check: bool = False) -> "JLinearMap":
        """JLinearMap with the matrix and NaN handling of a LinearMap."""
        return JLinearMap(mapping=lm.standard_matrix, bypass_nan_check=bypass_nan_check, handle_nans=lm.handle_nans)

    def to_linearmap(self) -> LinearMap:
        """Plain LinearMap with this map's matrix and NaN handling."""
        return LinearMap(mapping=self.standard_matrix, handle_nans=self.handle_nans)
