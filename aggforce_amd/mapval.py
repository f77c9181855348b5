r"""Map validation: MSCG projections and residual shifts on random force fields (reference jaxmapval.py).

A fitted force map is checked by projecting its mapped forces on random basis force fields (``random_force_proj``)
and by the change of the force residual when such a field is subtracted (``random_residual_shift``).  The default
basis, ``rsqpg_forces``, is the force of one Gaussian of the squared pair distance with a random offset; the
reference materialises that ``(T, n, 3)`` force array once per sample.  Here the default method takes a fused path:
all ``n_samples`` offsets are drawn at once with ``randg.random(n_samples)`` (the same stream, and the same generator
state afterwards, as one ``randg.random()`` per sample) and ONE kernel pass over the frames reduces every sample
(``aggf_gauss_proj`` / ``aggf_gauss_shift``, K7).  Any other ``method`` is called once per sample, as in the
reference, and reduced on the device (``aggf_dot``).

Periodic boundaries (not in the reference): ``random_force_proj(..., box=B)`` and ``random_residual_shift(..., box=B)``
with the default method measure every pair displacement as its image under ``B`` -- the lengths of an orthorhombic box,
``(3,)`` or ``(n_frames, 3)``, or a ``pbc.Cell`` -- on the periodic forms of the same kernels, still in one pass and
with the offsets and the generator state of the open call.  The field of an open distance on a wrapped trajectory jumps
whenever a site crosses a face of the cell: it is not a function of the periodic configuration, and a projection on it
says nothing about the map.  The single-field forms that take a box are ``pbc.sq_gaussian_energies``,
``pbc.sq_gaussian_forces`` and ``pbc.rsqpg_forces`` (the names of this module keep the reference's signatures).
``outer`` must not exceed half the smallest box length (``Cell.safe_radius`` for a cell, ``Cell.image_radius`` for a cell
with ``images="nearest"``, whose displacements are the nearest of 27 images: ``pbc``): beyond it the image switches
where the field is not small and the field is discontinuous.  That is checked for a box on the host (``ValueError``,
before any device work) and not for a box on a GPU (no synchronisation).  The Gaussian's tail past ``outer`` is the
caller's concern: choose ``width`` so that it has decayed at the switching distance.

Deviations from the reference: coordinates and forces must both have the shape ``(n_frames, n_sites, 3)`` and
``width`` must be positive (``ValueError``; the reference returns NaN / inf there); the residual shift is evaluated
as ``(sum |G|^2 - 2 sum F . G) / F.size``, which equals the reference's ``force_smoothness(F - G) -
force_smoothness(F)`` without its cancellation.  Results are Python floats (the reference returns JAX scalars for
its default method); arrays come back in the container and dtype of ``positions``.
"""
from typing import Callable, Iterable, List, Union

import numpy as np
import numpy.random as r

from . import _kernels as K
from ._cell import is_cell_rows, is_nearest
from .jaxutil import _as_box

_FAST_KWARGS = frozenset({"inner", "outer", "width", "sq_args", "box"})


def _shape_of(x) -> tuple:
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _check_trajectory(x, name: str) -> tuple:
    shape = _shape_of(x)
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"{name} must have shape (n_frames, n_sites, 3), got {shape}")
    return shape


def _check_pair(coords, forces) -> None:
    cs = _check_trajectory(coords, "coords")
    fs = _check_trajectory(forces, "forces")
    if cs != fs:
        raise ValueError(f"coords {cs} and forces {fs} must have the same shape")


def _check_width(width) -> None:
    if not float(width) > 0.0:
        raise ValueError(f"width must be positive, got {width} (the reference returns NaN / inf here)")


def random_uniform_forces(
    positions: np.ndarray,
    scale: float = 1.0,
    randg: Union[r.Generator, None] = None,
) -> np.ndarray:
    """Forces of a random linear force field: one random direction of magnitude ``scale`` for every site of every
    frame (reference jaxmapval.py:30-76; host NumPy, three uniforms from ``randg``)."""
    if randg is None:
        randg = r.default_rng()
    shape = positions.shape
    x, y, z = 2 * randg.random(size=3) - 1
    force = np.array([x, y, z])
    force /= ((force**2).sum()) ** (0.5)
    force *= scale
    out = np.empty((shape[0], shape[1], 3), dtype=force.dtype)
    out[...] = force
    return out


def _sq_params(inner, outer, width, sq_args):
    if sq_args:
        outer = outer**2
        inner = inner**2
        width = width**2
    return inner, outer - inner, width


def rsqpg_forces(
    positions,
    inner: float,
    outer: float,
    width: float,
    randg: Union[r.Generator, None] = None,
    sq_args: bool = True,
):
    """Forces of a random squared-distance Gaussian force field (reference jaxmapval.py:79-131): the offset is one
    ``randg.random()`` scaled to ``[inner, outer)`` (all three squared first if ``sq_args``)."""
    inner, interval_width, width = _sq_params(inner, outer, width, sq_args)
    if randg is None:
        randg = r.default_rng()
    offset = randg.random() * interval_width + inner
    return sq_gaussian_forces(positions, offset, width)


def _draw_offsets(randg: r.Generator, n_samples: int, inner, outer, width, sq_args=True):
    """The fused path's offsets: ``randg.random(n_samples)`` equals n_samples scalar draws (values and final state)."""
    inner, interval_width, width = _sq_params(inner, outer, width, sq_args)
    _check_width(width)
    return randg.random(n_samples) * interval_width + inner, width


def _host_box(box, n_frames: int, outer=None, sq_args: bool = True):
    """``box`` normalised (``jaxutil._as_box``: (3,), (n_frames, 3) or the (n_frames, 9) rows of a ``Cell``), or None.
    On the host, ``outer`` (if given) as a distance (its square root if it was given squared) must not exceed half the
    smallest length, ``Cell.safe_radius`` for a cell, ``Cell.image_radius`` for a cell with ``images="nearest"``
    (``ValueError``); a box on a GPU is not read."""
    if box is None:
        return None
    given = box
    box = _as_box(box, n_frames)
    if outer is not None and not box.is_cuda and box.numel():
        reach = float(outer) if sq_args else float(outer) ** 0.5
        if is_nearest(given):
            if reach > given.image_radius:
                raise ValueError(f"outer reaches {reach:g}, beyond the cell's image radius, half its shortest lattice "
                                 f"vector ({given.image_radius:g}): the field is discontinuous where the image switches")
            return box
        lengths = box[:, [0, 4, 8]] if is_cell_rows(box) else box
        half = float(lengths.min()) / 2
        if reach > half:
            raise ValueError(f"outer reaches {reach:g}, beyond half the smallest box length ({half:g}): the field is "
                             "discontinuous where the image switches")
    return box


def _device_box(box, X):
    return None if box is None else box.to(device=X.device, dtype=X.dtype).contiguous()


def _fast_path(method, kwargs) -> bool:
    if not set(kwargs) <= _FAST_KWARGS:
        return False
    if method is rsqpg_forces:
        return True
    from . import pbc

    return method is pbc.rsqpg_forces


def _fused(coords, forces, n_samples: int, randg, kwargs, shift: bool) -> List[float]:
    import torch

    kwargs = dict(kwargs)
    box = kwargs.pop("box", None)
    near = is_nearest(box)
    if box is not None:
        box = _host_box(box, _shape_of(coords)[0], kwargs.get("outer"), kwargs.get("sq_args", True))
    offsets, width = _draw_offsets(randg, n_samples, **kwargs)
    X = K.as_device(coords)
    F = K.as_device(forces)
    o = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.float64)).to(X.device)
    under = {} if box is None else {"box": _device_box(box, X)}
    if near:
        under["near"] = True
    if shift:
        ip, gsq = (v.cpu().numpy() for v in K.gauss_shift(X, F, o, width, **under))
        vals = (gsq - 2.0 * ip) / float(F.numel())
    else:
        vals = K.gauss_proj(X, F, o, width, **under).cpu().numpy() / float(X.shape[0])
    return [float(v) for v in vals]


def random_residual_shift(
    coords: np.ndarray,
    forces: np.ndarray,
    n_samples: int = 1000,
    randg: Union[r.Generator, None] = None,
    method: Callable = rsqpg_forces,
    average: bool = False,
    **kwargs,
) -> Union[float, List[float]]:
    """Force-residual shift of ``n_samples`` random force fields G_s against the flat one (reference
    jaxmapval.py:159-237): ``force_smoothness(forces - G_s) - force_smoothness(forces)`` per sample, or their mean
    if ``average``.  ``method(coords, randg=randg, **kwargs)`` makes G_s; the default takes the fused path, also with
    ``box=`` among the keywords (pair displacements as their images under a periodic box or ``pbc.Cell``: the module's
    text).  Any other method is handed ``box`` like every other keyword."""
    _check_pair(coords, forces)
    if randg is None:
        randg = r.default_rng()
    if n_samples <= 0:
        vals = []
    elif _fast_path(method, kwargs):
        vals = _fused(coords, forces, n_samples, randg, kwargs, shift=True)
    else:
        vals = []
        F = K.as_device(forces)
        for _ in range(n_samples):
            G = _trial(method(coords, randg=randg, **kwargs), F)
            vals.append((K.dot(G, G).item() - 2.0 * K.dot(F, G).item()) / F.numel())
    if average:
        return sum(vals) / n_samples
    return vals


def random_force_proj(
    coords: np.ndarray,
    forces: np.ndarray,
    n_samples: int = 1000,
    randg: Union[r.Generator, None] = None,
    method: Callable = rsqpg_forces,
    average: bool = True,
    **kwargs,
) -> Union[float, Iterable[float]]:
    """MSCG projections of ``forces`` on ``n_samples`` random basis force fields (reference jaxmapval.py:266-319):
    ``mscg_ip(forces, method(coords, randg=randg, **kwargs))`` per sample, or their mean if ``average``.  The
    default method takes the fused path, also with ``box=`` among the keywords (pair displacements as their images
    under a periodic box or ``pbc.Cell``: the module's text).  Any other method is handed ``box`` like every other
    keyword."""
    _check_pair(coords, forces)
    if randg is None:
        randg = r.default_rng()
    if n_samples <= 0:
        vals = []
    elif _fast_path(method, kwargs):
        vals = _fused(coords, forces, n_samples, randg, kwargs, shift=False)
    else:
        vals = []
        F = K.as_device(forces)
        for _ in range(n_samples):
            G = _trial(method(coords, randg=randg, **kwargs), F)
            vals.append(K.dot(F, G).item() / F.shape[0])
    if average:
        return sum(vals) / n_samples
    return vals


def _trial(funcs, F):
    G = K.as_device(funcs)
    if tuple(G.shape) != tuple(F.shape):
        raise ValueError(f"the force field has shape {tuple(G.shape)}, the forces {tuple(F.shape)}")
    return G


def mscg_ip(forces, funcs) -> float:
    """MSCG inner product (reference jaxmapval.py:322-360): ``sum(funcs * forces) / n_steps`` as a float, summed on
    the device in a fixed order.  ``funcs`` is an array of force-field values of the shape of ``forces``."""
    F = K.as_device(forces)
    G = _trial(funcs, F)
    return float(K.dot(F, G).item()) / F.shape[0]


def _positions(positions, width):
    _check_trajectory(positions, "positions")
    _check_width(width)
    return K.as_device(positions)


def sq_gaussian_energies(positions, offset: float, width: float):
    """Per-frame energy ``sum_{i,j} exp(-((|r_i - r_j|^2 - offset) / width)^2)`` over the full site matrix, diagonal
    included (reference jaxmapval.py:365-392); shape (n_frames,), in the container and dtype of ``positions``."""
    X = _positions(positions, width)
    _, E = K.gauss_pair_forces(X, offset, width, want_forces=False, want_energies=True)
    return K.like_input(E, positions)


def sq_gaussian_forces(positions, offset: float, width: float):
    """Forces ``-d sum_t E_t / d positions`` of ``sq_gaussian_energies`` (reference jaxmapval.py:396-401), in closed
    form: ``G_i = (8 / width^2) sum_j (x_ij - offset) g(x_ij) (r_i - r_j)``; in the container and dtype of
    ``positions``."""
    X = _positions(positions, width)
    G, _ = K.gauss_pair_forces(X, offset, width)
    return K.like_input(G, positions)


__all__ = [
    "random_uniform_forces",
    "rsqpg_forces",
    "random_residual_shift",
    "random_force_proj",
    "mscg_ip",
    "sq_gaussian_energies",
    "sq_gaussian_forces",
]
