"""Module path of the reference's map validation (jaxmapval.py): the HIP one (``mapval``)."""
from .mapval import (
    mscg_ip,
    random_force_proj,
    random_residual_shift,
    random_uniform_forces,
    rsqpg_forces,
    sq_gaussian_energies,
    sq_gaussian_forces,
)

__all__ = [
    "random_uniform_forces",
    "rsqpg_forces",
    "random_residual_shift",
    "random_force_proj",
    "mscg_ip",
    "sq_gaussian_energies",
    "sq_gaussian_forces",
]
