"""``box=`` on guess_pairwise_constraints, project_forces and project_forces_grid_cv: what holds without a GPU -- the
signatures and the two new C ABI names, the host (``cross_xyz``) form under a box, and the refusal of a bad box before
anything touches a device."""
import ctypes
import inspect

import numpy as np
import pytest

import guess_box_data as D
import pbc_ref as P
from aggforce_amd import LinearMap, _lib, guess_pairwise_constraints, project_forces
from aggforce_amd.agg import project_forces_grid_cv


@pytest.mark.parametrize("fn", [guess_pairwise_constraints, project_forces, project_forces_grid_cv])
def test_box_is_an_optional_keyword(fn):
    p = inspect.signature(fn).parameters["box"]
    assert p.default is None and p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_the_reference_order_of_the_guesser_is_kept():
    names = list(inspect.signature(guess_pairwise_constraints).parameters)
    assert names[:3] == ["xyz", "cross_xyz", "threshold"] and names.index("box") > 2


@pytest.mark.parametrize("name", ["aggf_pair_dist_var_pbc", "aggf_pair_dist_moments_pbc"])
def test_the_box_entry_points_are_bound_and_exported(name):
    assert name in _lib.PROTOTYPES
    open_args = _lib.PROTOTYPES[name.replace("_pbc", "")][1]
    assert len(_lib.PROTOTYPES[name][1]) == len(open_args) + 2  # (box, box_stride)
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), name) is not None


@pytest.mark.parametrize("per_frame", [False, True])
def test_cross_form_finds_a_rigid_pair_across_a_face(per_frame):
    T = 30
    rng = np.random.default_rng(7)
    L = P.frame_boxes(T, 8) if per_frame else P.BOX
    xyz = P.BOX * rng.random((1, 4, 3)) + 0.3 * rng.standard_normal((T, 4, 3))
    cross = P.BOX * rng.random((1, 3, 3)) + 0.3 * rng.standard_normal((T, 3, 3))
    xyz[:, 1] = np.array([0.05, 2.0, 3.0]) + 0.3 * rng.standard_normal((T, 3))  # jitters across the face x = 0
    cross[:, 2] = xyz[:, 1] + np.array([0.4, -0.7, 0.2])  # rigid: site 2 of cross_xyz, site 1 of xyz
    xyz_w, cross_w = D.wrap_into_cell(xyz, L), D.wrap_into_cell(cross, L)
    d = xyz_w[:, 1] - cross_w[:, 2]
    split = (np.abs(d) > 0.5 * (L if per_frame else L[None])).any(axis=1)
    assert split.any() and not split.all()
    assert guess_pairwise_constraints(xyz_w, cross_xyz=cross_w, box=L) == {(2, 1)}
    assert guess_pairwise_constraints(xyz_w, cross_xyz=cross_w) == set()
    assert guess_pairwise_constraints(xyz, cross_xyz=cross) == {(2, 1)}  # (open data: found with or without a box)
    assert guess_pairwise_constraints(xyz_w, cross_xyz=cross_w, box=L.tolist()) == {(2, 1)}  # (a sequence)


def _bad_boxes():
    T = D.T
    yield "shape (2,)", np.array([4.0, 5.0])
    yield "one frame too many", np.tile(P.BOX, (T + 1, 1))
    yield "zero length", np.array([4.1, 0.0, 6.7])
    yield "negative length", [4.1, -5.3, 6.7]
    nan = np.tile(P.BOX, (T, 1))
    nan[T // 2, 1] = np.nan
    yield "NaN length", nan


@pytest.mark.parametrize("what,box", list(_bad_boxes()), ids=[w for w, _ in _bad_boxes()])
def test_a_bad_box_is_refused_without_a_gpu(what, box):
    x, _ = D.wrapped(False, "float64")
    forces = np.zeros_like(x)
    cmap = LinearMap([[i] for i in range(10)], n_fg_sites=D.N)
    with pytest.raises(ValueError, match="box"):
        guess_pairwise_constraints(x, box=box)
    with pytest.raises(ValueError, match="box"):
        guess_pairwise_constraints(x, cross_xyz=x[:, :2], box=box)
    with pytest.raises(ValueError, match="box"):
        project_forces(x, forces, cmap, box=box)
    with pytest.raises(ValueError, match="box"):  # (ignored with explicit constraints, but still validated)
        project_forces(x, forces, cmap, constrained_inds=set(), box=box)
    with pytest.raises(ValueError, match="box"):
        project_forces_grid_cv({"l2_regularization": [1.0]}, x, forces, n_folds=2, coord_map=cmap, box=box)
