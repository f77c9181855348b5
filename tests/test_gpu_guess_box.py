"""K6 under a periodic box (aggf_pair_dist_var_pbc / aggf_pair_dist_moments_pbc) and the ``box=`` keyword it carries up
to guess_pairwise_constraints, project_forces and project_forces_grid_cv, against the float64 NumPy restatement of
tests/guess_box_data.py (np.var / np.mean over frames of sqrt(sum(wrap(d, L)**2)), on the inputs as stored).

The bound on variances and means is K6's own from tests/test_gpu_parity.py: max |got - ref| < 1e-10 max(1, ref.max()).
No element is masked: guess_box_data.wrapped asserts that no displacement component lies within 1e-9 of a half-box tie
(the device rounds d * (1 / L), the reference d / L; they differ by about 1e-15)."""
import numpy as np
import pytest
import torch

import guess_box_data as D
import pbc_ref as P
from aggforce_amd import LinearMap, guess_pairwise_constraints, project_forces
from aggforce_amd import _kernels as K
from aggforce_amd.agg import project_forces_grid_cv

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
SITES = [0, 5, 129, 12, 25, 38, 51, 64, 77, 90]  # a slice map of 10 sites, three of them in rigid pairs


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def close(got, ref, what):
    err, bound = float(np.max(np.abs(got - ref))), 1e-10 * max(1.0, float(ref.max()))
    print(f"{what}: max |got - ref| = {err:.3e}, bound {bound:.3e}")
    assert err < bound, f"{what}: {err:.3e} >= {bound:.3e}"


def symmetric_zero_diagonal(a):
    return np.array_equal(a, a.T) and not np.diagonal(a).any()


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_box", "box_per_frame"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_variance_matches_the_minimum_image_reference(dtype, per_frame):
    x, L = D.wrapped(per_frame, dtype)
    var = K.pair_dist_var(dev(x), box=dev(L)).cpu().numpy()
    close(var, D.ref_moments(per_frame, dtype)[1], f"var {dtype}")
    assert symmetric_zero_diagonal(var)


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_box", "box_per_frame"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_moments_match_the_reference(dtype, per_frame):
    x, L = D.wrapped(per_frame, dtype)
    mean, var = (a.cpu().numpy() for a in K.pair_dist_moments(dev(x), box=dev(L)))
    ref_mean, ref_var = D.ref_moments(per_frame, dtype)
    close(mean, ref_mean, f"mean {dtype}")
    close(var, ref_var, f"var {dtype}")
    assert symmetric_zero_diagonal(var) and symmetric_zero_diagonal(mean)


@pytest.mark.parametrize("dtype", DTYPES)
def test_shard_moments_pool_to_the_whole_trajectory(dtype):
    """Two shards of 23 and 18 frames, each under its own rows of the per-frame box, pooled as the guesser pools the
    ranks' moments (the sum over shards stands for the all-reduce)."""
    x, L = D.wrapped(True, dtype)
    shards = [(x[:23], L[:23]), (x[23:], L[23:])]
    moments = [K.pair_dist_moments(dev(xs), box=dev(Ls)) for xs, Ls in shards]
    weights = [xs.shape[0] / D.T for xs, _ in shards]
    mean = sum(K.axpby(w, m, 0.0, m) for w, (m, _) in zip(weights, moments))
    var = sum(K.pair_pool_term(v, m, mean, w) for w, (m, v) in zip(weights, moments))
    ref_mean, ref_var = D.ref_moments(True, dtype)
    close(mean.cpu().numpy(), ref_mean, f"pooled mean {dtype}")
    close(var.cpu().numpy(), ref_var, f"pooled var {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_huge_box_gives_the_open_bits(dtype):
    """k = rint(d / L) = 0 and fma(-0, L, d) = d: the box form under a box of 1e6 per side is the open form bit for bit."""
    x = dev(D.wrapped(False, dtype)[0])
    box = torch.full((3,), 1e6, dtype=x.dtype, device=x.device)
    assert torch.equal(K.pair_dist_var(x, box=box), K.pair_dist_var(x))
    open_mean, open_var = K.pair_dist_moments(x)
    box_mean, box_var = K.pair_dist_moments(x, box=box.expand(D.T, 3).contiguous())
    assert torch.equal(box_mean, open_mean) and torch.equal(box_var, open_var)


@pytest.mark.parametrize("on_gpu", [False, True], ids=["numpy", "gpu_tensors"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["one_box", "box_per_frame"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_guess_finds_the_rigid_pairs_only_with_the_box(dtype, per_frame, on_gpu):
    x, L = D.wrapped(per_frame, dtype)
    assert D.ref_guess(x, L) == D.RIGID_SET and not (D.ref_guess(x, None) & D.RIGID_SET)  # (the reference agrees)
    if on_gpu:
        x, L = dev(x), dev(L)
    assert guess_pairwise_constraints(x, box=L, threshold=1e-3) == D.RIGID_SET
    assert not (guess_pairwise_constraints(x, threshold=1e-3) & D.RIGID_SET)


@pytest.mark.parametrize("per_frame", [False, True], ids=["one_box", "box_per_frame"])
def test_a_bad_box_on_the_device(per_frame):
    """A zero length in a box that lives on the GPU: the guesser raises, the kernel marks (NaN off the diagonal, 0 on
    it) -- with a box per frame the bad frame is the last one, the single frame of the last split."""
    x, L = D.wrapped(per_frame, "float64")
    bad = np.array(L)
    if per_frame:
        bad[-1, 1] = 0.0
    else:
        bad[1] = 0.0
    x, bad = dev(x), dev(bad)
    with pytest.raises(ValueError, match="box"):
        guess_pairwise_constraints(x, box=bad)
    var = K.pair_dist_var(x, box=bad).cpu().numpy()
    off = ~np.eye(D.N, dtype=bool)
    assert np.isnan(var[off]).all() and not np.diagonal(var).any()


def test_project_forces_guesses_under_the_box():
    x, L = D.wrapped(True, "float64")
    forces = 30 * np.random.default_rng(11).standard_normal(x.shape)
    cmap = LinearMap([[s] for s in SITES], n_fg_sites=D.N)
    auto = project_forces(x, forces, cmap, box=L, l2_regularization=1.0)
    assert auto["constraints"] == D.RIGID_SET
    explicit = project_forces(x, forces, cmap, constrained_inds=set(D.RIGID_SET), l2_regularization=1.0)
    assert np.array_equal(auto["tmap"].force_map.standard_matrix, explicit["tmap"].force_map.standard_matrix)
    assert np.array_equal(auto["mapped_forces"], explicit["mapped_forces"])
    assert np.array_equal(auto["mapped_coords"], x[:, SITES])  # (the coordinates as given: the box does not touch them)
    no_box = project_forces(x, forces, cmap, l2_regularization=1.0)
    assert no_box["constraints"] != auto["constraints"] and not (no_box["constraints"] & D.RIGID_SET)
    # the same on GPU tensors, box included
    on_gpu = project_forces(dev(x), dev(forces), cmap, box=dev(L), l2_regularization=1.0)
    assert on_gpu["constraints"] == D.RIGID_SET
    assert torch.equal(on_gpu["mapped_forces"].cpu(), torch.as_tensor(explicit["mapped_forces"]))


def test_grid_cv_hands_each_training_subset_its_box():
    x, L = D.wrapped(True, "float64")
    x_open = D.open_coords()
    forces = 30 * np.random.default_rng(12).standard_normal(x.shape)
    cmap = LinearMap([[s] for s in SITES], n_fg_sites=D.N)
    # the folds project_forces_grid_cv will draw: both inputs give the same guess on every training subset
    frames = np.arange(D.T)
    np.random.default_rng(0).shuffle(frames)
    folds = np.array_split(frames, 2)
    for k in range(2):
        train = np.concatenate([f for j, f in enumerate(folds) if j != k])
        assert D.ref_guess(x[train], L[train]) == D.ref_guess(x_open[train], None) == D.RIGID_SET
    grid = {"l2_regularization": [1.0, 1e3]}
    boxed = project_forces_grid_cv(grid, x, forces, n_folds=2, rng=np.random.default_rng(0), coord_map=cmap, box=L)
    plain = project_forces_grid_cv(grid, x_open, forces, n_folds=2, rng=np.random.default_rng(0), coord_map=cmap)
    assert set(boxed["scores"]) == set(plain["scores"]) and len(boxed["scores"]) == 2
    for key, want in plain["scores"].items():
        got = boxed["scores"][key]
        print(f"{key}: {got!r} with the box, {want!r} open")
        assert boxed["n_runs"][key] == plain["n_runs"][key] == 2
        assert abs(got - want) <= 1e-10 * abs(want)
