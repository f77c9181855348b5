"""Inputs and float64 references shared by tests/test_guess_box_host.py and tests/test_gpu_guess_box.py: a trajectory
wrapped into an orthorhombic periodic cell with three exactly rigid pairs that the wrap splits across a face in some
frames, and the NumPy restatement of K6 under a box (np.var / np.mean over frames of the minimum-image distances,
``pbc_ref.wrap``), evaluated on the inputs as stored."""
import functools

import numpy as np

import pbc_ref as P

T, N = 41, 131  # three 64-pair tile rows (the last ragged), six frame splits of 8 frames and one of a single frame
SEED = 4  # fixed so that both conditions asserted in wrapped() hold (checked on the CPU)
RIGID = ((0, 1), (5, 70), (129, 130))
RIGID_SET = {frozenset(p) for p in RIGID}


def wrap_into_cell(x, L):
    """Every frame of x (T, N, 3) wrapped into its cell: x - L floor(x / L), in float64."""
    L = P.over(L, x)
    return x - L * np.floor(x / L)


@functools.lru_cache(maxsize=None)
def open_coords():
    """(T, N, 3) float64 open coordinates: sites jittering around random positions, three exactly rigid pairs."""
    rng = np.random.default_rng(SEED)
    x = P.BOX * rng.random((1, N, 3)) + 0.3 * rng.standard_normal((T, N, 3))
    for i, j in RIGID:
        x[:, j] = x[:, i] + rng.uniform(-1, 1, 3)  # well inside half the smallest box length
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def boxes(per_frame):
    L = P.frame_boxes(T, SEED + 1) if per_frame else P.BOX.copy()
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def wrapped(per_frame, dtype_name):
    """(x, L) as stored: the open coordinates wrapped into the cell in float64, then cast to ``dtype_name``; the box
    cast the same way.  The two conditions the tests rely on are asserted here, on the CPU, in float64."""
    L = boxes(per_frame)
    x = wrap_into_cell(open_coords(), L).astype(dtype_name)
    Ls = L.astype(dtype_name)
    xs, Lw = x.astype(np.float64), Ls.astype(np.float64)
    for i, j in RIGID:
        d = xs[:, j] - xs[:, i]
        split = (np.abs(d) > 0.5 * (Lw if Lw.ndim == 2 else Lw[None])).any(axis=1)
        assert split.any() and not split.all(), f"rigid pair {(i, j)} is split in {int(split.sum())} of {T} frames"
    disp = xs[:, None, :, :] - xs[:, :, None, :]
    assert P.tie_distance(disp, Lw) > 1e-9, "a displacement component sits at a half-box tie"
    x.setflags(write=False)
    Ls.setflags(write=False)
    return x, Ls


def ref_distances(x, L):
    """(T, N, N) float64 minimum-image distances of the inputs as stored (L None: open distances)."""
    xs = np.asarray(x, dtype=np.float64)
    disp = xs[:, None, :, :] - xs[:, :, None, :]
    if L is not None:
        disp = P.wrap(disp, np.asarray(L, dtype=np.float64))
    return np.sqrt(np.sum(disp * disp, axis=-1))


@functools.lru_cache(maxsize=None)
def ref_moments(per_frame, dtype_name):
    """(mean, var) (N, N) float64 over the frames of the wrapped trajectory under its box."""
    x, L = wrapped(per_frame, dtype_name)
    d = ref_distances(x, L)
    return d.mean(axis=0), d.var(axis=0)


def ref_guess(x, L, threshold=1e-3):
    """The guess from the reference distances: pairs i < j with np.std < threshold."""
    sd = ref_distances(x, L).std(axis=0)
    i, j = np.nonzero(np.triu(sd < threshold, k=1))
    return {frozenset((int(a), int(b))) for a, b in zip(i, j)}
