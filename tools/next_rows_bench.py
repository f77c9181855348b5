"""GPU box: one measured number for every SURVEY 8(f) row that is built (JSON lines on stdout).

  cv      project_forces_grid_cv, 5 folds x 4 l2 values: one-pass Gram reuse vs the reference-style loop
  staged  stagedjoptgauss_map fit + application at the C5 size
  k6      guess_pairwise_constraints' pair-distance statistics kernel, and its box form against it (one box, a box
          per frame): the k6_box row, kept in profiles/k6_box_bench.jsonl
  stream  out-of-core project_forces_streamed from memory-mapped .npy files
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from aggforce_amd import LinearMap, Trajectory, stagedjoptgauss_map  # noqa: E402
from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd.agg import project_forces_grid_cv  # noqa: E402
from aggforce_amd.stream import load_trajectory, project_forces_streamed  # noqa: E402


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def emit(**kw):
    print(json.dumps(kw), flush=True)


def bench_cv():
    T, N, n_cg = 500_000, 2048, 128
    forces = K.synth_normal(T, N, torch.float32, 1, sigma=30.0)
    coords = K.synth_normal(T, N, torch.float32, 2, sigma=0.3, lattice=1.5)
    cmap = LinearMap([[i * (N // n_cg)] for i in range(n_cg)], n_fg_sites=N)
    grid = {"l2_regularization": [0.0, 1e-3, 1e-1, 10.0]}
    res, times = {}, {}
    for name, reuse in (("one_pass", True), ("loop", False)):
        times[name] = []
        for rep in range(4 if reuse else 2):
            t0 = sync()
            r = project_forces_grid_cv(grid, coords, forces, n_folds=5, rng=np.random.default_rng(0),
                                       coord_map=cmap, constrained_inds=None, reuse_gram=reuse)
            times[name].append(sync() - t0)
        res[name] = (min(times[name][1:]), r)
    a, b = res["one_pass"][1]["scores"], res["loop"][1]["scores"]
    worst = max(abs(a[k] - b[k]) / abs(b[k]) for k in a)
    # (every repetition is listed: a box has shown one-off stalls of seconds in either form; the first is the warm-up)
    emit(row="cv", workload=f"{T} x {N} x {n_cg} fp32, 5 folds x 4 l2 values", one_pass_s=res["one_pass"][0],
         loop_s=res["loop"][0], speedup=res["loop"][0] / res["one_pass"][0], max_rel_score_diff=worst,
         one_pass_reps_s=times["one_pass"], loop_reps_s=times["loop"])


def bench_cv_noised():
    from aggforce_amd import joptgauss_map

    T, N, n_cg = 500_000, 2048, 128
    forces = K.synth_normal(T, N, torch.float32, 1, sigma=30.0)
    coords = K.synth_normal(T, N, torch.float32, 2, sigma=0.3, lattice=1.5)
    cmap = LinearMap([[i * (N // n_cg)] for i in range(n_cg)], n_fg_sites=N)
    grid = {"l2_regularization": [0.0, 1e-3, 1e-1, 10.0]}
    res = {}
    for name, reuse in (("one_pass", True), ("loop", False)):
        for rep in range(2):
            t0 = sync()
            r = project_forces_grid_cv(grid, coords, forces, n_folds=5, rng=np.random.default_rng(0), coord_map=cmap,
                                       constrained_inds=None, reuse_gram=reuse, method=joptgauss_map, var=0.01,
                                       kbt=0.6955215, seed=3)
            res[name] = (sync() - t0, r)
    a, b = res["one_pass"][1]["scores"], res["loop"][1]["scores"]
    worst = max(abs(a[k] - b[k]) / abs(b[k]) for k in a)
    emit(row="cv_noised", workload=f"joptgauss_map var 0.01, {T} x {N} x {n_cg} fp32, 5 folds x 4 l2 values",
         one_pass_s=res["one_pass"][0], loop_s=res["loop"][0], speedup=res["loop"][0] / res["one_pass"][0],
         max_rel_score_diff=worst, note="the loop draws fresh noise for every fit and application, the one-pass form one "
                                        "realisation for all: the difference is sampling noise")


def bench_staged():
    T, N, n_cg = 500_000, 2048, 128
    forces = K.synth_normal(T, N, torch.float32, 3, sigma=30.0)
    coords = K.synth_normal(T, N, torch.float32, 4, sigma=0.3, lattice=1.5)
    cmap = LinearMap([[i * (N // n_cg)] for i in range(n_cg)], n_fg_sites=N)
    traj = Trajectory(coords=coords, forces=forces)
    fits, applies = [], []
    for rep in range(4):
        t0 = sync()
        tm = stagedjoptgauss_map(traj, cmap, var=0.05, kbt=0.6, seed=7)
        t1 = sync()
        mapped = tm(traj)
        t2 = sync()
        fits.append(t1 - t0)
        applies.append(t2 - t1)
    fit_s, apply_s = min(fits[1:]), min(applies[1:])
    emit(row="staged", workload=f"stagedjoptgauss_map, {T} x {N} x {n_cg} fp32", fit_s=fit_s, apply_s=apply_s,
         frames_per_s=T / (fit_s + apply_s), mapped_shape=list(mapped.forces.shape), fit_reps_s=fits, apply_reps_s=applies)


def bench_k6():
    T, N = 2000, 4096
    x = K.synth_normal(T, N, torch.float32, 5, sigma=0.3, lattice=1.5)
    for rep in range(3):
        t0 = sync()
        K.pair_dist_var(x)
        dt = sync() - t0
    emit(row="k6", workload=f"pair-distance variance, {T} frames x {N} atoms", seconds=dt,
         pair_distances_per_s=T * N * (N - 1) / 2 / dt)
    del x
    bench_k6_box(T, N)


def bench_k6_box(T, N, calls=10, windows=5):
    """The open call, one box and a box per frame on the same float64 coordinates (wrapped into the cell), in one
    process: device events around ``calls`` calls, the three forms taken in turn, median of ``windows`` windows."""
    side = 1.5 * round(N ** (1 / 3))  # the cell of the lattice the sites jitter around
    x = K.synth_normal(T, N, torch.float64, 5, sigma=0.3, lattice=1.5)
    one = torch.full((3,), side, dtype=torch.float64, device=x.device)
    per_frame = (side * (1 + 0.03 * (2 * torch.rand(T, 3, dtype=torch.float64, device=x.device) - 1))).contiguous()
    x = (x - per_frame[:, None, :] * torch.floor(x / per_frame[:, None, :])).contiguous()
    forms = {"open": None, "box": one, "box_per_frame": per_frame}
    times = {name: [] for name in forms}
    for name, box in forms.items():  # warm-up: code objects, the workspace
        K.pair_dist_var(x, box=box)
    torch.cuda.synchronize()
    for _ in range(windows):
        for name, box in forms.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                K.pair_dist_var(x, box=box)
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) * 1e-3 / calls)
    med = {name: float(np.median(v)) for name, v in times.items()}
    emit(row="k6_box", workload=f"pair-distance variance, {T} frames x {N} atoms, float64, cell side {side:g}",
         timing=f"device events, {calls} calls per window, median of {windows} windows, forms in turn",
         open_s=med["open"], box_s=med["box"], box_per_frame_s=med["box_per_frame"],
         box_over_open=med["box"] / med["open"], box_per_frame_over_open=med["box_per_frame"] / med["open"],
         windows_s=times)


def bench_stream():
    T, N, n_cg = 200_000, 1024, 64
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        prefix = os.path.join(d, "run")
        for name, scale in (("coords", 0.3), ("forces", 30.0)):
            mm = np.lib.format.open_memmap(f"{prefix}_{name}.npy", mode="w+", dtype=np.float32, shape=(T, N, 3))
            for b in range(0, T, 20000):
                mm[b:b + 20000] = rng.standard_normal((min(20000, T - b), N, 3), dtype=np.float32) * scale
            mm.flush()
            del mm
        coords, forces = load_trajectory(prefix)
        cmap = LinearMap([[i * (N // n_cg)] for i in range(n_cg)], n_fg_sites=N)
        project_forces_streamed(coords[:2000], forces[:2000], cmap, None)
        for rep in range(2):
            t0 = time.perf_counter()
            project_forces_streamed(coords, forces, cmap, None)
            dt = time.perf_counter() - t0
    gb = 3 * T * N * 3 * 4 / 1e9
    emit(row="stream", workload=f"project_forces_streamed, {T} x {N} x {n_cg} fp32 from memory-mapped .npy",
         seconds=dt, host_to_device_GB_per_s=gb / dt, frames_per_s=T / dt)


if __name__ == "__main__":
    which = sys.argv[1:] or ["cv", "staged", "k6", "stream"]
    for w in which:
        {"cv": bench_cv, "cv_noised": bench_cv_noised, "staged": bench_staged, "k6": bench_k6, "stream": bench_stream}[w]()
        torch.cuda.empty_cache()
