"""Benchmark of the aggforce force-map hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

One step = one full ``project_forces`` (Gram build -> [all-reduce] -> constrained solve ->
map coordinates and forces -> residual) over a synthetic trajectory that is already resident
in HBM.  Default workload = the configuration BASELINE.json's metric is quoted on: 1e6 frames
x 4096 atoms x 256 CG beads, linear map, fp64 (configs[2]); it fits one MI355X (2 x 98.3 GB of
coordinates and forces + 12 GB of outputs).  With N > 1 ranks (torch.distributed.run, one
process per GPU) the SAME 1e6 frames are sharded over the ranks ("scaling": "strong"), each
rank builds the Gram matrix of its shard and one RCCL all-reduce combines them.  Typed as
``python bench.py --gpus N`` (no WORLD_SIZE in the environment) this process only LAUNCHES:
before anything touches the GPU it starts ``python -m torch.distributed.run --nproc-per-node N``
on this same file as a child, forwards rank 0's JSON line and exits with the child's code.

Rank 0 prints ONE JSON line: metric / value (frames/s, whole job) / roofline of the dominant
kernel (MFMA SYRK, HIP-event timed inside this run).  A plain run stops there: set-up, warm-up,
the timed steps, --dump-outputs, the line.  With --full (N=1 only) the line also carries
cpu_baseline (the NumPy oracle = a port of the reference's qplinear.py operation sequence, timed
on this box's host cores on a bounded frame sample; at c3 tens of seconds of host work).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# the host driver of this pool only supports dmabuf IPC (RCCL across processes needs it)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402

# torch is imported inside main(): the launcher branch must never initialise the GPU

WORKLOADS = {
    # name: (frames, atoms, cg beads, dtype)
    "c3": (1_000_000, 4096, 256, "f64"),   # BASELINE.json configs[2] -- the metric's configuration
    "c2": (100_000, 1024, 64, "f32"),      # configs[1]
    "tiny": (4096, 256, 16, "f64"),        # plumbing check
    "c4": (20_000, 1024, 64, "f32"),       # configs[3]: featurised id_feat + gb_feat (n_basis 8, cutoff 8)
    "c5": (500_000, 2048, 128, "f32"),     # configs[4]: joptgauss_map, var 0.01 (4 GPUs in BASELINE)
    # configs[0] at GPU scale: CLN025's topology (175 atoms, 10 CA beads, 59 constraint groups -> 97 reduced
    # variables; tests/golden/g4_cln025.npz) with many synthetic frames.  Intensity 97*98/(175*8) = 6.8 flop/B
    # is below the machine balance: the HBM-bound regime of the Gram build
    "c1": (4_000_000, 175, 10, "f64"),
}
METHOD_LABEL = {
    "c3": "linear qp_linear_map, no constraints",
    "c2": "linear qp_linear_map, no constraints",
    "tiny": "linear qp_linear_map, no constraints",
    "c4": "featurised qp_feat_linear_map (id_feat + gb_feat, n_basis 8), bond-pair constraints, fp64 Gram products",
    "c5": "noised joptgauss_map (var 0.01), no constraints",
    "c1": "linear qp_linear_map, CLN025 topology: 59 constraint groups (n_red 97), l2_regularization 1",
}
VARIANT_LABEL = {
    "pairs": "linear qp_linear_map, bond-pair constraints {3i, 3i+1} (n_red = N - N//3)",
    "zeronet": "linear qp_linear_map, no constraints, zero net force per frame (singular P)",
    "dense": "linear qp_linear_map, no constraints, dense centre-of-mass coordinate map",
}
PEAK_TFLOPS = {"f64": 78.6, "f32": 157.3}  # dense MFMA peaks (MI355X_MICROARCH.md / SURVEY 8(d))
SEED = 42100
KBT_BENCH = 0.6955215
VARIANT = "none"  # set by main(): the committed PMC profiles describe the plain c3 workload only


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    p.add_argument("--frames", type=int, default=None, help="override the total frame count")
    p.add_argument("--variant", default="none", choices=["none", "pairs", "zeronet", "dense"],
                   help="SURVEY 8(d) synthetic-input variants of the linear workloads (c2/c3/tiny): pairs = bond-pair "
                        "constraints {3i, 3i+1} (n_red = N - N//3: the `@ con_mat` group sums of qplinear.py:69-70); "
                        "zeronet = every frame's forces sum to zero (isolated molecule: P singular along the all-ones "
                        "vector, qplinear.py:71-86); dense = centre-of-mass coordinate map over contiguous blocks "
                        "(map/core.py:219-240: a second full K3 pass instead of the slice gather)")
    p.add_argument("--full", action="store_true",
                   help="also measure what the headline figure does not need: the CPU baseline after the timed steps "
                        "(N = 1 only). Off by default, so a plain run does set-up, warm-up, the timed steps and "
                        "--dump-outputs only")
    p.add_argument("--cpu-frames", type=int, default=20000,
                   help="with --full: frame sample of the CPU baseline (c3: ~20 s of host work: 2 GB of forces, two "
                        "2e12-flop matmuls, the single-threaded einsum apply)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    p.add_argument("--dry-run", action="store_true",
                   help="launcher self-test on CPU (gloo, no GPU, no product compute): NOT a measurement")
    p.add_argument("--dry-run-fail-rank", type=int, default=-1, help=argparse.SUPPRESS)
    p.add_argument("--rehearse-on-one-gpu", action="store_true",
                   help="N > 1 ranks that all use cuda:0 and talk over gloo (RCCL refuses two ranks on one device): "
                        "exercises the multi-rank code path on a one-GPU box; NOT a measurement")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last one returned to its caller as DIR/<name>.npy "
                        "(float32 / float64, at most 64 MB in all; the mapped trajectories as a fixed, seeded frame "
                        "sample when they are larger): the force map, the residual, mapped_forces, mapped_coords")
    a = p.parse_args(argv)
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    if a.dump_outputs and a.dry_run:
        p.error("--dump-outputs needs a run that computes (not --dry-run)")
    return a


def free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch(args, argv):
    """``python bench.py --gpus N`` typed by hand (N > 1, not under torch.distributed.run): start the N ranks as
    fresh child processes and forward rank 0's line.  Nothing here imports torch or calls HIP, so no process
    that has initialised the GPU is ever re-executed."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
    lines = []
    for raw in proc.stdout.decode(errors="replace").splitlines():
        try:
            rec = json.loads(raw)
        except ValueError:
            sys.stderr.write(raw + "\n")  # anything else a child printed
            continue
        if isinstance(rec, dict) and "metric" in rec:
            lines.append(raw)
    if proc.returncode != 0:
        sys.stderr.write(f"bench.py: a rank failed (torch.distributed.run exit code {proc.returncode})\n")
        return proc.returncode
    if len(lines) != 1:
        sys.stderr.write(f"bench.py: expected ONE result line from rank 0, got {len(lines)}\n")
        return 1
    sys.stdout.write(lines[0] + "\n")
    sys.stdout.flush()
    return 0


def dry_run(args, world, rank, result_fd):
    """The bench skeleton without the GPU: gloo rendezvous, barrier, max-over-ranks timing, the replicated-result
    check and the one-line output -- what the launcher test exercises on CPU."""
    import torch
    import torch.distributed as dist

    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    if rank == args.dry_run_fail_rank:
        raise SystemExit(3)
    t0 = time.perf_counter()
    payload = torch.arange(16, dtype=torch.float64)  # stands for the replicated solve's result
    if world > 1:
        dist.barrier()
    elapsed = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    spread = replicated_spread(payload, world)
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    if rank == 0:
        line = {"metric": "launcher dry run (no measurement)", "value": None, "unit": "frames/s", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "dry_run": True, "backend": "gloo",
                "world_size_seen": dist.get_world_size() if world > 1 else 1,
                "replicated_solve_max_abs_diff": spread}
        os.write(result_fd, (json.dumps(line) + "\n").encode())
    if world > 1:
        dist.destroy_process_group()


def replicated_spread(t, world):
    """max over entries of (max over ranks - min over ranks) of a tensor every rank computed for itself."""
    if world == 1:
        return 0.0
    import torch.distributed as dist

    hi, lo = t.clone(), t.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    return float((hi - lo).abs().max().item())


DUMP_BYTES = 60 << 20  # --dump-outputs: all arrays together; below 64 MB (decimal) with the .npy headers


def sample_frames(a, idx, begin, world):
    """Rows ``idx`` (sorted global frame numbers) of the frame-sharded array ``a`` (this rank holds frames
    begin..begin + len(a)), as a host array in a's dtype on every rank.  With N > 1 ranks each rank fills the rows
    it holds into a zero float64 buffer and one sum all-reduce assembles them: every row is non-zero on one rank
    only, and float32 survives the round trip through float64 exactly."""
    import torch

    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    mine = (idx >= begin) & (idx < begin + t.shape[0])
    rows = t[torch.from_numpy(idx[mine] - begin).to(t.device)]
    if world == 1:
        return rows.cpu().numpy()
    import torch.distributed as dist

    buf = torch.zeros((len(idx),) + tuple(t.shape[1:]), dtype=torch.float64, device="cuda")
    buf[torch.from_numpy(np.flatnonzero(mine)).cuda()] = rows.to("cuda", torch.float64)
    dist.all_reduce(buf)
    return buf.to(rows.dtype).cpu().numpy()


def dump_outputs(out_dir, out, solved, solved_name, T_total, begin, world, rank):
    """--dump-outputs: what the last timed step handed its caller, as out_dir/<name>.npy.  The fitted map and the
    residual are replicated on every rank; mapped_forces / mapped_coords are frame-sharded and share what is left of
    DUMP_BYTES: all frames when they fit, else the same seeded sample of frames for both (fixed by SEED and the total
    frame count, so runs with equal arguments dump equal frames whatever the GPU count).  Returns {name: shape}."""
    arrays = {solved_name: np.asarray(solved, dtype=np.float64), "residual": np.asarray(out["residual"], np.float64)}
    mapped = {k: out[k] for k in ("mapped_forces", "mapped_coords")}
    room = (DUMP_BYTES - sum(v.nbytes for v in arrays.values())) // len(mapped)
    row_bytes = max(int(np.prod(v.shape[1:])) * (v.element_size() if hasattr(v, "element_size") else v.dtype.itemsize)
                    for v in mapped.values())
    n = min(T_total, room // row_bytes)
    idx = (np.arange(T_total, dtype=np.int64) if n == T_total
           else np.sort(np.random.default_rng(SEED).choice(T_total, size=n, replace=False)).astype(np.int64))
    for k, v in mapped.items():
        arrays[k] = sample_frames(v, idx, begin, world)
    for k, v in arrays.items():
        if v.dtype not in (np.float32, np.float64):
            arrays[k] = v.astype(np.float64)
    total = sum(v.nbytes for v in arrays.values())
    assert total <= DUMP_BYTES, f"--dump-outputs: {total} bytes exceed the {DUMP_BYTES} byte budget"
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        for k, v in arrays.items():
            np.save(os.path.join(out_dir, k + ".npy"), v)
    return {k: list(v.shape) for k, v in arrays.items()}


def profiled_traffic(workload, world):
    """HBM-side bytes per launch of the Gram kernel from the committed rocprofv3 PMC passes
    (profiles/r05_c3_rocprof_summary.json; separate runs by construction).  FETCH_SIZE is in KiB
    and counts 128-byte requests as 64 bytes on gfx950 (MI355X_MICROARCH.md, HBM): x 2."""
    if workload != "c3" or world != 1 or VARIANT != "none":
        return None
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "r05_c3_rocprof_summary.json")))
        rd = [e["FETCH_SIZE"]["per_dispatch"] for e in d["pmc_fetch"] if "gram_tile" in e["kernel"]][0]
        wr = [e["WRITE_SIZE"]["per_dispatch"] for e in d.get("pmc_write", []) if "gram_tile" in e["kernel"]]
        return 2.0 * rd * 1024 + (wr[0] * 1024 if wr else 0.0)
    except Exception:
        return None


def profile_label():
    """Where `traffic` / `mfma_busy_frac_pmc` come from: PMC passes are separate rocprofv3 runs by construction, so
    the line quotes the committed profile and says which one (file, and the tree / date recorded inside it)."""
    rel = "profiles/r05_c3_rocprof_summary.json"
    label = f"{rel} (separate rocprofv3 --pmc passes; NOT measured in this run)"
    try:
        src = json.load(open(os.path.join(ROOT, rel))).get("profiled_from") or {}
        if src:
            label += f"; profiled from tree {src.get('tree')} on {src.get('date')}"
    except Exception:
        pass
    return label


def profiled_mfma_busy(workload, world):
    """Fraction of the Gram kernel's cycles in which the MFMA pipes were busy, from the committed PMC pass
    (profiles/r05_c3_mfma_counters.json: SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8))."""
    if workload != "c3" or world != 1 or VARIANT != "none":
        return None
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "r05_c3_mfma_counters.json")))
        return [v["mfma_utilisation"] for k, v in d["kernels"].items() if "gram_tile" in k][0]
    except Exception:
        return None


def blas_threads():
    """BLAS threads the CPU baseline runs on: every logical core of the host is ASKED for (threadpoolctl); the
    library grants at most the thread count it was built for (NumPy's bundled OpenBLAS: 64), and what it granted is
    what the line reports."""
    try:
        from threadpoolctl import threadpool_info, threadpool_limits

        threadpool_limits(limits=os.cpu_count() or 1, user_api="blas")
        n = [i["num_threads"] for i in threadpool_info() if i.get("user_api") == "blas"]
        return max(n) if n else 1
    except Exception:
        return 1


def gram_kernel_name(launched, family):
    """The Gram kernel of the timed steps, named by the library's own launch table (aggf_coverage_dump): the
    instantiation of `family` with the most launches since the reset -- the string rocprofv3 prints, minus the
    argument list."""
    best = max(((cnt, pretty) for pretty, cnt in launched.values() if family in pretty and cnt > 0), default=None)
    if best is None:
        return None
    name = best[1]
    depth = 0
    for i, ch in enumerate(name):  # cut the parameter list: the first '(' outside the template brackets
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            name = name[:i]
            break
    return name.replace("void ", "").strip()


def cpu_baseline(N, n_cg, np_dtype, T_total, T_cpu, cores, cmat=None, constraints=None, l2=0.0, zeronet=False,
                 noised=None):
    """Reference operation sequence (qplinear.py:66-88, util.py:119-125, agg.py:120-136) in NumPy
    on a frame sample; T-linear stages are scaled to T_total, the solve is counted once.
    ``noised`` = (var, kbt): the joptgauss_map sequence (jgauss.py:114-131: augment, linear fit on N + n_cg sites,
    re-augment and apply as AugmentedTMap.__call__ does, tmap.py:240-243) with NumPy's generator for the noise."""
    from oracle import aggforce_oracle as orc

    rng = np.random.default_rng(SEED)
    forces = (30 * rng.standard_normal((T_cpu, N, 3))).astype(np_dtype)
    coords = rng.random((T_cpu, N, 3)).astype(np_dtype)
    if zeronet:
        forces -= forces.mean(axis=1, keepdims=True)
    if cmat is None:
        cmat = orc.list_mapping_matrix([[i * (N // n_cg)] for i in range(n_cg)], N)
    cons = set() if constraints is None else constraints
    # The sequence is timed TWICE on the same sample and the faster pass is reported (the first pass also warms the
    # BLAS thread pool and the page cache of the sample; box-to-box the figure still moves by tens of per cent with the
    # host's load and core count: a stated baseline, not a measured speed-up -- VERDICT r3 weak 11).
    passes = []
    for _rep in range(2):
        passes.append(_cpu_pass(orc, rng, coords, forces, cmat, cons, l2, noised, N, n_cg, np_dtype, T_cpu))
    best = min(passes, key=lambda p: p["lin"] * (T_total / T_cpu) + p["solve"])
    t_aug, gram_s, solve_s, apply_s, n_red_cpu, res, mc_sum = (best[k] for k in ("aug", "gram", "solve", "apply", "n_red", "res", "mc"))
    full = best["lin"] * (T_total / T_cpu) + solve_s
    values = [T_total / (p["lin"] * (T_total / T_cpu) + p["solve"]) for p in passes]
    return {
        "value": T_total / full,
        "unit": "frames/s",
        "cores": cores,
        "kind": "port",
        "passes_frames_per_s": values,
        "sample": (f"{T_cpu} of {T_total} frames x {N} atoms on the host ({os.cpu_count()} logical cores; every one was asked "
                   f"for, BLAS threads granted = cores field -- the thread count NumPy's OpenBLAS is built for; the einsum apply "
                   f"is single-threaded as in the reference), faster of two passes: "
                   + (f"augment {t_aug:.2f}s, " if noised is not None else "")
                   + f"gram {gram_s:.2f}s (n_red {n_red_cpu}), "
                   f"solve {solve_s:.2f}s (exact direct solve instead of {n_cg} OSQP runs), "
                   + ("re-augment + " if noised is not None else "")
                   + f"apply+residual {apply_s:.2f}s; T-linear stages scaled to {T_total} frames, "
                   f"solve counted once"),
        "_check": float(res + mc_sum * 0),
    }


def _cpu_pass(orc, rng, coords, forces, cmat, cons, l2, noised, N, n_cg, np_dtype, T_cpu):
    """One timed pass of the reference's operation sequence on the sample (see cpu_baseline)."""
    t_aug = 0.0
    fit_cmat, fit_coords, fit_forces = cmat, coords, forces
    if noised is not None:
        var, kbt = noised
        ta = time.perf_counter()
        noise = rng.standard_normal((T_cpu, n_cg, 3)).astype(np_dtype)
        fit_coords, fit_forces = orc.augment(coords, forces, cmat, var, kbt, noise, dtype=np_dtype)
        fit_cmat = orc.list_mapping_matrix([[x] for x in range(N, N + n_cg)], N + n_cg)
        t_aug = time.perf_counter() - ta
    t0 = time.perf_counter()
    pr = orc.linear_problem(fit_forces, fit_cmat, cons, l2)     # qp_form, @con_mat, Gram
    t1 = time.perf_counter()
    X = orc.eq_qp_solve(pr["qp_mat"], None, pr["A"], np.eye(n_cg))  # exact solve in place of OSQP
    W = (pr["con_mat"] @ X).T
    t2 = time.perf_counter()
    if noised is not None:  # the returned map re-augments with fresh noise when it is applied
        noise = rng.standard_normal((T_cpu, n_cg, 3)).astype(np_dtype)
        fit_coords, fit_forces = orc.augment(coords, forces, cmat, noised[0], noised[1], noise, dtype=np_dtype)
    mc = orc.linearmap_apply(fit_coords, fit_cmat)
    mf = orc.linearmap_apply(fit_forces, W)
    res = orc.force_smoothness(mf)
    t3 = time.perf_counter()
    return {"lin": t_aug + (t1 - t0) + (t3 - t2), "aug": t_aug, "gram": t1 - t0, "solve": t2 - t1, "apply": t3 - t2,
            "n_red": pr["qp_mat"].shape[0], "res": float(res), "mc": float(mc.sum())}


def cpu_baseline_featurised(cores, n_basis=8, outer=8.0, T_cpu=500):
    """The featurised fit in the reference's formulation cannot run at BASELINE config 4's size at all (the dense
    one-hot feature tensor is 2e4 x 1024 x 6139 float32 = 503 GB per cg site), so the port is timed at
    CLN025-like size -- 175 atoms, 10 CA beads, the 59 constraint groups of tests/golden/g4_cln025.npz, T_cpu
    frames -- and the figure says so: it is NOT the same workload as `value`."""
    from oracle import aggforce_oracle as orc

    topo = np.load(os.path.join(ROOT, "tests", "golden", "g4_cln025.npz"))
    cons = {frozenset(int(x) for x in row if x >= 0) for row in topo["pairs"]}
    N, ca = 175, [int(i) for i in topo["ca"]]
    cmat = orc.list_mapping_matrix([[i] for i in ca], N)
    rng = np.random.default_rng(SEED)
    side = 6
    base = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:N] * 1.5
    coords = (base[None] + 0.3 * rng.standard_normal((T_cpu, N, 3))).astype(np.float32)
    forces = (30 * rng.standard_normal((T_cpu, N, 3))).astype(np.float32)
    t0 = time.perf_counter()
    ids = orc.id_feat_ids(N, cons)
    G = int(ids.max()) + 1
    smear = orc.smear_matrix(orc.reduce_constraint_sets(cons), N)
    cg = orc.linearmap_apply(coords, cmat)
    onehot = np.zeros((T_cpu, N, G), dtype=np.float32)
    onehot[:, np.arange(N), ids] = 1
    frames = [rng.choice(T_cpu, size=20, replace=False) for _ in ca]
    feats, divs, coefs = [], [], []
    for c in range(len(ca)):  # featlinearmap.py:349-384, site by site like the reference's lazy generators
        gf, gd = orc.gb_feat_site(coords, cg[:, c, :], ids, smear, outer=outer, n_basis=n_basis, n_channels=G - 1)
        feat = np.concatenate([onehot, gf], axis=2)
        div = np.concatenate([np.zeros((T_cpu, G, 3), np.float32), gd], axis=1)
        A, b = orc.feat_constraint_arrays(feat, c, cmat, frames[c])
        _, qp_mat = orc.feat_site_problem(forces, feat, div, KBT_BENCH, 10.0)
        coefs.append(orc.eq_qp_solve(qp_mat, None, A, b))
        feats.append(feat)
        divs.append(div)
    t1 = time.perf_counter()
    mf = orc.cla_apply(forces, feats, divs, coefs)  # the reference re-runs the featuriser here (featlinearmap.py:513,518)
    t2 = time.perf_counter()
    return {
        "value": T_cpu / (t2 - t0),
        "unit": "frames/s",
        "cores": cores,
        "kind": "port",
        "sample": (f"NOT this workload: the reference's dense formulation at CLN025-like size ({T_cpu} frames x {N} atoms x "
                   f"{len(ca)} beads, 59 constraint groups, n_feat {feats[0].shape[2]}, n_basis {n_basis}, 20 constraint frames); "
                   f"fit {t1 - t0:.2f}s, apply {t2 - t1:.2f}s (features reused, the reference recomputes them twice). At "
                   f"config-4 size its feature tensor alone is 503 GB per site"),
        "_check": float(np.sum(mf) * 0),
    }


def main():
    argv = sys.argv[1:]
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch(args, argv))
    # ONE JSON line on stdout: libraries (RCCL prints a version banner on init) write to fd 1, so fd 1
    # is pointed at stderr for the run and the result line goes to the saved descriptor.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.dry_run:
        return dry_run(args, world, rank, result_fd)
    import torch

    if args.rehearse_on_one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    comm = None
    if world > 1 or "TORCHELASTIC_RUN_ID" in os.environ:  # under torch.distributed.run: always RCCL
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.rehearse_on_one_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        comm = dist.group.WORLD

    from aggforce_amd import LinearMap, project_forces
    from aggforce_amd import _kernels as K
    from aggforce_amd.distributed import frame_shard

    global VARIANT
    VARIANT = args.variant
    T_total, N, n_cg, dt = WORKLOADS[args.workload]
    if args.frames:
        T_total = args.frames
    tdt = torch.float64 if dt == "f64" else torch.float32
    begin, end = frame_shard(T_total, rank, world)
    T_local = end - begin
    # synthetic, counter-based: identical data for any GPU count
    forces = K.synth_normal(T_local, N, tdt, SEED, frame_offset=begin, sigma=30.0)
    coords = K.synth_normal(T_local, N, tdt, SEED + 1, frame_offset=begin, sigma=0.3, lattice=1.5)
    cmap = LinearMap([[i * (N // n_cg)] for i in range(n_cg)], n_fg_sites=N)
    kwargs = {"comm": comm} if comm is not None else {}
    constraints = set()
    KBT = KBT_BENCH
    if args.variant != "none" and args.workload not in ("c2", "c3", "tiny"):
        raise SystemExit("--variant applies to the linear workloads c2 / c3 / tiny")
    n_red = N
    if args.variant == "pairs":
        constraints = {frozenset([3 * i, 3 * i + 1]) for i in range(N // 3)}
        n_red = N - N // 3
    elif args.variant == "zeronet":
        # data preparation (outside the timed region): every frame's net force removed, in place, by frame blocks
        blk = max(1, (1 << 28) // (3 * N))
        for t0_ in range(0, T_local, blk):
            chunk = forces[t0_:t0_ + blk]
            chunk -= chunk.mean(dim=1, keepdim=True)
        del chunk
    elif args.variant == "dense":
        w = N // n_cg
        cmap = LinearMap([list(range(i * w, (i + 1) * w)) for i in range(n_cg)], n_fg_sites=N)
    if args.workload == "c4":
        # bond-pair constraints {3i, 3i+1}; every cg site is a constrained atom (its smeared position
        # differs from the site, r > 0 -- as for CLN025's CA/HA; with r == 0 the reference is NaN)
        from aggforce_amd.qp import Multifeaturize, gb_feat, id_feat, qp_feat_linear_map
        from aggforce_amd.util import Curry

        constraints = {frozenset([3 * i, 3 * i + 1]) for i in range(N // 3)}
        cmap = LinearMap([[3 * (i * (N // n_cg) // 3)] for i in range(n_cg)], n_fg_sites=N)
        kwargs.update(method=qp_feat_linear_map, kbt=KBT, l2_regularization=10.0, n_constraint_frames=20,
                      featurizer=Multifeaturize([id_feat, Curry(gb_feat, outer=8.0, inner=0.0, n_basis=8, width=1.0)]),
                      rng=np.random.default_rng(SEED))
    elif args.workload == "c5":
        from aggforce_amd import joptgauss_map

        kwargs.update(method=joptgauss_map, var=0.01, kbt=KBT, seed=SEED, frame_offset=begin)
    elif args.workload == "c1":
        topo = np.load(os.path.join(ROOT, "tests", "golden", "g4_cln025.npz"))
        constraints = {frozenset(int(x) for x in row if x >= 0) for row in topo["pairs"]}
        cmap = LinearMap([[int(i)] for i in topo["ca"]], n_fg_sites=N)
        kwargs.update(l2_regularization=1.0)

    def step():
        return project_forces(coords=coords, forces=forces, coord_map=cmap, constrained_inds=constraints, **kwargs)

    def barrier():
        if comm is not None:
            import torch.distributed as dist

            dist.barrier()
        torch.cuda.synchronize()

    # the previous step's 12 GB of mapped arrays are released before the next step, as a caller's
    # loop would do; otherwise every step pays a fresh hipMalloc of its outputs
    out = None
    for _ in range(args.warmup):
        out = None
        out = step()
    barrier()
    from aggforce_amd import _lib
    from aggforce_amd import distributed as D

    _lib.load().aggf_coverage_reset()   # the launch table then names the kernels of the timed steps only
    D.reset_collective_stats()
    K.start_timers()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = None
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    stages = K.stop_timers()
    launched = _lib.coverage(names=True)  # mangled -> (name as rocprofv3 prints it, launches in the timed region)
    coll = D.collective_stats()
    if comm is not None:
        import torch.distributed as dist

        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = tmax.item()
    fmap = getattr(out["tmap"], "force_map", None)
    if fmap is None and hasattr(out["tmap"], "tmap"):  # noised maps: the linear map of the extended system
        fmap = getattr(out["tmap"].tmap, "force_map", None)
    if hasattr(fmap, "standard_matrix"):
        W = fmap.standard_matrix
        cons_resid = (float(np.max(np.abs(cmap.standard_matrix @ W.T - np.eye(n_cg))))
                      if W.shape[1] == cmap.standard_matrix.shape[1] else None)
        solved = np.asarray(W, dtype=np.float64)
        solved_name = "force_map"
    else:
        cons_resid = None
        solved = np.stack([np.asarray(c, dtype=np.float64) for c in fmap.tags["coef_list"]])
        solved_name = "force_map_coefs"
    # the solve is replicated, not broadcast: every rank must hold the same map, bit for bit
    w_spread = replicated_spread(torch.from_numpy(np.ascontiguousarray(solved)).cuda(), world)
    dumped = None
    if args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, out, solved, solved_name, T_total, begin, world, rank)
    world_seen = 1
    if comm is not None:
        import torch.distributed as dist

        world_seen = dist.get_world_size()

    if rank == 0:
        gram = stages.get("gram", {"ms": float("nan"), "calls": 1})
        gram_ms = gram["ms"] / max(1, gram["calls"])
        gdt = "f64" if args.workload == "c4" else dt  # arithmetic type of the Gram products
        s_bytes = 8 if dt == "f64" else 4
        n_gram = n_red
        if args.workload == "c5":
            n_gram = N + n_cg
        elif args.workload == "c1":
            n_gram = 97
        flops = 3.0 * T_local * n_gram * (n_gram + 1)  # SYRK, upper triangle, per launch
        gram_note = None
        if args.workload == "c4":
            # one launch per cg site, over the feature columns that site keeps (columns that vanish over the whole
            # trajectory are left out, qp/gbfeat.py); flops_per_launch = mean over the sites' launches
            kept = out["tmap"].force_map.tags["fit_info"]["kept_columns"]
            # the id x id block (whole 128-tiles of it) is identical for all sites: formed by the first launch only
            lead = ((N - N // 3) // 128) * 128
            flops = float(np.mean([3.0 * T_local * (k * (k + 1) - (lead * (lead + 1) if i else 0))
                                   for i, k in enumerate(kept)]))
            gram_note = (f"{len(kept)} launches per step over {min(kept)}..{max(kept)} kept feature columns of "
                         f"{out['tmap'].force_map.tags['fit_info']['n_feat']} (mean {np.mean(kept):.0f}); the launches of "
                         f"different sites overlap on 3 streams (solve batches {out['tmap'].force_map.tags['fit_info']['solve_batches']}), so ms_per_launch = (HIP-event time of the whole site loop on "
                         "the main stream, which also contains the gb_regmat_cols and constraint-row kernels) / launches: "
                         "a lower bound of the kernel's own rate")
            phase = stages.get("fit_sites")
            if phase:
                gram_ms = phase["ms"] / args.steps / len(kept)  # one bracket per batch of sites, all launches of a step
        if args.workload == "c1":
            # HBM-bound: algorithmic bytes of the Gram pass = one read of the forces (3 N s per frame)
            algo_bytes = 3.0 * N * s_bytes * T_local
            achieved = algo_bytes / (gram_ms * 1e-3) / 1e9
            roof = {"kernel": f"aggf_gram = {gram_kernel_name(launched, 'gram_small_kernel')} (fused group sums, one pass over F) + gram_reduce_small_kernel",
                    "bound": "hbm", "co_limited_by": "hbm+mfma+lds: per frame and CU 403 cycles of HBM, 336 of MFMA (28 upper-triangle "
                    "16x16 blocks), ~340 of group sums; float64 MFMAs occupy their SIMD's vector datapath, so sums and MFMAs add up "
                    "instead of overlapping whatever the wave roles (profiles/r05_ws_ablation_*.txt; the stream itself reaches "
                    "6.4-7.1 TB/s: profiles/r05_ldsdma_fill.jsonl): floor ~0.48 of 8 TB/s for this formulation; ablations in "
                    "profiles/r04_small_ablate.jsonl (no MFMA phase 2.86 ms, no loads 4.05, no group sums 3.73, complete 4.79)",
                    "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                    "traffic": None, "ms_per_launch": gram_ms, "bytes_per_launch": algo_bytes,
                    "flops_per_launch": flops, "mfma_tflops": flops / (gram_ms * 1e-3) / 1e12}
        else:
            achieved = flops / (gram_ms * 1e-3) / 1e12
            # the full template name as rocprofv3 prints it, read from the library's launch table of the timed steps
            kname = "%s (+ gram_reduce_kernel) = %s" % (
                gram_kernel_name(launched, "gram_tile_dma_kernel") or gram_kernel_name(launched, "gram_small_kernel"),
                "aggf_gram_pair" if args.workload == "c5" else "aggf_gram")
            packer = gram_kernel_name(launched, "pack_groups_kernel")
            if packer:  # constraint-group sums / conversion / padding in front of the tile kernel
                kname = packer + " + " + kname
            roof = {"kernel": kname, "bound": "mfma", "achieved": achieved, "peak": PEAK_TFLOPS[gdt], "unit": "TFLOP/s",
                    "frac": achieved / PEAK_TFLOPS[gdt], "traffic": profiled_traffic(args.workload, world),
                    "traffic_source": profile_label() if profiled_traffic(args.workload, world) is not None else None,
                    "mfma_busy_frac_pmc": profiled_mfma_busy(args.workload, world), "ms_per_launch": gram_ms,
                    "flops_per_launch": flops}
            if gram_note:
                roof["launches"] = gram_note
        per_step = {k: v["ms"] / args.steps for k, v in stages.items()}
        line = {
            "metric": "frames/sec through project_forces (Gram+solve), 1e6x4096-atom traj, 1/2/4/8 GPU",
            "value": T_total * args.steps / elapsed,
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": dt,
            "data": "synthetic",
            "config": {
                "workload": (f"{args.workload}{'' if args.variant == 'none' else '+' + args.variant}: {T_total} frames x {N} atoms x "
                             f"{n_cg} CG beads, {VARIANT_LABEL.get(args.variant) or METHOD_LABEL[args.workload]}, "
                             f"{dt} trajectory, {'dense block-average' if args.variant == 'dense' else 'slice'} coord map, "
                             f"frames sharded over {world} GPU(s)"),
                "variant": args.variant,
                "n_red": n_gram,
                "frames_per_gpu": T_local,
                "stage_ms_per_step": per_step,
                # the terms of the strong-scaling model, read off this run instead of projected: what divides by the
                # number of GPUs (gram, apply, gather, ...), what does not (the replicated solve + the host time between
                # the stages: wall minus every stage of the main stream) and the collective (pack + all-reduce + unpack)
                "allreduce_ms_per_step": per_step.get("allreduce", 0.0 if comm is None else None),
                # payload of the sum all-reduces per step (the packed upper triangle of G + scalars) and the ring's bus
                # bandwidth 2 (N - 1) / N x bytes / time, to read against xGMI's ~153 GB/s per link
                "allreduce_bytes_per_step": coll["allreduce_bytes"] / args.steps,
                "allreduce_calls_per_step": coll["allreduce_calls"] / args.steps,
                "allreduce_bus_GBps": (2.0 * (world - 1) / world * coll["allreduce_bytes"] / args.steps
                                       / (per_step["allreduce"] * 1e-3) / 1e9
                                       if world > 1 and per_step.get("allreduce") else None),
                "replicated_ms_per_step": per_step.get("solve", 0.0) + max(0.0, 1e3 * elapsed / args.steps - sum(
                    v for k, v in per_step.items() if k != "gather")),
                "constraint_residual": cons_resid,
                "residual": out["residual"],
                "collective": ("REHEARSAL: gloo, all ranks on cuda:0 -- not a measurement" if args.rehearse_on_one_gpu
                               else "RCCL all-reduce of the Gram matrix (torch.distributed backend nccl)" if comm is not None
                               else "none (single process)"),
                "backend": (None if comm is None else "gloo" if args.rehearse_on_one_gpu else "nccl (RCCL)"),
                "world_size_seen": world_seen if comm is not None else None,
                "replicated_solve_max_abs_diff_across_ranks": w_spread,
            },
            "roofline": roof,
        }
        if dumped is not None:
            line["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        if args.full and world == 1 and not args.no_cpu_baseline:
            del out
            npdt = np.float64 if dt == "f64" else np.float32
            cm_host = np.asarray(cmap.standard_matrix, dtype=np.float64)
            if args.workload == "c4":
                cb = cpu_baseline_featurised(blas_threads())
            elif args.workload == "c5":
                cb = cpu_baseline(N, n_cg, npdt, T_total, min(args.cpu_frames // 5, T_total), blas_threads(), cmat=cm_host,
                                  noised=(0.01, KBT))
            elif args.workload == "c1":
                cb = cpu_baseline(N, n_cg, npdt, T_total, min(20 * args.cpu_frames, T_total), blas_threads(), cmat=cm_host,
                                  constraints=constraints, l2=1.0)
            else:
                cb = cpu_baseline(N, n_cg, npdt, T_total, min(args.cpu_frames, T_total), blas_threads(), cmat=cm_host,
                                  constraints=constraints, zeronet=args.variant == "zeronet")
            cb.pop("_check")
            line["cpu_baseline"] = cb
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(line) + "\n").encode())
    if comm is not None:
        import torch.distributed as dist

        dist.destroy_process_group()


if __name__ == "__main__":
    main()
