"""Map application and its backward contractions (K3 / K3c forward, K8 backward) on one GPU.

Prints one JSON line per case:
  2-D map   T = 1e5, N = 4096, n_cg = 256 (f64, f32) and CLN025's size T = 1e6, N = 166, n_cg = 10 (f64):
            fwd = K3 apply, fwd_T = K3 on the transposed map (the dP of the backward), cross = K8a (the map gradient);
  3-D factor T = 1e4, n_cg = 64, N = 1024 (f32, f64):
            fwd = K3c, frames_t = K8b (dP), outer = K8c (dF).
For each kernel: ``<op>_ms`` (with --rocprof: the dispatch time from a separate `rocprofv3 --kernel-trace --stats` run of
this script, the median of --reps dispatches; without: CUDA events around the call, best of --reps), the algorithmic
flops or bytes, and the share of the relevant peak (78.6 TF fp64 MFMA, 157.3 TF fp32 MFMA, 8 TB/s HBM).
``backward_ms``: CUDA events around a full autograd backward() of Apply / ApplyFrames with both gradients, best of --reps,
and ``backward_over_fwd`` its ratio to the forward's event time.
Usage (GPU box): python tools/trjgrad_bench.py [--rocprof OUTDIR] > lines.jsonl
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64, PEAK_F32, PEAK_BW = 78.6e12, 157.3e12, 8.0e12
CASES = [  # (name, rank, T, n_cg, N, dtype)
    ("map2d_f64", 2, 100000, 256, 4096, "f64"),
    ("map2d_f32", 2, 100000, 256, 4096, "f32"),
    ("cln025_f64", 2, 1000000, 10, 166, "f64"),
    ("frames_f32", 3, 10000, 64, 1024, "f32"),
    ("frames_f64", 3, 10000, 64, 1024, "f64"),
]
OPS = {2: ("fwd", "fwd_T", "cross"), 3: ("fwd", "frames_t", "outer")}
FAMILY = {"fwd": ("apply_kernel", "apply_small_kernel", "apply_dma_kernel", "trjdot_frames_kernel"),
          "fwd_T": ("apply_kernel", "apply_small_kernel", "apply_dma_kernel"),
          "cross": ("trjdot_cross_kernel", "trjdot_cross_reduce"),
          "frames_t": ("trjdot_frames_t_kernel",), "outer": ("trjdot_frames_outer_kernel",)}


def make(rank, T, n_cg, N, dt):
    import torch

    dtype = torch.float32 if dt == "f32" else torch.float64
    g = torch.Generator(device="cuda").manual_seed(T + N)
    P = torch.randn((T, N, 3), generator=g, device="cuda", dtype=dtype)
    H = torch.randn((T, n_cg, 3), generator=g, device="cuda", dtype=dtype)
    M = torch.rand((n_cg, N) if rank == 2 else (T, n_cg, N), generator=g, device="cuda", dtype=dtype)
    return P, H, M


def op_calls(rank, P, H, M):
    from aggforce_amd import _kernels as K

    if rank == 2:
        MT = M.t().contiguous()
        return {"fwd": lambda: K.linearmap_apply(P, M), "fwd_T": lambda: K.linearmap_apply(H, MT),
                "cross": lambda: K.trjdot_cross(H, P, M.dtype)}
    return {"fwd": lambda: K.trjdot_frames(P, M), "frames_t": lambda: K.trjdot_frames_t(H, M, P.dtype),
            "outer": lambda: K.trjdot_frames_outer(H, P, M.dtype)}


def work(rank, op, T, n_cg, N, s):
    """('flop' | 'byte', algorithmic amount) of one call."""
    if op == "cross":
        return "flop", 2.0 * n_cg * N * 3 * T
    if rank == 2:  # K3 both ways: the (T, N, 3) and (T, n_cg, 3) arrays once each
        return "byte", float(s * T * 3 * (N + n_cg))
    if op == "outer":  # writes (T, n_cg, N), reads both (T, ., 3)
        return "byte", float(s * T * (n_cg * N + 3 * N + 3 * n_cg))
    return "byte", float(s * T * (n_cg * N + 3 * N + 3 * n_cg))


def event_ms(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def backward_ms(rank, P, H, M, reps):
    import torch

    from aggforce_amd._autograd import Apply, ApplyFrames

    p, m = P.detach().requires_grad_(True), M.detach().requires_grad_(True)

    def step():
        y = Apply.apply(p, m) if rank == 2 else ApplyFrames.apply(p, m)
        p.grad = m.grad = None
        t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t[0].record()
        y.backward(H)
        t[1].record()
        t[1].synchronize()
        return t[0].elapsed_time(t[1])

    step()
    return min(step() for _ in range(reps))


def child(args):
    """One dispatch of every op, --reps times, cases and ops in order (the rocprofv3 run)."""
    import torch

    for name, rank, T, n_cg, N, dt in CASES:
        if args.cases and name not in args.cases:
            continue
        P, H, M = make(rank, T, n_cg, N, dt)
        calls = op_calls(rank, P, H, M)
        for op in OPS[rank]:
            for _ in range(args.reps):
                calls[op]()
            torch.cuda.synchronize()
        del P, H, M, calls
        torch.cuda.empty_cache()


def rocprof(args, recs):
    d = os.path.abspath(args.rocprof)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
    if args.cases:
        cmd += ["--cases", *args.cases]
    with open(os.path.join(d, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=args.rocprof_timeout)
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(trace) == 1, trace
    rows = [r for r in csv.DictReader(open(trace[0])) if "aggf::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    i = 0
    for rec in recs:
        for op in OPS[rec["rank"]]:
            per_call = 2 if op == "cross" else 1
            times, names = [], set()
            for _ in range(args.reps):
                ns = 0
                for _ in range(per_call):
                    r = rows[i]
                    i += 1
                    assert any(f in r["Kernel_Name"] for f in FAMILY[op]), (rec["case"], op, r["Kernel_Name"])
                    names.add(r["Kernel_Name"].split("(")[0].replace("void ", ""))
                    ns += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                times.append(ns * 1e-6)
            rec[op + "_ms"] = round(statistics.median(times), 4)
            rec[op + "_kernels"] = sorted(names)
            rec[op + "_timing"] = "rocprofv3"
    assert i == len(rows), (i, len(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=None)
    ap.add_argument("--rocprof", metavar="OUTDIR")
    ap.add_argument("--rocprof-timeout", type=int, default=900)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    import torch

    recs = []
    for name, rank, T, n_cg, N, dt in CASES:
        if args.cases and name not in args.cases:
            continue
        P, H, M = make(rank, T, n_cg, N, dt)
        s = P.element_size()
        rec = {"case": name, "rank": rank, "T": T, "n_cg": n_cg, "N": N, "dtype": dt}
        for op, fn in op_calls(rank, P, H, M).items():
            rec[op + "_ms"] = round(event_ms(fn, args.reps), 4)
            rec[op + "_timing"] = "events"
        rec["backward_ms"] = round(backward_ms(rank, P, H, M, args.reps), 4)
        rec["backward_over_fwd"] = round(rec["backward_ms"] / rec["fwd_ms"], 3)
        recs.append(rec)
        del P, H, M
        torch.cuda.empty_cache()
    if args.rocprof:
        rocprof(args, recs)
    for rec in recs:
        s = 4 if rec["dtype"] == "f32" else 8
        for op in OPS[rec["rank"]]:
            kind, amount = work(rec["rank"], op, rec["T"], rec["n_cg"], rec["N"], s)
            sec = rec[op + "_ms"] * 1e-3
            if kind == "flop":
                peak = PEAK_F32 if rec["dtype"] == "f32" else PEAK_F64
                rec[op + "_tflops"] = round(amount / sec * 1e-12, 2)
            else:
                peak = PEAK_BW
                rec[op + "_tbps"] = round(amount / sec * 1e-12, 3)
            rec[op + "_" + kind + "s"] = amount
            rec[op + "_peak_share"] = round(amount / sec / peak, 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
