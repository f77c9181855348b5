"""Differentiable pair distances (K9) on one GPU: kernel rates, and jaxutil.distances against the plain-torch body it
replaces.

Prints one JSON line per case, (T, m, n) = (1e4, 256, 256) and (1e5, 64, 64) in float32 and float64:
  kernels    dist = K9a DIST, dot = K9a DOT, pull = K9b on given weights, pull_dv = K9b dividing by a distance array:
             ``<op>_ms`` (with --rocprof: the dispatch time from a separate `rocprofv3 --kernel-trace --stats` run of
             this script, the median of --reps dispatches; without: device events around the call, median of --reps),
             the algorithmic bytes (the (T, m, n) arrays once, the site arrays once) and their share of 8 TB/s;
  end to end the self-distance matrix of x, U = sum exp(-(d - 1)^2): ``fwd_bwd`` = distances + U + backward to x,
             ``double_bwd`` = the force-matching step g = dU/dx (create_graph), d|g|^2/dx; ``fused`` = jaxutil.distances,
             ``plain`` = the torch body restated below (displacements (T, m, n, 3), then a norm).  Device events, median
             of --reps, the two alternating in one loop; ``*_peak_gb`` = torch.cuda.max_memory_allocated of one step.
             The plain double backward returns NaN (the zero diagonal); its time and memory are still those of the ops.
Usage (GPU box): python tools/distgrad_bench.py [--rocprof OUTDIR] > profiles/distgrad_bench.jsonl
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

PEAK_BW = 8.0e12
CASES = [  # (name, T, m, n, dtype)
    ("n256_f32", 10000, 256, 256, "f32"),
    ("n256_f64", 10000, 256, 256, "f64"),
    ("n64_f32", 100000, 64, 64, "f32"),
    ("n64_f64", 100000, 64, 64, "f64"),
]
OPS = ("dist", "dot", "pull", "pull_dv")
FAMILY = {"dist": "pairdist_kernel", "dot": "pairdist_kernel", "pull": "pairpull_kernel", "pull_dv": "pairpull_kernel"}


def make(T, m, n, dt):
    import torch

    dtype = torch.float32 if dt == "f32" else torch.float64
    g = torch.Generator(device="cuda").manual_seed(T + n)
    side = 1  # bench.py's recipe: a 1.5-spaced lattice with 0.3 of noise per frame
    while side**3 < n:
        side += 1
    a = torch.arange(n, device="cuda")
    lat = 1.5 * torch.stack([a % side, (a // side) % side, a // side**2], dim=1).to(dtype)
    x = lat[None] + 0.3 * torch.randn((T, n, 3), generator=g, device="cuda", dtype=dtype)
    v = torch.randn((T, n, 3), generator=g, device="cuda", dtype=dtype)
    w = torch.randn((T, m, n), generator=g, device="cuda", dtype=dtype)
    return x.contiguous(), v, w


def op_calls(x, v, w):
    from aggforce_amd import _kernels as K

    d = K.pair_dist(x, x, K.PAIR_DIST)
    return {"dist": lambda: K.pair_dist(x, x, K.PAIR_DIST), "dot": lambda: K.pair_dist(x, x, K.PAIR_DOT, v, v),
            "pull": lambda: K.pair_pull(w, x, x), "pull_dv": lambda: K.pair_pull(w, x, x, dv=d)}


def op_bytes(op, T, m, n, s):
    sites = 3 * (n + m)
    if op == "dist":
        return float(s * T * (m * n + sites))
    if op == "dot":
        return float(s * T * (m * n + 2 * sites))
    return float(s * T * ((2 if op == "pull_dv" else 1) * m * n + 2 * sites))


def plain_distances(xyz, square=False):
    """The body of jaxutil.distances before K9 (self form)."""
    import torch

    disp = xyz[:, None, :, :] - xyz[:, :, None, :]
    return (disp**2).sum(dim=-1) if square else torch.linalg.vector_norm(disp, dim=-1)


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def end_to_end(x, reps):
    """{quantity_path_ms, quantity_path_peak_gb} for fwd_bwd / double_bwd x fused / plain."""
    import torch

    from aggforce_amd import jaxutil

    def fwd_bwd(dist):
        p = x.detach().requires_grad_(True)
        torch.exp(-(dist(p) - 1) ** 2).sum().backward()
        return p.grad

    def double_bwd(dist):
        p = x.detach().requires_grad_(True)
        (g,) = torch.autograd.grad(torch.exp(-(dist(p) - 1) ** 2).sum(), p, create_graph=True)
        return torch.autograd.grad((g * g).sum(), p)[0]

    out = {}
    paths = (("fused", jaxutil.distances), ("plain", plain_distances))
    for qname, quantity in (("fwd_bwd", fwd_bwd), ("double_bwd", double_bwd)):
        times = {p: [] for p, _ in paths}
        for rep in range(reps + 1):  # (the first round warms up)
            for pname, dist in paths:
                if times[pname] is None:
                    continue
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                try:
                    ms = event_ms(lambda: quantity(dist))
                except torch.cuda.OutOfMemoryError:
                    times[pname] = None
                    out[f"{qname}_{pname}_ms"] = "out of memory"
                    continue
                out[f"{qname}_{pname}_peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
                if rep:
                    times[pname].append(ms)
        for pname, ts in times.items():
            if ts:
                out[f"{qname}_{pname}_ms"] = round(statistics.median(ts), 3)
        a, b = out.get(f"{qname}_fused_ms"), out.get(f"{qname}_plain_ms")
        if isinstance(a, float) and isinstance(b, float):
            out[f"{qname}_plain_over_fused"] = round(b / a, 2)
    out["double_bwd_fused_finite"] = bool(torch.isfinite(double_bwd(jaxutil.distances)).all())
    return out


def child(args):
    """One dispatch of every op, --reps times, cases and ops in order (the rocprofv3 run)."""
    import torch

    for name, T, m, n, dt in CASES:
        if args.cases and name not in args.cases:
            continue
        x, v, w = make(T, m, n, dt)
        calls = op_calls(x, v, w)
        torch.cuda.synchronize()
        for op in OPS:
            for _ in range(args.reps):
                calls[op]()
            torch.cuda.synchronize()
        del x, v, w, calls
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
    rows = [r for r in csv.DictReader(open(trace[0])) if "aggf::pair" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    i = 0
    for rec in recs:
        i += 1  # (op_calls computes the case's distance array first)
        for op in OPS:
            times, names = [], set()
            for _ in range(args.reps):
                r = rows[i]
                i += 1
                assert FAMILY[op] in r["Kernel_Name"], (rec["case"], op, r["Kernel_Name"])
                ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                names.add(r["Kernel_Name"].split("(")[0].replace("void ", ""))
                if i < len(rows) and "pairpull_reduce_kernel" in rows[i]["Kernel_Name"]:  # the partial row sums of B
                    names.add(rows[i]["Kernel_Name"].split("(")[0].replace("void ", ""))
                    ns += int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])
                    i += 1
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
    ap.add_argument("--rocprof-timeout", type=int, default=600)
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    import torch

    recs = []
    for name, T, m, n, dt in CASES:
        if args.cases and name not in args.cases:
            continue
        x, v, w = make(T, m, n, dt)
        rec = {"case": name, "T": T, "m": m, "n": n, "dtype": dt}
        calls = op_calls(x, v, w)
        for op in OPS:
            calls[op]()
            torch.cuda.synchronize()
            rec[op + "_ms"] = round(statistics.median(event_ms(calls[op]) for _ in range(args.reps)), 4)
            rec[op + "_timing"] = "events"
        del v, w, calls
        torch.cuda.empty_cache()
        if not args.no_end_to_end:
            rec.update(end_to_end(x, args.reps))
        recs.append(rec)
        del x
        torch.cuda.empty_cache()
    if args.rocprof:
        rocprof(args, recs)
    for rec in recs:
        s = 4 if rec["dtype"] == "f32" else 8
        for op in OPS:
            amount = op_bytes(op, rec["T"], rec["m"], rec["n"], s)
            sec = rec[op + "_ms"] * 1e-3
            rec[op + "_bytes"] = amount
            rec[op + "_tbps"] = round(amount / sec * 1e-12, 3)
            rec[op + "_peak_share"] = round(amount / sec / PEAK_BW, 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
