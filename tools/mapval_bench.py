"""Map validation (K7) on one GPU: the fused path of random_force_proj / random_residual_shift against the generic
per-sample loop (rsqpg_forces wrapped in a lambda: one force field per sample, then a device dot product).

Prints one JSON line per case.  Cases: n = 10 (CLN025's CA map) and n = 256, T frames (default 1e5), S samples
(default 1000), float32 and float64, proj and shift.
  fused_ms              the public call (offset draw, one kernel pass, slab reduction, copy back), host clock
                        around a synchronised call, best of --reps;
  generic_ms_per_sample the generic loop, timed over --generic-samples samples (the loop is linear in S);
  generic_ms_for_S      that rate times S;
  evals                 pair-sample evaluations of the fused kernel: S T n (n - 1) / 2 (proj, unordered pairs) or
                        S T n^2 (shift, ordered pairs of the per-site form);
  kernel_ms             with --rocprof: the fused kernel's time in a separate `rocprofv3 --kernel-trace --stats` run
                        of this script (--child), one dispatch per case, in case order.
--box ortho | cell: the same calls with box= (the periodic forms of the kernels): the cube the sites are drawn in, as
three lengths or as a ``pbc.Cell`` with that diagonal and a skew of a fifth of the edge; `outer` is then the smaller of
12 and half the edge, as the public functions require.  The record names the box.
Usage (GPU box): python tools/mapval_bench.py [--rocprof OUTDIR] > lines.jsonl
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(inner=6.0, outer=12.0, width=0.5)  # the reference tests' parameters


def cases(args):
    for n in args.n:
        for dt in args.dtypes:
            for kind in ("proj", "shift"):
                yield n, dt, kind


def make_data(T, n, dt, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    dtype = torch.float32 if dt == "f32" else torch.float64
    X = (edge(n) * torch.rand((T, n, 3), generator=g, device="cuda", dtype=torch.float64)).to(dtype)
    F = (30.0 * torch.randn((T, n, 3), generator=g, device="cuda", dtype=torch.float64)).to(dtype)
    return X, F


def edge(n):
    return 10.0 * (n / 10.0) ** (1.0 / 3.0)  # CLN025's CA density


def box_kwargs(args, n):
    """The keywords of one case: KW, under --box with box= and `outer` within half the edge."""
    if args.box == "none":
        return dict(KW)
    import torch

    from aggforce_amd import pbc

    L = edge(n)
    kw = dict(KW, outer=min(KW["outer"], L / 2))
    if args.box == "ortho":
        return dict(kw, box=torch.full((3,), L, dtype=torch.float64, device="cuda"))
    s = L / 5
    return dict(kw, box=pbc.Cell(torch.tensor([[L, 0, 0], [s, L, 0], [-s, s, L]], dtype=torch.float64, device="cuda")))


def evals(kind, T, n, S):
    return S * T * (n * (n - 1) // 2 if kind == "proj" else n * n)


def run(args, child=False):
    import numpy as np
    import torch

    from aggforce_amd import jaxmapval as mv
    from aggforce_amd import pbc

    out = []
    for n, dt, kind in cases(args):
        fn = mv.random_force_proj if kind == "proj" else mv.random_residual_shift
        X, F = make_data(args.T, n, dt, 1234)
        kw = box_kwargs(args, n)
        if child:  # exactly one fused dispatch per case
            fn(X, F, args.S, np.random.default_rng(0), average=False, **kw)
            torch.cuda.synchronize()
            continue
        Xw, Fw = make_data(64, n, dt, 1)
        fn(Xw, Fw, args.S, np.random.default_rng(0), **kw)  # module load, workspace
        best = float("inf")
        for r in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(X, F, args.S, np.random.default_rng(r), average=False, **kw)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)

        def generic(coords, randg=None, **kw):
            return (mv.rsqpg_forces if args.box == "none" else pbc.rsqpg_forces)(coords, randg=randg, **kw)

        sg = min(args.S, args.generic_samples)
        fn(Xw, Fw, 2, np.random.default_rng(0), method=generic, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(X, F, sg, np.random.default_rng(0), method=generic, average=False, **kw)
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / sg
        ev = evals(kind, args.T, n, args.S)
        rec = {"case": f"{kind}_n{n}_{dt}" + ("" if args.box == "none" else f"_{args.box}"), "box": args.box,
               "kind": kind, "T": args.T, "n": n, "S": args.S, "dtype": dt,
               "fused_ms": round(best * 1e3, 3), "generic_ms_per_sample": round(per * 1e3, 4),
               "generic_samples_timed": sg, "generic_ms_for_S": round(per * args.S * 1e3, 1),
               "speedup": round(per * args.S / best, 2), "evals": ev, "evals_per_s_fused": float(f"{ev / best:.4g}")}
        out.append(rec)
        del X, F
        torch.cuda.empty_cache()
    return out


def rocprof(args, recs):
    """Kernel time of every case's fused dispatch, from a separate rocprofv3 run of this script."""
    d = os.path.abspath(args.rocprof)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", "--T", str(args.T), "--S", str(args.S),
           "--n", *map(str, args.n), "--dtypes", *args.dtypes, "--box", args.box]
    with open(os.path.join(d, "child.log"), "w") as log:
        subprocess.run(cmd, check=True, stdout=log, stderr=subprocess.STDOUT, timeout=args.rocprof_timeout)
    trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(trace) == 1, trace
    rows = [r for r in csv.DictReader(open(trace[0]))
            if "gauss_proj_kernel" in r["Kernel_Name"] or "gauss_shift_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(recs), (len(rows), len(recs))
    for rec, row in zip(recs, rows):
        assert ("gauss_" + rec["kind"]) in row["Kernel_Name"], (rec["case"], row["Kernel_Name"])
        ms = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
        rec["kernel"] = row["Kernel_Name"].split("(")[0]
        rec["kernel_ms"] = round(ms, 3)
        rec["evals_per_s_kernel"] = float(f"{rec['evals'] / (ms * 1e-3):.4g}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--T", type=int, default=100_000)
    ap.add_argument("--S", type=int, default=1000)
    ap.add_argument("--n", type=int, nargs="+", default=[10, 256])
    ap.add_argument("--dtypes", nargs="+", default=["f32", "f64"], choices=["f32", "f64"])
    ap.add_argument("--box", default="none", choices=["none", "ortho", "cell"],
                    help="run under a periodic box: three lengths (ortho) or a triclinic pbc.Cell (cell)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--generic-samples", type=int, default=50)
    ap.add_argument("--rocprof", metavar="OUTDIR", help="also take kernel times from a rocprofv3 run into OUTDIR")
    ap.add_argument("--rocprof-timeout", type=int, default=900)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        run(args, child=True)
        return
    recs = run(args)
    if args.rocprof:
        rocprof(args, recs)
    for rec in recs:
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
