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
With --pairlist the rows of the pair-list kernels instead (K9c / K9d, device events, median of --reps):
  triangle_*   the list triu_indices at the four cases: list_dist / list_dot (K9c), list_pull / list_pull_dv (K9d),
               with ``matrix_*`` = K9a / K9b on the (T, n, n) matrix of the same sites in the same run; and the upper
               triangles end to end, U = sum exp(-(d - 1)^2) over i < j: ``list`` = jaxutil.distances(x,
               return_matrix=False), ``matrix`` = the route of the commit --parent (the matrix, then a gather) rebuilt
               in the same process, the two alternating; ``*_matrix_ms_min_max`` = the spread of the matrix route's repeats
  bonded_*     a 256-site chain with its 1-3 and 1-4 neighbours (762 pairs), 1e4 frames
  form_sweep_* K9d's lane-per-site and wave-per-site forms on lists of 2 .. 128 entries per site (PLP_LANE_DEG)
With --pbc the rows of the periodic-box kernels (device events, median of --reps):
  pbc_triangle_*  K9c / K9d on the triangle list at (1e4, 256) and (1e5, 64), both dtypes, under a constant box
               (``box_*_ms``) and a per-frame box (``frames_*_ms``), each beside its open form (``open_*_ms``) measured
               in the same process, alternating; ``*_box_over_open`` = open time / box time (1 = parity)
  pairmin_*    K9e at (T, n) = (1e5, 256) and (1e4, 1024), open and under a box: ms and (frame, pair) evaluations per
               second (T n^2 / time)
Usage (GPU box): python tools/distgrad_bench.py [--rocprof OUTDIR] > profiles/distgrad_bench.jsonl
                 python tools/distgrad_bench.py --pairlist --parent HASH >> profiles/distgrad_bench.jsonl
                 python tools/distgrad_bench.py --pbc >> profiles/distgrad_bench.jsonl
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


# ------------------------------------------------------------------ pair lists (K9c / K9d): --pairlist
def bonded_list(n):
    """A chain with its 1-3 and 1-4 neighbours: (i, i + k), k = 1, 2, 3 (up to 3 entries per site and table)."""
    import numpy as np

    return np.concatenate([np.stack([np.arange(n - k), np.arange(k, n)], axis=1) for k in (1, 2, 3)])


def ring_list(n, deg):
    """Every site with its next ``deg`` sites around a ring: ``deg`` entries per site in both tables."""
    import numpy as np

    s = np.arange(n)
    return np.concatenate([np.stack([s, (s + k) % n], axis=1) for k in range(1, deg + 1)])


def median_ms(fn, reps):
    fn()
    return round(statistics.median(event_ms(fn) for _ in range(reps)), 4)


def list_kernel_row(name, kind, pairs, T, n, dt, reps, matrix=True):
    """K9c / K9d on one list, beside K9a / K9b on the (T, n, n) matrix of the same sites in the same run."""
    import torch

    from aggforce_amd import _kernels as K
    from aggforce_amd.jaxutil import PairList

    s = 4 if dt == "f32" else 8
    x, v, _ = make(T, 1, n, dt)
    pl = PairList(pairs, n)
    tab, P = pl.on("cuda"), pl.n_pairs
    w = torch.randn((T, P), device="cuda", dtype=x.dtype)
    d = K.pair_list_dist(x, x, tab)
    rec = {"case": name, "list": kind, "T": T, "n": n, "P": P, "dtype": dt, "timing": "events",
           "max_degree": [pl.tables()[0][2], pl.tables()[1][2]]}
    calls = {"list_dist": lambda: K.pair_list_dist(x, x, tab), "list_dot": lambda: K.pair_list_dist(x, x, tab, K.PAIR_DOT, v, v),
             "list_pull": lambda: K.pair_list_pull(w, x, x, tab), "list_pull_dv": lambda: K.pair_list_pull(w, x, x, tab, dv=d)}
    sites = 3 * 2 * n
    amount = {"list_dist": s * T * (P + sites), "list_dot": s * T * (P + 2 * sites), "list_pull": s * T * (P + 2 * sites),
              "list_pull_dv": s * T * (2 * P + 2 * sites)}
    for op, fn in calls.items():
        rec[op + "_ms"] = median_ms(fn, reps)
        rec[op + "_bytes"] = float(amount[op])
        rec[op + "_tbps"] = round(amount[op] / (rec[op + "_ms"] * 1e-3) * 1e-12, 3)
    del w, d, calls
    torch.cuda.empty_cache()
    if matrix:
        wm = torch.randn((T, n, n), device="cuda", dtype=x.dtype)
        for op, fn in op_calls(x, v, wm).items():
            rec["matrix_" + op + "_ms"] = median_ms(fn, reps)
            rec["matrix_" + op + "_tbps"] = round(op_bytes(op, T, n, n, s) / (rec["matrix_" + op + "_ms"] * 1e-3) * 1e-12, 3)
        del wm
    torch.cuda.empty_cache()
    return rec, x


def triangle_end_to_end(x, reps, parent):
    """fwd_bwd and double_bwd of the upper triangles: ``list`` = jaxutil.distances(x, return_matrix=False) as it is,
    ``matrix`` = the route of commit ``parent`` rebuilt from its pieces (the (T, n, n) matrix on K9a, then a gather),
    alternating in one loop; the spread of the matrix route's own repeats is kept beside the medians."""
    import torch

    from aggforce_amd import jaxutil
    from aggforce_amd._autograd import PairDist

    def matrix_route(p):
        return jaxutil._upper_triangles(PairDist.apply(p, p, False))

    def list_route(p):
        return jaxutil.distances(p, return_matrix=False)

    def fwd_bwd(dist):
        p = x.detach().requires_grad_(True)
        torch.exp(-(dist(p) - 1) ** 2).sum().backward()
        return p.grad

    def double_bwd(dist):
        p = x.detach().requires_grad_(True)
        (g,) = torch.autograd.grad(torch.exp(-(dist(p) - 1) ** 2).sum(), p, create_graph=True)
        return torch.autograd.grad((g * g).sum(), p)[0]

    out = {"parent": parent, "parent_route": "rebuilt in this process: _upper_triangles(PairDist.apply(x, x))"}
    paths = (("list", list_route), ("matrix", matrix_route))
    for qname, quantity in (("fwd_bwd", fwd_bwd), ("double_bwd", double_bwd)):
        times = {p: [] for p, _ in paths}
        for rep in range(reps + 1):  # (the first round warms up)
            for pname, dist in paths:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                ms = event_ms(lambda: quantity(dist))
                out[f"{qname}_{pname}_peak_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
                if rep:
                    times[pname].append(ms)
        for pname, ts in times.items():
            out[f"{qname}_{pname}_ms"] = round(statistics.median(ts), 3)
        out[f"{qname}_matrix_ms_min_max"] = [round(min(times["matrix"]), 3), round(max(times["matrix"]), 3)]
        out[f"{qname}_matrix_over_list"] = round(out[f"{qname}_matrix_ms"] / out[f"{qname}_list_ms"], 2)
    out["double_bwd_list_finite"] = bool(torch.isfinite(double_bwd(list_route)).all())
    return out


def form_sweep(T, n, dt, reps):
    """K9d's two forms on ring lists of growing degree, the form forced through the degree handed to the C entry
    point (which only chooses the form): where the wave per site overtakes the lane per site."""
    import torch

    from aggforce_amd import _kernels as K
    from aggforce_amd.jaxutil import PairList

    x, _, _ = make(T, 1, n, dt)
    rec = {"case": f"form_sweep_n{n}_{dt}", "T": T, "n": n, "dtype": dt, "timing": "events", "degree": [], "lane_ms": [],
           "wave_ms": []}
    for deg in (2, 4, 8, 16, 24, 32, 48, 64, 128):
        real = PairList(ring_list(n, deg), n).on("cuda")
        w = torch.randn((T, real.n_pairs), device="cuda", dtype=x.dtype)
        rec["degree"].append(deg)
        for form, fake in (("lane", 0), ("wave", 1 << 30)):
            tab = K.PairTables(real.pairs, real.a_ptr, real.a_idx, real.b_ptr, real.b_idx, fake, fake, n, n)
            rec[form + "_ms"].append(median_ms(lambda: K.pair_list_pull(w, x, x, tab), reps))
        del w
    return rec


def pairlist_rows(args):
    import numpy as np
    import torch

    for name, T, _, n, dt in CASES:
        if args.cases and name not in args.cases:
            continue
        rec, x = list_kernel_row("triangle_" + name, "triangle", np.stack(np.triu_indices(n, 1), axis=1), T, n, dt, args.reps)
        if not args.no_end_to_end:
            rec.update(triangle_end_to_end(x, args.reps, args.parent))
        print(json.dumps(rec), flush=True)
        del x
        torch.cuda.empty_cache()
    for dt in ("f32", "f64"):
        rec, _ = list_kernel_row("bonded_n256_" + dt, "chain + 1-3 + 1-4", bonded_list(256), 10000, 256, dt, args.reps,
                                 matrix=False)
        print(json.dumps(rec), flush=True)
        print(json.dumps(form_sweep(10000, 256, dt, args.reps)), flush=True)


# ------------------------------------------------------------------ periodic boxes (K9c / K9d box forms, K9e): --pbc
def alternating_ms(calls, reps):
    """{name: median ms} of several calls measured in turn, one after the other in every repeat."""
    for fn in calls.values():
        fn()
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            times[k].append(event_ms(fn))
    return {k: round(statistics.median(v), 4) for k, v in times.items()}


def pbc_rows(args):
    import numpy as np
    import torch

    from aggforce_amd import _kernels as K
    from aggforce_amd.jaxutil import PairList

    lengths = (9.1, 10.3, 11.7)  # (the lattice of `make` spans about 10: most pairs wrap in some component)
    for name, T, _, n, dt in CASES:
        if args.cases and name not in args.cases:
            continue
        x, v, _ = make(T, 1, n, dt)
        tab = PairList(np.stack(np.triu_indices(n, 1), axis=1), n).on("cuda")
        P = tab.n_pairs
        w = torch.randn((T, P), device="cuda", dtype=x.dtype)
        box = torch.tensor(lengths, device="cuda", dtype=x.dtype)
        boxes = (box[None] * (1 + 0.02 * torch.rand((T, 3), device="cuda", dtype=x.dtype))).contiguous()
        d = K.pair_list_dist(x, x, tab, box=box)
        rec = {"case": "pbc_triangle_" + name, "T": T, "n": n, "P": P, "dtype": dt, "timing": "events", "box": lengths}
        ops = {"list_dist": lambda **k: K.pair_list_dist(x, x, tab, **k),
               "list_dot": lambda **k: K.pair_list_dist(x, x, tab, K.PAIR_DOT, v, v, **k),
               "list_pull": lambda **k: K.pair_list_pull(w, x, x, tab, **k),
               "list_pull_dv": lambda **k: K.pair_list_pull(w, x, x, tab, dv=d, **k)}
        for op, fn in ops.items():
            ms = alternating_ms({"open": fn, "box": lambda: fn(box=box), "frames": lambda: fn(box=boxes)}, args.reps)
            for form, t in ms.items():
                rec[f"{form}_{op}_ms"] = t
            rec[f"{op}_box_over_open"] = round(ms["open"] / ms["box"], 3)
            rec[f"{op}_frames_over_open"] = round(ms["open"] / ms["frames"], 3)
        print(json.dumps(rec), flush=True)
        del x, v, w, d, boxes
        torch.cuda.empty_cache()
    for T, n in ((100000, 256), (10000, 1024)):
        for dt in ("f32", "f64"):
            x, _, _ = make(T, 1, n, dt)
            box = torch.tensor(lengths if n == 256 else (16.1, 17.3, 18.7), device="cuda", dtype=x.dtype)
            ms = alternating_ms({"open": lambda: K.pair_min(x, x), "box": lambda: K.pair_min(x, x, box=box)}, args.reps)
            rec = {"case": f"pairmin_T{T}_n{n}_{dt}", "T": T, "n": n, "dtype": dt, "timing": "events"}
            for form, t in ms.items():
                rec[f"{form}_ms"] = t
                rec[f"{form}_evals_per_s"] = float(f"{T * n * n / (t * 1e-3):.4g}")
            print(json.dumps(rec), flush=True)
            del x
            torch.cuda.empty_cache()


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
    ap.add_argument("--pairlist", action="store_true", help="the K9c / K9d rows instead (device events)")
    ap.add_argument("--pbc", action="store_true", help="the periodic-box rows instead (K9c / K9d box forms, K9e)")
    ap.add_argument("--parent", default="", help="8-character hash of the commit whose triangle route is compared")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    if args.pairlist:
        pairlist_rows(args)
        return
    if args.pbc:
        pbc_rows(args)
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
