"""The triclinic forms of K9c / K9d, K9e, K6 and K11 beside the box forms of the same kernels, on one GPU in one run.

Shapes: those of ``tools/distgrad_bench.py --pbc`` (the triangle list at (T, n) = (1e4, 256) and (1e5, 64), K9e at
(1e5, 256) and (1e4, 1024)) and of ``tools/whole_bench.py`` ((T, N) = (1e4, 4096), chains of 300 bonds), both dtypes;
K6 at (T, N) = (1e4, 1024).  The box form runs under a box per frame, (T, 3), the triclinic form under the (T, 9) rows of
a cell per frame with the same diagonal and skews of a third of it: both read their cell once per frame.  One JSON line
per case, appended to profiles/cell_bench.jsonl and printed:
  box_<op>_ms / cell_<op>_ms     median of --reps, device events around the call after --warmup calls; the two forms
                                 take turns in one loop
  <op>_cell_over_box             cell_ms / box_ms from that same loop: what the triclinic form costs
  *_ms_min_max                   the spread
No target is set: nobody has measured these kernels before.
Usage (GPU box): python tools/cell_bench.py [--reps 7] [--warmup 2] [--cases K9 K9e K6 K11]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def take_turns(calls, warmup, reps):
    """{name: the times in ms} of several calls measured in turn, one after the other in every repeat."""
    times = {k: [] for k in calls}
    for rep in range(warmup + reps):
        for k, fn in calls.items():
            ms = event_ms(fn)
            if rep >= warmup:
                times[k].append(ms)
    return times


def record(rec, op, times):
    for form, v in times.items():
        rec[f"{form}_{op}_ms"] = round(statistics.median(v), 4)
        rec[f"{form}_{op}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    rec[f"{op}_cell_over_box"] = round(rec[f"cell_{op}_ms"] / rec[f"box_{op}_ms"], 3)


def frame_cells(lengths, T, dtype, seed):
    """((T, 3) box lengths, (T, 9) cell rows with the same diagonal) on the device, varying by 2 % per frame."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    L = torch.tensor(lengths, device="cuda", dtype=torch.float64)[None] * (
        1 + 0.02 * torch.rand((T, 3), generator=g, device="cuda", dtype=torch.float64))
    H = torch.zeros((T, 3, 3), device="cuda", dtype=torch.float64)
    H[:, 0, 0], H[:, 1, 1], H[:, 2, 2] = L[:, 0], L[:, 1], L[:, 2]
    H[:, 1, 0], H[:, 2, 0], H[:, 2, 1] = L[:, 0] / 3, -L[:, 0] / 3, L[:, 1] / 3
    return L.to(dtype).contiguous(), H.reshape(T, 9).to(dtype).contiguous()


def k9_rows(args, out):
    import numpy as np
    import torch

    import distgrad_bench as D
    from aggforce_amd import _kernels as K
    from aggforce_amd.jaxutil import PairList

    lengths = (9.1, 10.3, 11.7)  # (distgrad_bench --pbc: the lattice spans about 10, most pairs wrap in some component)
    for name, T, _, n, dt in D.CASES:
        x, v, _ = D.make(T, 1, n, dt)
        tab = PairList(np.stack(np.triu_indices(n, 1), axis=1), n).on("cuda")
        w = torch.randn((T, tab.n_pairs), device="cuda", dtype=x.dtype)
        box, cell = frame_cells(lengths, T, x.dtype, 5)
        d = K.pair_list_dist(x, x, tab, box=box)
        rec = {"case": "cell_triangle_" + name, "T": T, "n": n, "P": tab.n_pairs, "dtype": dt, "timing": "events",
               "reps": args.reps}
        ops = {"list_dist": lambda b: K.pair_list_dist(x, x, tab, box=b),
               "list_dot": lambda b: K.pair_list_dist(x, x, tab, K.PAIR_DOT, v, v, box=b),
               "list_pull": lambda b: K.pair_list_pull(w, x, x, tab, box=b),
               "list_pull_dv": lambda b: K.pair_list_pull(w, x, x, tab, dv=d, box=b)}
        for op, fn in ops.items():
            record(rec, op, take_turns({"box": lambda: fn(box), "cell": lambda: fn(cell)}, args.warmup, args.reps))
        out(rec)
        del x, v, w, d
        torch.cuda.empty_cache()


def k9e_rows(args, out):
    import torch

    import distgrad_bench as D
    from aggforce_amd import _kernels as K

    for T, n in ((100000, 256), (10000, 1024)):
        for dt in ("f32", "f64"):
            x, _, _ = D.make(T, 1, n, dt)
            box, cell = frame_cells((9.1, 10.3, 11.7) if n == 256 else (16.1, 17.3, 18.7), T, x.dtype, 6)
            rec = {"case": f"cell_pairmin_T{T}_n{n}_{dt}", "T": T, "n": n, "dtype": dt, "timing": "events", "reps": args.reps}
            record(rec, "pairmin", take_turns({"box": lambda: K.pair_min(x, x, box=box),
                                               "cell": lambda: K.pair_min(x, x, box=cell)}, args.warmup, args.reps))
            out(rec)
            del x
            torch.cuda.empty_cache()


def k6_rows(args, out):
    import torch

    import distgrad_bench as D
    from aggforce_amd import _kernels as K

    T, N = 10000, 1024
    for dt in ("f32", "f64"):
        x, _, _ = D.make(T, 1, N, dt)
        box, cell = frame_cells((16.1, 17.3, 18.7), T, x.dtype, 7)
        rec = {"case": f"cell_pairvar_T{T}_N{N}_{dt}", "T": T, "N": N, "dtype": dt, "timing": "events", "reps": args.reps}
        record(rec, "pair_dist_var", take_turns({"box": lambda: K.pair_dist_var(x, box=box),
                                                 "cell": lambda: K.pair_dist_var(x, box=cell)}, args.warmup, args.reps))
        out(rec)
        del x
        torch.cuda.empty_cache()


def k11_rows(args, out):
    import numpy as np
    import torch

    import whole_bench as W
    from aggforce_amd import MoleculeTree
    from aggforce_amd import _kernels as K

    T, N = 10000, 4096
    for dt, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        par = W.forest("chain", N)
        tree = MoleculeTree(par)
        tab = tree.on("cuda")
        level = tree.level
        levels = [(torch.as_tensor(np.flatnonzero(level == d), device="cuda"),
                   torch.as_tensor(par[level == d], device="cuda")) for d in range(1, tree.depth + 1)]
        x, box = W.wrapped_walk(par, levels, T, dtype, 17 + N)
        cell = torch.zeros((T, 3, 3), device="cuda", dtype=dtype)
        cell[:, 0, 0], cell[:, 1, 1], cell[:, 2, 2] = box[:, 0], box[:, 1], box[:, 2]
        cell[:, 1, 0], cell[:, 2, 0], cell[:, 2, 1] = box[:, 0] / 3, -box[:, 0] / 3, box[:, 1] / 3
        cell = cell.reshape(T, 9).contiguous()
        outbuf = torch.empty_like(x)
        rec = {"case": f"cell_whole_T{T}_N{N}_{dt}_chain", "T": T, "N": N, "dtype": dt, "depth": tree.depth,
               "rounds": tree.n_rounds, "timing": "events", "reps": args.reps}
        for op, form in (("whole_lds", K.WHOLE_LDS), ("whole_global", K.WHOLE_GLOBAL)):
            record(rec, op, take_turns({"box": lambda: K.make_whole(x, box, tab, out=outbuf, _form=form),
                                        "cell": lambda: K.make_whole(x, cell, tab, out=outbuf, _form=form)},
                                       args.warmup, args.reps))
        out(rec)
        del x, outbuf
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", nargs="*", default=["K9", "K9e", "K6", "K11"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cell_bench.jsonl"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("cell_bench.py times kernels on a GPU: none found")
    rows = []

    def out(rec):
        rows.append(rec)
        print(json.dumps(rec), flush=True)

    for name, fn in (("K9", k9_rows), ("K9e", k9e_rows), ("K6", k6_rows), ("K11", k11_rows)):
        if name in args.cases:
            fn(args, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        for rec in rows:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
