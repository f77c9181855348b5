"""The nearest-image forms of K9c, the K9d pull, K9e and the K7 projections beside the brick forms of the same kernels at
the same shapes, on one GPU in one run (``Cell(vectors, images="nearest")`` against ``Cell(vectors)``).

Shapes: those of ``tools/cell_bench.py`` for K9 (the triangle list at (T, n) = (1e4, 256) and (1e5, 64)) and K9e
((1e5, 256) and (1e4, 1024)), both dtypes; the K7 projection at (T, n, S) = (2000, 256, 1024).  The cell is a rhombic
dodecahedron per frame (breathing by 2 %) whose image distance is the extent of the sites, so pairs of every length the
cell has occur and the search is taken by the pairs beyond the safe radius (``searched``: their fraction).  One JSON line
per case, appended to profiles/nearest_bench.jsonl and printed:
  brick_<op>_ms / nearest_<op>_ms   median of --reps, device events around the call after --warmup calls; the two forms
                                    take turns in one loop
  <op>_nearest_over_brick           nearest_ms / brick_ms from that same loop: what the 27-candidate search costs
  *_ms_min_max                      the spread
No target is set: nobody has measured these kernels before.
Usage (GPU box): python tools/nearest_bench.py [--reps 7] [--warmup 2] [--cases K9 K9e K7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cell_bench import take_turns  # noqa: E402


def record(rec, op, times):
    for form, v in times.items():
        rec[f"{form}_{op}_ms"] = round(statistics.median(v), 4)
        rec[f"{form}_{op}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    rec[f"{op}_nearest_over_brick"] = round(rec[f"nearest_{op}_ms"] / rec[f"brick_{op}_ms"], 3)


def dodecahedra(d, T, dtype, seed):
    """(T, 9) rows on the device: the square rhombic dodecahedron of image distance d, breathing by 2 % per frame."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    s = d * (1 + 0.02 * torch.rand(T, generator=g, device="cuda", dtype=torch.float64))
    H = torch.zeros((T, 3, 3), device="cuda", dtype=torch.float64)
    H[:, 0, 0], H[:, 1, 1], H[:, 2, 2] = s, s, s * 0.5**0.5
    H[:, 2, 0], H[:, 2, 1] = s / 2, s / 2
    return H.reshape(T, 9).to(dtype).contiguous()


def searched(x, tab, cell):
    """The fraction of the pairs whose brick image is longer than the safe radius in the first frame."""
    from aggforce_amd import _kernels as K

    d = K.pair_list_dist(x[:1].contiguous(), x[:1].contiguous(), tab, box=cell[:1].contiguous())
    return round(float((d > cell[0, 8] / 2).double().mean()), 3)


def k9_rows(args, out):
    import numpy as np
    import torch

    import distgrad_bench as D
    from aggforce_amd import _kernels as K
    from aggforce_amd.jaxutil import PairList

    for name, T, _, n, dt in D.CASES:
        x, v, _ = D.make(T, 1, n, dt)
        tab = PairList(np.stack(np.triu_indices(n, 1), axis=1), n).on("cuda")
        w = torch.randn((T, tab.n_pairs), device="cuda", dtype=x.dtype)
        cell = dodecahedra(10.0, T, x.dtype, 5)
        d = K.pair_list_dist(x, x, tab, box=cell, near=True)
        rec = {"case": "nearest_triangle_" + name, "T": T, "n": n, "P": tab.n_pairs, "dtype": dt, "timing": "events",
               "reps": args.reps, "searched": searched(x, tab, cell)}
        ops = {"list_dist": lambda near: K.pair_list_dist(x, x, tab, box=cell, near=near),
               "list_pull": lambda near: K.pair_list_pull(w, x, x, tab, box=cell, near=near),
               "list_pull_dv": lambda near: K.pair_list_pull(w, x, x, tab, dv=d, box=cell, near=near)}
        for op, fn in ops.items():
            record(rec, op, take_turns({"brick": lambda: fn(False), "nearest": lambda: fn(True)}, args.warmup, args.reps))
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
            cell = dodecahedra(10.0 if n == 256 else 17.0, T, x.dtype, 6)
            rec = {"case": f"nearest_pairmin_T{T}_n{n}_{dt}", "T": T, "n": n, "dtype": dt, "timing": "events",
                   "reps": args.reps}
            record(rec, "pairmin", take_turns({"brick": lambda: K.pair_min(x, x, box=cell),
                                               "nearest": lambda: K.pair_min(x, x, box=cell, near=True)},
                                              args.warmup, args.reps))
            out(rec)
            del x
            torch.cuda.empty_cache()


def k7_rows(args, out):
    import torch

    import distgrad_bench as D
    from aggforce_amd import _kernels as K

    T, n, S = 2000, 256, 1024
    for dt in ("f32", "f64"):
        x, _, _ = D.make(T, 1, n, dt)
        f = torch.randn_like(x)
        cell = dodecahedra(10.0, T, x.dtype, 7)
        o = torch.rand(S, device="cuda", dtype=torch.float64) * 24.0 + 1.0
        rec = {"case": f"nearest_gauss_T{T}_n{n}_S{S}_{dt}", "T": T, "n": n, "S": S, "dtype": dt, "timing": "events",
               "reps": args.reps}
        record(rec, "gauss_proj", take_turns({"brick": lambda: K.gauss_proj(x, f, o, 2.0, box=cell),
                                              "nearest": lambda: K.gauss_proj(x, f, o, 2.0, box=cell, near=True)},
                                             args.warmup, args.reps))
        out(rec)
        del x, f
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", nargs="*", default=["K9", "K9e", "K7"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_bench.jsonl"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("nearest_bench.py times kernels on a GPU: none found")
    rows = []

    def out(rec):
        rows.append(rec)
        print(json.dumps(rec), flush=True)

    for name, fn in (("K9", k9_rows), ("K9e", k9e_rows), ("K7", k7_rows)):
        if name in args.cases:
            fn(args, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        for rec in rows:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
