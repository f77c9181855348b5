"""make_whole (K11) on one GPU: both forms of the kernel, in place and out of place, beside a level-by-level torch body
of the same operation, in the same run on the same device.

Shapes: (T, N) = (1e4, 4096) in float32 and float64, for a chain-like forest (chains of 300 bonds laid end to end:
depth 300, 9 rounds of pointer jumping) and for a star (depth 1, no rounds), molecules longer than the cell wrapped into
it, a box per frame.  One JSON line per (dtype, forest), appended to profiles/whole_bench.jsonl and printed:
  lds_ms / lds_inplace_ms          the LDS form (the library's choice at this N), out of place and in place
  global_ms / global_inplace_ms    the global form (forced), its count buffers within the wrapper's 256 MiB cap
  torch_ms                         the torch body: per level of the forest, gather parents, wrap, scatter (out of place:
                                   one clone, then in place level by level)
  *_gbs                            (bytes read + bytes written) / time with the coordinates counted once each way:
                                   2 T N 3 s bytes, in GB/s
Device events around the Python call after ``--warmup`` calls, median of ``--reps``; the forms take turns in one loop.
The outputs of all forms are compared before anything is timed (the kernels bit for bit, the torch body to 1e-5 / 1e-12
relative: it rounds differently).
Usage (GPU box): python tools/whole_bench.py [--frames 10000] [--sites 4096] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def forest(kind, n):
    import numpy as np

    if kind == "star":
        par = np.zeros(n, dtype=np.int64)
        par[0] = -1
        return par
    par = np.arange(-1, n - 1)
    par[::301] = -1  # chains of 300 bonds
    return par


def wrapped_walk(par, levels, T, dtype, seed):
    """(x, box) on the device: every atom a step of at most 0.44 box lengths per component from its parent, wrapped."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    box = torch.tensor([4.1, 5.3, 6.7], device="cuda", dtype=torch.float64) * (
        1 + 0.03 * (2 * torch.rand((T, 3), generator=g, device="cuda", dtype=torch.float64) - 1))
    L = box[:, None, :]
    n = len(par)
    x = L * torch.rand((T, n, 3), generator=g, device="cuda", dtype=torch.float64)
    step = 0.44 * L * (2 * torch.rand((T, n, 3), generator=g, device="cuda", dtype=torch.float64) - 1)
    for idx, pidx in levels:
        x[:, idx] = x[:, pidx] + step[:, idx]
    del step
    x -= L * torch.floor(x / L)
    return x.to(dtype).contiguous(), box.to(dtype).contiguous()


def torch_body(x, box, levels, out=None):
    """The sequential unwrap, a level of the forest at a time."""
    import torch

    u = x.clone() if out is None else out
    L = box[:, None, :]
    for idx, pidx in levels:
        d = u[:, idx] - u[:, pidx]
        u[:, idx] = u[:, pidx] + (d - L * torch.round(d / L))
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--sites", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whole_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch

    from aggforce_amd import MoleculeTree
    from aggforce_amd import _kernels as K

    T, N = args.frames, args.sites
    rows = []
    for dt, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        for kind in ("chain", "star"):
            par = forest(kind, N)
            tree = MoleculeTree(par)
            tab = tree.on("cuda")
            level = tree.level
            levels = [(torch.as_tensor(np.flatnonzero(level == d), device="cuda"),
                       torch.as_tensor(par[level == d], device="cuda")) for d in range(1, tree.depth + 1)]
            x, box = wrapped_walk(par, levels, T, dtype, 17 + N)
            out = torch.empty_like(x)
            work = x.clone()
            forms = {
                "lds": lambda: K.make_whole(x, box, tab, out=out, _form=K.WHOLE_LDS),
                "lds_inplace": lambda: K.make_whole(work, box, tab, out=work, _form=K.WHOLE_LDS),
                "global": lambda: K.make_whole(x, box, tab, out=out, _form=K.WHOLE_GLOBAL),
                "global_inplace": lambda: K.make_whole(work, box, tab, out=work, _form=K.WHOLE_GLOBAL),
                "torch": lambda: torch_body(x, box, levels),
            }
            # the forms agree (an in-place call on its own output changes nothing: timing it repeatedly is sound)
            ref = K.make_whole(x, box, tab, _form=K.WHOLE_LDS)
            assert torch.equal(K.make_whole(x, box, tab, _form=K.WHOLE_GLOBAL), ref)
            work.copy_(x)
            forms["lds_inplace"]()
            assert torch.equal(work, ref)
            forms["global_inplace"]()
            assert torch.equal(work, ref)
            tb = torch_body(x, box, levels)
            tol = 1e-5 if dtype == torch.float32 else 1e-12
            assert float((tb - ref).abs().max()) <= tol * float(ref.abs().max()), "the torch body disagrees"
            del tb
            times = {k: [] for k in forms}
            for rep in range(args.warmup + args.reps):
                for k, fn in forms.items():
                    ms = event_ms(fn)
                    if rep >= args.warmup:
                        times[k].append(ms)
            nbytes = 2.0 * T * N * 3 * x.element_size()
            rec = {"case": f"whole_T{T}_N{N}_{dt}_{kind}", "T": T, "N": N, "dtype": dt, "forest": kind,
                   "depth": tree.depth, "rounds": tree.n_rounds, "timing": "events", "reps": args.reps,
                   "bytes": nbytes}
            for k, v in times.items():
                ms = statistics.median(v)
                rec[f"{k}_ms"] = round(ms, 4)
                rec[f"{k}_gbs"] = round(nbytes / ms / 1e6, 1)
                rec[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
            rec["torch_over_lds"] = round(rec["torch_ms"] / rec["lds_ms"], 2)
            rows.append(rec)
            print(json.dumps(rec), flush=True)
            del x, out, work, ref
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as fh:
        for rec in rows:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
