"""The box forms of the K4 kernels beside the open ones, at BASELINE config 4's shape, in one run on one device.

Geometry, constraints, coordinate map and basis are bench.py's c4 workload (20000 frames x 1024 atoms x 64 sites,
float32, id_feat + gb_feat with n_basis 8 and outer 8.0); the kept Gaussian columns are those of the OPEN fused fit and
are used for both forms, with random coefficients on them, so that both do the same number of expf and the difference
is the wrap: three v_rndne + fma per distance, and the box lengths read once per frame.  The cell is the lattice's own
extent, (3,) and one row per frame (lengths varied by 1 %).

One JSON line per kernel, appended to profiles/featpbc_bench.jsonl and printed:
  open_ms / box3_ms / boxT3_ms    device events around the Python call(s) after --warmup calls, median of --reps, the
                                  three forms taking turns in one loop; gb_regmat_cols: all 64 sites, one after the other
  box3_over_open, boxT3_over_open
  --box cell | nearest            the cell forms instead of boxT3: a reduced skewed cell on the same extent (bx = Lx / 4,
                                  cx = -Lx / 5, cy = 3 Ly / 10; half its shortest diagonal entry is about the basis's
                                  outer, so under "nearest" most distances go through the 27-candidate search), as
                                  (T, 9) rows, beside open and box3 in the same loop: cell_ms / nearest_ms,
                                  *_over_box3, *_over_open, and parent_box3_ms, the box3 figure of the last line of this
                                  case that the parent commit left in the jsonl
Usage (GPU box): python tools/featpbc_bench.py [--frames 20000] [--reps 7] [--box box|cell|nearest]
  --bench-lines FILE LABEL        instead: append the JSON result lines of bench.py runs kept in FILE (one per line)
                                  to the same jsonl under "case": LABEL, so that the c4 figures of this commit and of
                                  its parent stand beside the kernels'
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "featpbc_bench.jsonl")


def emit(rec):
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as fh:
        fh.write(line + "\n")


def previous_lines():
    if not os.path.exists(OUT):
        return []
    return [json.loads(line) for line in open(OUT) if line.strip().startswith("{")]


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench_lines(path, label):
    for line in open(path):
        line = line.strip()
        if not line.startswith("{"):
            continue
        r = json.loads(line)
        emit({"case": label, "ms_per_step": r["ms_per_step"], "steps": r["steps"], "warmup": r["warmup"],
              "stage_ms_per_step": r.get("config", {}).get("stage_ms_per_step"), "residual": r.get("config", {}).get("residual")})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=20000)
    p.add_argument("--sites", type=int, default=1024)
    p.add_argument("--cg", type=int, default=64)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--box", choices=["box", "cell", "nearest"], default="box")
    p.add_argument("--bench-lines", nargs=2, metavar=("FILE", "LABEL"))
    args = p.parse_args()
    if args.bench_lines:
        return bench_lines(*args.bench_lines)

    import numpy as np
    import torch

    from aggforce_amd import LinearMap
    from aggforce_amd import _kernels as K
    from aggforce_amd.qp import gbfeat

    T, N, n_cg = args.frames, args.sites, args.cg
    torch.cuda.set_device(0)
    forces = K.synth_normal(T, N, torch.float32, 1234, sigma=30.0)
    coords = K.synth_normal(T, N, torch.float32, 1235, sigma=0.3, lattice=1.5)
    cons = {frozenset([3 * i, 3 * i + 1]) for i in range(N // 3)}
    cmap = LinearMap([[3 * (i * (N // n_cg) // 3)] for i in range(n_cg)], n_fg_sites=N)
    su = gbfeat._fused_setup(coords, forces, cmap, cons, True, dict(outer=8.0, inner=0.0, n_basis=8, width=1.0), None)
    geo = su.geo
    extent = (coords.amax(dim=(0, 1)) - coords.amin(dim=(0, 1))).to(torch.float32) + 1.5
    g = torch.Generator(device="cuda").manual_seed(7)
    boxes = {"open": None, "box3": extent.contiguous(),
             "boxT3": (extent[None, :] * (1 + 0.01 * (2 * torch.rand((T, 3), generator=g, device="cuda") - 1))).contiguous()}
    near = {k: False for k in boxes}
    if args.box != "box":
        Lx, Ly, Lz = (float(x) for x in extent.tolist())
        H = torch.tensor([Lx, 0, 0, Lx / 4, Ly, 0, -Lx / 5, 0.3 * Ly, Lz], dtype=torch.float32, device="cuda")
        del boxes["boxT3"]
        boxes[args.box] = H[None, :].expand(T, 9).contiguous()
        near[args.box] = args.box == "nearest"
    rng = np.random.default_rng(5)
    coef_h = np.zeros((n_cg, su.n_feat))
    for site, cols in enumerate(su.cols_of):
        coef_h[site, :su.n_id] = rng.standard_normal(su.n_id)
        coef_h[site, su.n_id + cols] = rng.standard_normal(len(cols))
    coef = torch.from_numpy(coef_h).cuda()
    compact = K.gb_compact_coefficients(coef_h, su.n_id, geo.dev)
    cols_dev = [torch.from_numpy(c).cuda() for c in su.cols_of]
    ld = -(-max(su.n_act) // 128) * 128
    R3 = torch.zeros((T, ld, 3), dtype=torch.float64, device="cuda")

    def regmat(box, nr):
        for site in range(n_cg):
            K.gb_regmat_cols(su.Fg, geo.Pg, geo.cg, site, geo.sizes, su.n_id, cols_dev[site], su.centers, su.width,
                             gbfeat.CLIP, 0.6955215, R3, box=box, near=nr)

    kernels = {
        "gb_apply": lambda box, nr: K.gb_apply(su.Fg, geo.Pg, geo.cg, geo.sizes, su.n_id, su.n_ch, su.centers, su.width,
                                               gbfeat.CLIP, coef, box=box, near=nr),
        "gb_apply_cols": lambda box, nr: K.gb_apply_cols(su.Fg, geo.Pg, geo.cg, geo.sizes, su.n_id, su.centers, su.width,
                                                         gbfeat.CLIP, compact, box=box, near=nr),
        "gb_regmat_cols": regmat,
    }
    for name, fn in kernels.items():
        case = f"featpbc_{name}_T{T}_N{N}_cg{n_cg}"
        times = {k: [] for k in boxes}
        for rep in range(args.warmup + args.reps):
            for form, box in boxes.items():
                ms = event_ms(lambda: fn(box, near[form]))
                if rep >= args.warmup:
                    times[form].append(ms)
        med = {k: statistics.median(v) for k, v in times.items()}
        rec = {"case": case, "kernel": name, "T": T, "N": N, "n_cg": n_cg, "n_basis": 8,
               "kept_columns_mean": float(np.mean(su.n_act)), "n_feat": su.n_feat, "timing": "events", "reps": args.reps,
               "box": [round(float(x), 3) for x in extent.tolist()],
               **{f"{k}_ms": round(v, 4) for k, v in med.items()},
               **{f"{k}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
               "box3_over_open": round(med["box3"] / med["open"], 4)}
        if args.box == "box":
            rec["boxT3_over_open"] = round(med["boxT3"] / med["open"], 4)
        else:
            form = args.box
            rec.update({"form": form, "cell": [round(float(x), 3) for x in boxes[form][0].tolist()],
                        f"{form}_over_box3": round(med[form] / med["box3"], 4),
                        f"{form}_over_open": round(med[form] / med["open"], 4)})
            parent = [r for r in previous_lines() if r.get("case") == case and "form" not in r and "box3_ms" in r]
            if parent:
                rec["parent_box3_ms"] = parent[-1]["box3_ms"]
                rec[f"{form}_over_parent_box3"] = round(med[form] / parent[-1]["box3_ms"], 4)
                rec["box3_over_parent_box3"] = round(med["box3"] / parent[-1]["box3_ms"], 4)
        emit(rec)


if __name__ == "__main__":
    main()
