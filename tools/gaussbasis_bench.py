"""The Gaussian radial basis (K10) on one GPU: kernel rates, and qp.jaxfeat.gaussian_dist_basis against the plain-torch
body of the same function on the same device.

Prints one JSON line per case.
  basis cases  the self-distance matrix of 1e4 frames x 256 sites (6.6e8 distances), n_basis = 10, float32 / float64:
    kernels     expand = K10a (the value), expand_q1 = K10a (first derivative), contract = K10b with H per element:
                ``<op>_ms`` (device events around the call, median of --reps), the algorithmic bytes (K10a: the output
                written and the distances read once; K10b: H and the distances read, one value per distance written)
                and their rate;
    end to end  ``fwd`` = the basis, ``fwd_bwd`` = U = sum of the basis and dU/dd, ``double_bwd`` = g = dU/dd
                (create_graph), d|g|^2/dd; ``fused`` = gaussian_dist_basis, ``plain`` = its plain-torch body.  Median
                of --reps, the two alternating in one loop; ``*_peak_gb`` = torch.cuda.max_memory_allocated of a step.
  channel case the collapsed channelised form at 2e4 frames x 1024 sites, n_basis = 8, 600 channels (BASELINE config 4,
                one cg site): K10c alone -- plain torch would need the (T, N, 4800) one-hot array.
Usage (GPU box): python tools/gaussbasis_bench.py > profiles/gaussbasis_bench.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASIS_CASES = [("n256_f32", 10000, 256, "f32"), ("n256_f64", 10000, 256, "f64")]
KW = dict(outer=8.0, inner=0.0, n_basis=10, width=1.0, dist_power=0.5, clip=1e-3)


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    return round(statistics.median(event_ms(fn) for _ in range(reps)), 4)


def sites(T, n, dtype):
    import torch

    g = torch.Generator(device="cuda").manual_seed(T + n)
    side = 1  # bench.py's recipe: a 1.5-spaced lattice with 0.3 of noise per frame
    while side**3 < n:
        side += 1
    a = torch.arange(n, device="cuda")
    lat = 1.5 * torch.stack([a % side, (a // side) % side, a // side**2], dim=1).to(dtype)
    return (lat[None] + 0.3 * torch.randn((T, n, 3), generator=g, device="cuda", dtype=dtype)).contiguous()


def end_to_end(d, reps):
    import torch

    from aggforce_amd.qp import jaxfeat

    centers = jaxfeat._grid(d.dtype, KW["outer"], KW["inner"], KW["n_basis"], KW["dist_power"])

    def fused(r):
        return jaxfeat.gaussian_dist_basis(r, **KW)

    def plain(r):
        return jaxfeat._plain_basis(r, centers, KW["width"], KW["clip"])

    def fwd(basis):
        with torch.no_grad():
            return basis(d)

    def fwd_bwd(basis):
        r = d.detach().requires_grad_(True)
        basis(r).sum().backward()
        return r.grad

    def double_bwd(basis):
        r = d.detach().requires_grad_(True)
        (g,) = torch.autograd.grad(basis(r).sum(), r, create_graph=True)
        return torch.autograd.grad((g * g).sum(), r)[0]

    out = {}
    for qname, quantity in (("fwd", fwd), ("fwd_bwd", fwd_bwd), ("double_bwd", double_bwd)):
        times = {"fused": [], "plain": []}
        for rep in range(reps + 1):  # (the first round warms up)
            for pname, basis in (("fused", fused), ("plain", plain)):
                if times[pname] is None:
                    continue
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                try:
                    ms = event_ms(lambda: quantity(basis))
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
    return out


def basis_case(name, T, n, dt, reps, with_end_to_end):
    import torch

    from aggforce_amd import _kernels as K
    from aggforce_amd.qp import jaxfeat

    dtype = torch.float32 if dt == "f32" else torch.float64
    s = 4 if dt == "f32" else 8
    x = sites(T, n, dtype)
    d = K.pair_dist(x, x, K.PAIR_DIST)
    del x
    nb = KW["n_basis"]
    spec = jaxfeat._basis_spec(d, jaxfeat._grid(dtype, KW["outer"], KW["inner"], nb, KW["dist_power"]), KW["width"], KW["clip"])
    rec = {"case": name, "T": T, "m": n, "n": n, "n_basis": nb, "dtype": dt, "timing": "events"}
    E = d.numel()
    for op, q in (("expand", 0), ("expand_q1", 1)):
        rec[op + "_ms"] = median_ms(lambda: K.gbasis_expand(d, spec, q), reps)
        rec[op + "_bytes"] = float(s * E * (nb + 1))
    h = K.gbasis_expand(d, spec, 0)
    rec["contract_ms"] = median_ms(lambda: K.gbasis_contract(h, d, spec, 0, K.GB_H_ELEM), reps)
    rec["contract_bytes"] = float(s * E * (nb + 2))
    del h
    torch.cuda.empty_cache()
    for op in ("expand", "expand_q1", "contract"):
        rec[op + "_tbps"] = round(rec[op + "_bytes"] / (rec[op + "_ms"] * 1e-3) * 1e-12, 3)
    if with_end_to_end:
        rec.update(end_to_end(d, reps))
    return rec


def channel_case(reps):
    import torch

    from aggforce_amd import _kernels as K
    from aggforce_amd.qp import jaxfeat

    T, N, nb, n_ch = 20000, 1024, 8, 600
    x = sites(T, N, torch.float32)
    d = K.pair_dist(x, x[:, :1].contiguous(), K.PAIR_DIST)[:, 0].contiguous()
    channels = tuple(a % n_ch for a in range(N))
    spec = jaxfeat._basis_spec(d, jaxfeat._grid(torch.float32, 8.0, 0.0, nb, 0.5), 1.0, 1e-3, channels, n_ch)
    rec = {"case": "c4_collapsed_f32", "T": T, "n": N, "n_basis": nb, "channels": n_ch, "dtype": "f32", "timing": "events"}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rec["sum_ms"] = median_ms(lambda: K.gbasis_sum(d, spec, 0), reps)
    rec["sum_peak_mb"] = round((torch.cuda.max_memory_allocated() - before) / 1e6, 3)
    rec["sum_bytes"] = float(4 * (T * N + n_ch * nb))
    rec["sum_exps"] = float(T * N * nb)
    rec["sum_gexp_per_s"] = round(rec["sum_exps"] / (rec["sum_ms"] * 1e-3) * 1e-9, 2)
    rec["one_hot_bytes"] = float(4 * T * N * n_ch * nb)
    table = torch.randn((n_ch, nb), device="cuda", dtype=torch.float32)
    rec["contract_slot_ms"] = median_ms(lambda: K.gbasis_contract(table, d, spec, 1, K.GB_H_SLOT), reps)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=None)
    ap.add_argument("--no-end-to-end", action="store_true")
    args = ap.parse_args()
    import torch

    for name, T, n, dt in BASIS_CASES:
        if args.cases and name not in args.cases:
            continue
        print(json.dumps(basis_case(name, T, n, dt, args.reps, not args.no_end_to_end)), flush=True)
        torch.cuda.empty_cache()
    if not args.cases or "c4_collapsed_f32" in args.cases:
        print(json.dumps(channel_case(args.reps)), flush=True)


if __name__ == "__main__":
    main()
