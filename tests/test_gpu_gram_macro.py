"""The macro-tile Gram kernel (gram_tile_dma_kernel_x2: 16 waves, two 128x128 tiles that share a panel per workgroup):
float64 frames read in place in whole panels, from `macro_min_tiles` tile rows on (profiles/r05_routing.json).  Row
pairs with three and with two panels, the two-panel pairs of leftover diagonal tiles, the lone leftover tile, ragged and
very short frame ranges, accumulation, the planner's workspace -- against an independent contraction and against the
single-tile kernel forced on the same frames (AGGF_GRAM_ROUTE=single)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from aggforce_amd import _kernels as K  # noqa: E402
from aggforce_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_TILES = json.load(open(os.path.join(ROOT, "profiles", "r05_routing.json")))["thresholds"]["macro_min_tiles"]["value"]
SINGLE = "gram_tile_dma_kernel<double, 0, 3, 2, 8, true, 1, true, false, false, double>"
F64 = torch.float64


def ran(family="gram_tile_dma_kernel"):
    return sorted(n.split("(")[0].replace("void ", "").replace("aggf::", "") for n, c in _lib.coverage(names=True).values()
                  if c > 0 and family in n)


def gram_on(f, route=None, **kw):
    """(G, the tile kernels that ran); route = a value of the AGGF_GRAM_ROUTE measurement hook"""
    old = os.environ.pop("AGGF_GRAM_ROUTE", None)
    if route:
        os.environ["AGGF_GRAM_ROUTE"] = route
    try:
        _lib.load().aggf_coverage_reset()
        g = K.gram(f, None, None, f.shape[1], F64, **kw)
        torch.cuda.synchronize()
        return g, ran()
    finally:
        os.environ.pop("AGGF_GRAM_ROUTE", None)
        if old is not None:
            os.environ["AGGF_GRAM_ROUTE"] = old


def is_macro(kernels):
    return len(kernels) == 1 and kernels[0].startswith("gram_tile_dma_kernel_x2<")


def contraction(f):
    T, N, _ = f.shape
    F2 = f.permute(0, 2, 1).reshape(3 * T, N)
    return F2.T @ F2


def rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


def check_against_both(f):
    g, k = gram_on(f)
    assert is_macro(k), k
    assert torch.equal(g, g.T)
    g1, k1 = gram_on(f, "single")
    assert k1 == [SINGLE], k1
    scale = float(g1.abs().max())
    assert float((g - g1).abs().max()) < 1e-13 * scale
    assert rel(g, contraction(f)) < 1e-12
    return g


def test_macro_tiles_at_the_flagship_row_length():
    """4096 atoms (32 tile rows: 240 row pairs with three panels, 16 with two, 8 pairs of leftover diagonal tiles), 3001
    frames: many splits and a ragged last stage."""
    assert MIN_TILES <= 32
    f = K.synth_normal(3001, 4096, F64, seed=9101, sigma=30.0)
    g = check_against_both(f)
    g2, _ = gram_on(f)
    assert torch.equal(g, g2)  # bit reproducible
    assert ran("build_macro_table_kernel") == ["build_macro_table_kernel"] and not ran("build_tile_table_kernel")


@pytest.mark.parametrize("N", [3968, 4352])
def test_leftover_diagonal_tiles_in_pairs_and_alone(N):
    """31 tile rows leave 16 diagonal tiles over: eight two-panel macro-tiles.  34 leave 17: the last one runs alone."""
    assert MIN_TILES <= 31
    check_against_both(K.synth_normal(1037, N, F64, seed=9102 + N, sigma=30.0))


def test_threshold_between_the_two_tile_kernels():
    assert MIN_TILES > 8
    T = 333
    f = K.synth_normal(T, MIN_TILES * 128, F64, seed=9103, sigma=30.0)
    check_against_both(f)
    below = f[:, :(MIN_TILES - 1) * 128, :].contiguous()
    g, k = gram_on(below)
    assert k == [SINGLE], k
    assert rel(g, contraction(below)) < 1e-12 and torch.equal(g, g.T)


@pytest.mark.parametrize("T", [5, 36])
def test_fewer_stages_than_the_ring_is_deep(T):
    f = K.synth_normal(T, 4096, F64, seed=9104 + T, sigma=30.0)
    check_against_both(f)


def test_accumulate_and_skipped_leading_block():
    N = 4096
    f = K.synth_normal(8003, N, F64, seed=9105, sigma=30.0)
    g, k = gram_on(f)
    assert is_macro(k), k
    scale = float(g.abs().max())
    acc, k = gram_on(f[:7000].contiguous())
    assert is_macro(k), k
    _, k = gram_on(f[7000:].contiguous(), out=acc, accumulate=True)
    assert is_macro(k), k
    assert float((acc - g).abs().max()) < 1e-11 * scale
    # a skipped leading block keeps the single-tile kernel
    part = torch.full((N, N), -7.0, dtype=F64, device="cuda")
    _, k = gram_on(f, out=part, first_col=256)
    assert k == [SINGLE], k
    mask = torch.ones((N, N), dtype=torch.bool, device="cuda")
    mask[:256, :256] = False
    assert float((part[mask] - g[mask]).abs().max()) < 1e-13 * scale
    assert float((part[:256, :256] + 7.0).abs().max()) == 0.0


def test_workspace_query_is_the_plan_of_the_call():
    """aggf_gram_workspace_bytes suffices for the call it describes (K.gram passes exactly that), and a workspace cut to
    half the slabs gives the same G to rounding with fewer splits."""
    T, N = 3001, 4096
    f = K.synth_normal(T, N, F64, seed=9106, sigma=30.0)
    need = _lib.load().aggf_gram_workspace_bytes(T, N, N, K.dtype_code(F64), K.dtype_code(F64), 0)
    g, k = gram_on(f, ws_limit_bytes=need)
    assert is_macro(k), k
    half, k = gram_on(f, ws_limit_bytes=need // 2)
    assert is_macro(k), k
    scale = float(g.abs().max())
    assert float((half - g).abs().max()) < 1e-13 * scale and torch.equal(half, half.T)
    assert rel(half, contraction(f)) < 1e-12
