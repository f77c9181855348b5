"""Thin Python wrappers over the libaggf C ABI, operating on torch (ROCm) tensors.

torch is only the array container here (device memory, current stream); all
arithmetic happens in the hand-written HIP kernels behind ``include/aggf.h``.
"""
from __future__ import annotations

import contextlib
import weakref
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, drop_workspace, dtype_code, lib, ptr, stream_ptr, workspace  # noqa: F401

_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
_NP_OF = {torch.float32: np.dtype(np.float32), torch.float64: np.dtype(np.float64)}

# ------------------------------------------------------------------ per-stage HIP-event timers

_timers: Optional[dict] = None


def start_timers() -> None:
    """Bracket every libaggf stage with HIP events on the launching stream (bench.py)."""
    global _timers
    _timers = {}


def stop_timers() -> dict:
    """{stage: {"ms": total, "calls": n}}; synchronises the device."""
    global _timers
    out = {}
    if _timers is not None:
        torch.cuda.synchronize()
        for name, pairs in _timers.items():
            out[name] = {"ms": float(sum(a.elapsed_time(b) for a, b in pairs)), "calls": len(pairs)}
    _timers = None
    return out


@contextlib.contextmanager
def _timed(name: str):
    if _timers is None:
        yield
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    try:
        yield
    finally:
        b.record()
        _timers.setdefault(name, []).append((a, b))


# ------------------------------------------------------------------ containers

_cache_stack: list = []


@contextlib.contextmanager
def upload_cache():
    """Within this context a NumPy array is copied to the GPU at most once (keyed by identity)."""
    _cache_stack.append({})
    try:
        yield
    finally:
        _cache_stack.pop()


def is_torch(x) -> bool:
    return isinstance(x, torch.Tensor)


def default_device() -> torch.device:
    lib()
    return torch.device("cuda", torch.cuda.current_device())


def as_device(x, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """NumPy array / CPU tensor / GPU tensor -> contiguous GPU tensor (float32 or float64)."""
    if is_torch(x):
        t = x
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
        if not t.is_cuda:
            t = t.to(default_device())
        if dtype is not None and t.dtype != dtype:
            t = t.to(dtype)
        return t.contiguous()
    arr = np.asarray(x)
    key = None
    if _cache_stack and isinstance(x, np.ndarray):
        key = (id(x), str(dtype))
        hit = _cache_stack[-1].get(key)
        if hit is not None and hit[0]() is x:
            return hit[1]
    if arr.dtype not in (np.float32, np.float64):
        arr = arr.astype(np.float64)
    t = torch.from_numpy(np.ascontiguousarray(arr)).to(default_device())
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    if key is not None:
        _cache_stack[-1][key] = (weakref.ref(x), t)
    return t


def like_input(t: torch.Tensor, template):
    """Return t as the same kind of container as template (NumPy array or torch tensor)."""
    if is_torch(template):
        return t if template.is_cuda else t.cpu()
    return t.cpu().numpy()


def np_dtype_of(x) -> np.dtype:
    if is_torch(x):
        return _NP_OF.get(x.dtype, np.dtype(np.float64))
    return np.asarray(x).dtype if not isinstance(x, np.ndarray) else x.dtype


def torch_dtype(npdt) -> torch.dtype:
    return _TORCH_OF[np.dtype(npdt)]


# ------------------------------------------------------------------ K1 Gram


def gram(
    forces: torch.Tensor,
    grp_ptr: Optional[torch.Tensor],
    grp_atoms: Optional[torch.Tensor],
    n_red: int,
    compute_dtype: torch.dtype,
    out: Optional[torch.Tensor] = None,
    accumulate: bool = False,
    ws_limit_bytes: Optional[int] = None,
    first_col: int = 0,
) -> torch.Tensor:
    """G (n_red, n_red) float64 from forces (T, N, 3); see aggf_gram in include/aggf.h.  ``first_col`` > 0
    (a multiple of 128, no constraint groups): the leading first_col x first_col block of ``out`` is the
    caller's and is not computed (aggf_gram_from_column)."""
    l = lib()
    T, N, D = forces.shape
    if D != 3:
        raise ValueError("forces must have shape (n_frames, n_sites, 3)")
    if T == 0:
        raise ValueError("empty trajectory")
    dev = forces.device
    if out is None:
        out = torch.empty((n_red, n_red), dtype=torch.float64, device=dev)
        accumulate = False
    ind, cd = dtype_code(forces.dtype), dtype_code(compute_dtype)
    if first_col and grp_ptr is None:
        need = l.aggf_gram_from_column_workspace_bytes(T, N, n_red, ind, cd, int(first_col))
    else:
        need = l.aggf_gram_workspace_bytes(T, N, n_red, ind, cd, 1 if grp_ptr is not None else 0)
    if ws_limit_bytes is not None:
        need = min(need, int(ws_limit_bytes))
    ws = workspace(need, dev, "gram")
    with _timed("gram"):
        if first_col:
            if grp_ptr is not None:
                raise ValueError("first_col needs a regression matrix without constraint groups")
            check(
                l.aggf_gram_from_column(ptr(forces), T, N, ind, cd, n_red, int(first_col), ptr(out),
                                        1 if accumulate else 0, ptr(ws), need, stream_ptr()),
                "aggf_gram_from_column",
            )
        else:
            check(
                l.aggf_gram(ptr(forces), T, N, ind, cd, ptr(grp_ptr), ptr(grp_atoms), n_red, ptr(out),
                            1 if accumulate else 0, ptr(ws), need, stream_ptr()),
                "aggf_gram",
            )
    return out


def eq_qp_solve(
    G: torch.Tensor,
    l2: float,
    l2_diag: Optional[torch.Tensor],
    A: torch.Tensor,
    B: Optional[torch.Tensor] = None,
    schur_reg: float = 0.0,
    n_refine: int = 1,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """X (nrhs, n) and stats (4,) -- both on the device; see aggf_eq_qp_solve."""
    l = lib()
    n = G.shape[0]
    m = A.shape[0]
    nrhs = m if B is None else B.shape[1]
    dev = G.device
    X = torch.empty((nrhs, n), dtype=torch.float64, device=dev)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    need = l.aggf_eq_qp_workspace_bytes(n, m, nrhs)
    ws = workspace(need, dev, "solve")
    with _timed("solve"):
        check(
            l.aggf_eq_qp_solve(ptr(G), n, float(l2), ptr(l2_diag), ptr(A), m, ptr(B), nrhs, float(schur_reg),
                               int(n_refine), ptr(X), ptr(stats), ptr(ws), need, stream_ptr()),
            "aggf_eq_qp_solve",
        )
    return X, stats


def eq_qp_solve_pinned(G: torch.Tensor, l2: float, l2_diag: Optional[torch.Tensor], pin_idx: torch.Tensor):
    """X (m, n) and stats (4,) for one-hot constraint rows: row i of the constraint matrix is the unit vector at
    pin_idx[i] (int32 device array, distinct entries), right-hand sides = identity; see aggf_eq_qp_solve_pinned."""
    l = lib()
    n, m = G.shape[0], pin_idx.numel()
    X = torch.empty((m, n), dtype=torch.float64, device=G.device)
    stats = torch.empty(4, dtype=torch.float64, device=G.device)
    need = l.aggf_eq_qp_pinned_workspace_bytes(n, m)
    ws = workspace(need, G.device, "solve")
    with _timed("solve"):
        check(l.aggf_eq_qp_solve_pinned(ptr(G), n, float(l2), ptr(l2_diag), ptr(pin_idx), m, ptr(X), ptr(stats), ptr(ws),
                                        need, stream_ptr()), "aggf_eq_qp_solve_pinned")
    return X, stats


def eq_qp_batched_bytes(n: int, m: int, nrhs: int, n_problems: int) -> int:
    return int(lib().aggf_eq_qp_batched_workspace_bytes(n, m, nrhs, n_problems))


def eq_qp_solve_batched(
    G: torch.Tensor,
    l2: float,
    l2_diag: Optional[torch.Tensor],
    A: torch.Tensor,
    B: Optional[torch.Tensor] = None,
    schur_reg: float = 0.0,
    n_refine: int = 1,
    AtA: Optional[torch.Tensor] = None,
    perm: Optional[torch.Tensor] = None,
    a_first_col: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Independent problems side by side: G (p, n, n), A (p, m, n), B (p, m, nrhs) or None ->
    X (p, nrhs, n), stats (p, 4); see aggf_eq_qp_solve_batched.  ``AtA`` (p, n, n): the caller's A'A (lower
    triangle read), aggf_eq_qp_solve_batched_shift; with it ``perm`` (p, n) int32 = the order in which the
    factorisation takes the variables and ``a_first_col`` = the number of leading variables (in that order) no
    constraint row touches in any problem."""
    l = lib()
    if G.dim() != 3 or A.dim() != 3 or G.shape[0] != A.shape[0] or G.shape[1] != G.shape[2] or A.shape[2] != G.shape[1]:
        raise ValueError(f"shape mismatch: G {tuple(G.shape)}, A {tuple(A.shape)}")
    if G.dtype != torch.float64 or A.dtype != torch.float64 or not G.is_contiguous() or not A.is_contiguous():
        raise ValueError("G and A must be contiguous float64")
    npb, n, _ = G.shape
    m = A.shape[1]
    if B is not None and (B.dim() != 3 or B.shape[0] != npb or B.shape[1] != m or B.dtype != torch.float64
                          or not B.is_contiguous()):
        raise ValueError(f"shape mismatch: B {tuple(B.shape)}")
    nrhs = m if B is None else B.shape[2]
    dev = G.device
    X = torch.empty((npb, nrhs, n), dtype=torch.float64, device=dev)
    stats = torch.empty((npb, 4), dtype=torch.float64, device=dev)
    need = l.aggf_eq_qp_batched_workspace_bytes(n, m, nrhs, npb)
    ws = workspace(need, dev, "solve")
    if AtA is not None:
        if AtA.shape != G.shape or AtA.dtype != torch.float64 or not AtA.is_contiguous():
            raise ValueError(f"AtA must be contiguous float64 of G's shape, got {tuple(AtA.shape)}")
        if perm is not None and (perm.shape != (npb, n) or perm.dtype != torch.int32 or not perm.is_contiguous()):
            raise ValueError(f"perm must be contiguous int32 of shape {(npb, n)}, got {tuple(perm.shape)}")
        with _timed("solve"):
            check(
                l.aggf_eq_qp_solve_batched_shift(ptr(G), n, float(l2), ptr(l2_diag), ptr(A), ptr(AtA), ptr(perm),
                                                 int(a_first_col) if perm is not None else 0, m, ptr(B), nrhs,
                                                 float(schur_reg), int(n_refine), npb, ptr(X), ptr(stats), ptr(ws), need,
                                                 stream_ptr()),
                "aggf_eq_qp_solve_batched_shift",
            )
        return X, stats
    if perm is not None:
        raise ValueError("perm needs AtA (aggf_eq_qp_solve_batched_shift)")
    with _timed("solve"):
        check(
            l.aggf_eq_qp_solve_batched(ptr(G), n, float(l2), ptr(l2_diag), ptr(A), m, ptr(B), nrhs, float(schur_reg),
                                       int(n_refine), npb, ptr(X), ptr(stats), ptr(ws), need, stream_ptr()),
            "aggf_eq_qp_solve_batched",
        )
    return X, stats


def device_memory(device=None) -> Tuple[int, int]:
    """(free, total) bytes of HBM on the current device (aggf_device_info)."""
    import ctypes as C

    cu, free, total = C.c_int32(0), C.c_size_t(0), C.c_size_t(0)
    check(lib().aggf_device_info(C.byref(cu), C.byref(free), C.byref(total)), "aggf_device_info")
    return int(free.value), int(total.value)


def expand_map(X: torch.Tensor, group_of_atom: torch.Tensor, N: int) -> torch.Tensor:
    l = lib()
    n_rows, n_red = X.shape
    W = torch.empty((n_rows, N), dtype=torch.float64, device=X.device)
    check(l.aggf_expand_map(ptr(X), n_rows, n_red, ptr(group_of_atom), N, ptr(W), stream_ptr()), "aggf_expand_map")
    return W


# ------------------------------------------------------------------ K3 apply


def linearmap_apply(
    points: torch.Tensor,
    matrix: torch.Tensor,
    nan_fill: Optional[float] = None,
    want_sumsq: bool = False,
    nan_probe: Optional[torch.Tensor] = None,
):
    """out (T, n_cg, 3) in matrix.dtype; optional device scalar sum of squares.

    ``nan_probe``: zeroed int32 device scalar that is set to 1 if ``points`` holds a NaN."""
    l = lib()
    T, N, D = points.shape
    n_cg, N2 = matrix.shape
    if D != 3 or N2 != N:
        raise ValueError(f"shape mismatch: points {tuple(points.shape)}, matrix {tuple(matrix.shape)}")
    dev = points.device
    out = torch.empty((T, n_cg, 3), dtype=matrix.dtype, device=dev)
    if T == 0:
        return (out, torch.zeros(1, dtype=torch.float64, device=dev)) if want_sumsq else out
    sumsq = torch.empty(1, dtype=torch.float64, device=dev) if want_sumsq else None
    need = l.aggf_linearmap_apply_workspace_bytes(T, N, n_cg) if want_sumsq else 0
    ws = workspace(need, dev, "apply") if want_sumsq else None
    with _timed("apply"):
        check(
            l.aggf_linearmap_apply(ptr(points), T, N, dtype_code(points.dtype), ptr(matrix), n_cg,
                                   dtype_code(matrix.dtype),
                                   _lib.NAN_REPLACE if nan_fill is not None else _lib.NAN_PROPAGATE,
                                   0.0 if nan_fill is None else float(nan_fill), ptr(out), ptr(sumsq), ptr(nan_probe),
                                   ptr(ws), need, stream_ptr()),
            "aggf_linearmap_apply",
        )
    return (out, sumsq) if want_sumsq else out


def slice_gather(points: torch.Tensor, idx: torch.Tensor, out_dtype: torch.dtype,
                 nan_probe: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t, c, :] = points[t, idx[c], :] (aggf_slice_gather).  ``nan_probe``: zeroed int32 device scalar (from
    :func:`take_flag`) that is set to 1 if a gathered value is NaN -- the scan rides along with the gather."""
    l = lib()
    T, N, D = points.shape
    n_cg = idx.numel()
    out = torch.empty((T, n_cg, 3), dtype=out_dtype, device=points.device)
    if T == 0:
        return out
    with _timed("gather"):
        check(
            l.aggf_slice_gather(ptr(points), T, N, dtype_code(points.dtype), ptr(idx), n_cg, dtype_code(out_dtype),
                                ptr(out), ptr(nan_probe), stream_ptr()),
            "aggf_slice_gather",
        )
    return out


_flag_pool: dict = {}
_side_streams: dict = {}


def take_flag(device) -> torch.Tensor:
    """A ZEROED int32 device scalar (shape (1,)) from a per-device pool; hand it back with :func:`read_flag`.

    Why a pool: ``torch.zeros(1)`` is a fill kernel on the current stream, and a one-workgroup kernel queued while a
    grid-stride kernel of another stream (the coordinate gather underneath the force map's apply) owns every wave
    slot waits until one of that kernel's workgroups retires -- 1.4 ms + 0.55 ms per step at BASELINE's
    configuration (rocprofv3 timeline, round 3).  Pool flags are zeroed in blocks of 64 and re-zeroed only after a
    kernel has actually set them, so the steady state issues no fill at all."""
    pool = _flag_pool.setdefault(str(device), [])
    if not pool:
        # The flags are used on any stream, so their fill must be over before the first one is handed out.  It runs
        # on a stream of the pool's own and only THAT stream is waited for, once per 64 flags: the caller's current
        # stream (which may sit behind a long kernel) is never waited for here.
        key = (str(device), "flags")
        st = _side_streams.get(key)
        if st is None:
            st = _side_streams[key] = torch.cuda.Stream(device=device)
        with torch.cuda.stream(st):
            block = torch.zeros(64, dtype=torch.int32, device=device)
        st.synchronize()
        pool.extend(block[i:i + 1] for i in range(64))
    return pool.pop()


def read_flag(flag: torch.Tensor) -> bool:
    """Host value of a flag from :func:`take_flag` (synchronises); the flag goes back to the pool, zeroed.  A flag is
    handed back exactly once: a second hand-back would let two later kernels share it."""
    pool = _flag_pool.setdefault(str(flag.device), [])
    if any(f.data_ptr() == flag.data_ptr() for f in pool):
        raise RuntimeError("read_flag: this flag is already back in the pool")
    v = bool(flag.item())
    if v:
        flag.zero_()
        torch.cuda.current_stream(flag.device).synchronize()  # the next user may sit on another stream
    pool.append(flag)
    return v


def nan_flag(x: torch.Tensor) -> torch.Tensor:
    """Device int32 flag (shape (1,), from :func:`take_flag`: read it with :func:`read_flag`): non-zero iff x holds a
    NaN.  No host synchronisation."""
    flag = take_flag(x.device)
    if x.numel():
        check(lib().aggf_has_nan(ptr(x), x.numel(), dtype_code(x.dtype), ptr(flag), stream_ptr()), "aggf_has_nan")
    return flag


def side_stream(device) -> "torch.cuda.Stream":
    """One auxiliary stream per device for work that may overlap the main stream's kernels."""
    key = str(device)
    st = _side_streams.get(key)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side_streams[key] = st
    return st


def side_streams(device, n: int) -> list:
    """n auxiliary streams per device, created once (workspaces are cached per stream: fresh streams on
    every call would pin a new set of scratch buffers each time)."""
    key = (str(device), "pool")
    pool = _side_streams.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


def has_nan(x: torch.Tensor) -> bool:
    l = lib()
    if x.numel() == 0:
        return False
    flag = take_flag(x.device)
    check(l.aggf_has_nan(ptr(x), x.numel(), dtype_code(x.dtype), ptr(flag), stream_ptr()), "aggf_has_nan")
    return read_flag(flag)


def allclose(a: torch.Tensor, b: torch.Tensor, rtol: float = 1e-5, atol: float = 1e-8) -> bool:
    l = lib()
    if a.numel() == 0:
        return True
    flag = take_flag(a.device)
    check(
        l.aggf_not_close(ptr(a), ptr(b), a.numel(), dtype_code(a.dtype), float(rtol), float(atol), ptr(flag),
                         stream_ptr()),
        "aggf_not_close",
    )
    return not read_flag(flag)


def sumsq(x: torch.Tensor) -> torch.Tensor:
    """Device scalar (shape (1,), float64): sum of squares of x, fixed summation order."""
    l = lib()
    out = torch.zeros(1, dtype=torch.float64, device=x.device)
    if x.numel() == 0:
        return out
    need = l.aggf_sumsq_workspace_bytes()
    ws = workspace(need, x.device, "sumsq")
    check(l.aggf_sumsq(ptr(x), x.numel(), dtype_code(x.dtype), ptr(out), ptr(ws), need, stream_ptr()), "aggf_sumsq")
    return out


def sym_pack_upper(G: torch.Tensor) -> torch.Tensor:
    """Packed upper triangles (batch, n (n + 1) / 2) of symmetric float64 matrices G (..., n, n)."""
    l = lib()
    n = G.shape[-1]
    assert G.dtype == torch.float64 and G.shape[-2] == n and G.is_contiguous()
    batch = G.numel() // (n * n)
    out = torch.empty((batch, n * (n + 1) // 2), dtype=torch.float64, device=G.device)
    check(l.aggf_sym_pack_upper(ptr(G), n, batch, ptr(out), stream_ptr(G.device)), "aggf_sym_pack_upper")
    return out


def sym_unpack_upper(packed: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """Both triangles of G (..., n, n) from packed upper triangles; in place, returns G."""
    l = lib()
    n = G.shape[-1]
    assert G.dtype == torch.float64 and packed.dtype == torch.float64 and G.is_contiguous() and packed.is_contiguous()
    batch = G.numel() // (n * n)
    assert packed.numel() == batch * (n * (n + 1) // 2)
    check(l.aggf_sym_unpack_upper(ptr(packed), n, batch, ptr(G), stream_ptr(G.device)), "aggf_sym_unpack_upper")
    return G


def gram_quadform(G: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """q[i] = x_i' G x_i for the rows of X (m, n); float64 on the device."""
    l = lib()
    n = G.shape[0]
    m = X.shape[0]
    assert G.dtype == torch.float64 and X.dtype == torch.float64 and X.shape[1] == n
    q = torch.empty(m, dtype=torch.float64, device=G.device)
    need = l.aggf_gram_quadform_workspace_bytes(n, m)
    ws = workspace(need, G.device, "quadform")
    check(l.aggf_gram_quadform(ptr(G.contiguous()), n, ptr(X.contiguous()), m, ptr(q), ptr(ws), need, stream_ptr()),
          "aggf_gram_quadform")
    return q


def axpby(a: float, x: torch.Tensor, b: float, y: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a*x + b*y (float64, same shape)."""
    assert x.dtype == torch.float64 and y.dtype == torch.float64 and x.shape == y.shape
    x = x.contiguous()
    y = y.contiguous()
    if out is None:
        out = torch.empty_like(x)
    check(lib().aggf_daxpby(x.numel(), float(a), ptr(x), float(b), ptr(y), ptr(out), stream_ptr()), "aggf_daxpby")
    return out


# ------------------------------------------------------------------ K5 augment


def premap_columns(matrix_host: np.ndarray, dtype: torch.dtype, device):
    """Columns of the premap M (n_cg, N) in compressed form for aggf_condnormal_augment."""
    mt = np.ascontiguousarray(matrix_host.T)  # (N, n_cg)
    rows, cols = np.nonzero(mt)
    ptr_h = np.zeros(mt.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=mt.shape[0]), out=ptr_h[1:])
    return (torch.from_numpy(ptr_h).to(device), torch.from_numpy(cols.astype(np.int32)).to(device),
            torch.from_numpy(mt[rows, cols]).to(device=device, dtype=dtype))


def condnormal_augment(
    coords: torch.Tensor,
    forces: torch.Tensor,
    columns,
    n_cg: int,
    mean: torch.Tensor,
    var: float,
    kbt: float,
    noise: Optional[torch.Tensor],
    seed: int,
    frame_offset: int,
):
    l = lib()
    T, N, _ = coords.shape
    mt_ptr, mt_idx, mt_val = columns
    out_dtype = torch.promote_types(coords.dtype, mt_val.dtype)
    oc = torch.empty((T, N + n_cg, 3), dtype=out_dtype, device=coords.device)
    of = torch.empty((T, N + n_cg, 3), dtype=out_dtype, device=coords.device)
    if T == 0:
        return oc, of
    with _timed("augment"):
        check(
            l.aggf_condnormal_augment(ptr(coords), ptr(forces), T, N, dtype_code(coords.dtype), ptr(mt_ptr),
                                      ptr(mt_idx), ptr(mt_val), n_cg, dtype_code(mt_val.dtype), ptr(mean), ptr(noise),
                                      int(seed) & (2**64 - 1), int(frame_offset), float(var), float(kbt), ptr(oc),
                                      ptr(of), stream_ptr()),
            "aggf_condnormal_augment",
        )
    return oc, of


def condnormal_sites(mean: torch.Tensor, var: float, kbt: float, noise: Optional[torch.Tensor], seed: int,
                     frame_offset: int, out_dtype: torch.dtype):
    """(y, Fa): generated-site coordinates and forces (T, n_cg, 3), the non-copy part of the extended trajectory;
    same arithmetic and Philox stream as :func:`condnormal_augment` (aggf_condnormal_sites)."""
    T, n_cg, _ = mean.shape
    y = torch.empty((T, n_cg, 3), dtype=out_dtype, device=mean.device)
    fa = torch.empty((T, n_cg, 3), dtype=out_dtype, device=mean.device)
    if T == 0:
        return y, fa
    with _timed("augment"):
        check(lib().aggf_condnormal_sites(ptr(mean), ptr(noise), int(seed) & (2**64 - 1), int(frame_offset), T, n_cg,
                                          dtype_code(mean.dtype), float(var), float(kbt), ptr(y), ptr(fa),
                                          dtype_code(out_dtype), stream_ptr()), "aggf_condnormal_sites")
    return y, fa


def residual_over_var(gen: torch.Tensor, mean: torch.Tensor, var: float, out_dtype: torch.dtype, want_pos: bool = True,
                      want_neg: bool = True):
    """(r, -r) with r = (gen - mean) / var, elementwise, in ``out_dtype`` (aggf_residual_over_var): the log-gradients
    of a scalar-covariance conditional normal.  An output that is not wanted is None."""
    assert gen.shape == mean.shape and gen.is_contiguous() and mean.is_contiguous()
    pos = torch.empty(gen.shape, dtype=out_dtype, device=gen.device) if want_pos else None
    neg = torch.empty(gen.shape, dtype=out_dtype, device=gen.device) if want_neg else None
    if gen.numel():
        with _timed("augment"):
            check(lib().aggf_residual_over_var(ptr(gen), dtype_code(gen.dtype), ptr(mean), dtype_code(mean.dtype),
                                               gen.numel(), float(var), ptr(pos), ptr(neg), dtype_code(out_dtype),
                                               stream_ptr()), "aggf_residual_over_var")
    return pos, neg


def frames_matmul(x: torch.Tensor, b: torch.Tensor, sub: Optional[torch.Tensor] = None,
                  add: Optional[torch.Tensor] = None, alpha: float = 1.0) -> torch.Tensor:
    """``add + alpha (x - sub) @ b.T`` on flattened frames: x, sub (T, K), b (J, K), add (T, J), one dtype
    (aggf_frames_matmul)."""
    T, Kd = x.shape
    J = b.shape[0]
    assert b.shape[1] == Kd and b.dtype == x.dtype and x.is_contiguous() and b.is_contiguous()
    assert sub is None or (sub.shape == x.shape and sub.dtype == x.dtype and sub.is_contiguous())
    assert add is None or (tuple(add.shape) == (T, J) and add.dtype == x.dtype and add.is_contiguous())
    out = torch.empty((T, J), dtype=x.dtype, device=x.device)
    if T:
        with _timed("augment"):
            check(lib().aggf_frames_matmul(ptr(x), ptr(sub), T, Kd, ptr(b), J, ptr(add), float(alpha),
                                           dtype_code(x.dtype), ptr(out), stream_ptr()), "aggf_frames_matmul")
    return out


def augment_concat(coords: torch.Tensor, forces: torch.Tensor, gen: torch.Tensor, corr: torch.Tensor,
                   lgrad: torch.Tensor, kbt: float):
    """([coords ; gen], [forces + kbt corr ; kbt lgrad]) in the promoted dtype (aggf_augment_concat): the
    concatenation step of the general Augmenter protocol (trajectory/core.py:384-390)."""
    T, N, _ = coords.shape
    n_aug = gen.shape[1]
    assert forces.shape == coords.shape and forces.dtype == coords.dtype
    assert gen.dtype == corr.dtype == lgrad.dtype and corr.shape == coords.shape and lgrad.shape == gen.shape
    out_dtype = torch.promote_types(coords.dtype, gen.dtype)
    oc = torch.empty((T, N + n_aug, 3), dtype=out_dtype, device=coords.device)
    of = torch.empty((T, N + n_aug, 3), dtype=out_dtype, device=coords.device)
    if T:
        with _timed("augment"):
            check(lib().aggf_augment_concat(ptr(coords), ptr(forces), dtype_code(coords.dtype), ptr(gen), ptr(corr),
                                            ptr(lgrad), dtype_code(gen.dtype), T, N, n_aug, float(kbt), ptr(oc),
                                            ptr(of), stream_ptr()), "aggf_augment_concat")
    return oc, of


def gram_pair_ok(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Can aggf_gram_pair read [a | b] in place?  (same dtype, 128-multiples of sites, 16-byte aligned)"""
    return (a.dtype == b.dtype and a.dtype in (torch.float32, torch.float64) and a.shape[0] == b.shape[0] and a.shape[0] > 0
            and a.shape[1] % 128 == 0 and b.shape[1] % 128 == 0 and a.is_contiguous() and b.is_contiguous()
            and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)


def gram_pair(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Gram matrix ((Na + Nb)^2 float64) of the column-concatenation [a | b] of two (T, ., 3) arrays, read where
    they lie (aggf_gram_pair); products in the arrays' dtype."""
    l = lib()
    T, N, _ = a.shape
    N2 = b.shape[1]
    out = torch.empty((N + N2, N + N2), dtype=torch.float64, device=a.device)
    need = l.aggf_gram_pair_workspace_bytes(T, N, N2, dtype_code(a.dtype))
    ws = workspace(need, a.device, "gram")
    with _timed("gram"):
        check(l.aggf_gram_pair(ptr(a), N, ptr(b), N2, T, dtype_code(a.dtype), ptr(out), 0, ptr(ws), need, stream_ptr()),
              "aggf_gram_pair")
    return out


def augmented_gram(Gx: torch.Tensor, N: int, columns) -> torch.Tensor:
    """Tm' Gx Tm, Tm = [[I, 0], [-C, I]]: Gram matrix of [F - Fa C | Fa] from that of [F | Fa] (aggf_augmented_gram);
    ``columns`` = premap_columns(C, float64)."""
    l = lib()
    n = Gx.shape[0]
    n2 = n - N
    cp, ci, cv = columns
    assert Gx.dtype == torch.float64 and cv.dtype == torch.float64 and Gx.is_contiguous()
    out = torch.empty_like(Gx)
    need = l.aggf_augmented_gram_workspace_bytes(N, n2)
    ws = workspace(need, Gx.device, "auggram")
    check(l.aggf_augmented_gram(ptr(Gx), N, n2, ptr(cp), ptr(ci), ptr(cv), ptr(out), ptr(ws), need, stream_ptr()),
          "aggf_augmented_gram")
    return out


def sym_group_reduce(G: torch.Tensor, grp_ptr: torch.Tensor, grp_atoms: torch.Tensor, n_red: int) -> torch.Tensor:
    """C' G C for the 0/1 constraint matrix given as CSR groups (aggf_sym_group_reduce)."""
    out = torch.empty((n_red, n_red), dtype=torch.float64, device=G.device)
    check(lib().aggf_sym_group_reduce(ptr(G.contiguous()), G.shape[0], ptr(grp_ptr), ptr(grp_atoms), n_red, ptr(out),
                                      stream_ptr()), "aggf_sym_group_reduce")
    return out


# ------------------------------------------------------------------ synthetic data


def index_to_device(host: np.ndarray, device) -> torch.Tensor:
    """A host index array as a device tensor WITHOUT waiting for the caller's stream: staged in pinned memory and copied
    asynchronously on the current stream.  (``torch.from_numpy(host).to(device)`` copies from pageable memory and
    returns only when the current stream has drained: behind a long kernel of the caller's the host stood still.)"""
    staged = torch.from_numpy(np.ascontiguousarray(host)).pin_memory()
    return staged.to(device, non_blocking=True)  # (the pinned block is not reused before this copy has run)


def take_frames(x: torch.Tensor, idx) -> torch.Tensor:
    """x[idx] along the frame axis as one gather kernel (aggf_take_frames); ``idx``: integer array-like or tensor.
    A host index is checked on the host and the call does not wait for the stream; an index tensor on the DEVICE is
    range-checked on the host too, which waits for the current stream once."""
    x = x.contiguous()
    n_src = x.shape[0]
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        # host index array (the fold bookkeeping of the cross-validation): validated and wrapped on the host, where it
        # lies -- no device min / max, no synchronisation inside the fold loops
        host = np.asarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64).reshape(-1)
        if host.size and (host.min() < -n_src or host.max() >= n_src):
            raise IndexError(f"frame index out of range for {n_src} frames")
        if host.size and host.min() < 0:
            host = np.where(host < 0, host + n_src, host)
        idx = index_to_device(host, x.device)
    else:
        idx = idx.to(dtype=torch.int64).contiguous()
        lo, hi = (int(v) for v in torch.stack([idx.min(), idx.max()]).tolist()) if idx.numel() else (0, 0)  # one sync
        if idx.numel() and (lo < -n_src or hi >= n_src):
            raise IndexError(f"frame index out of range for {n_src} frames")
        if idx.numel() and lo < 0:
            idx = torch.where(idx < 0, idx + n_src, idx)
    n = idx.numel()
    out = torch.empty((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    if n and n_src:
        row = int(np.prod(x.shape[1:])) if x.dim() > 1 else 1
        check(lib().aggf_take_frames(ptr(x), n_src, row, dtype_code(x.dtype), ptr(idx), n, ptr(out), stream_ptr()),
              "aggf_take_frames")
    return out


def concat_sites(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[a ; b] along the site axis of two (T, ., 3) arrays, in the promoted dtype (aggf_concat_sites)."""
    assert a.dim() == 3 and b.dim() == 3 and a.shape[0] == b.shape[0] and a.shape[2] == 3 and b.shape[2] == 3
    a, b = a.contiguous(), b.contiguous()
    dt = torch.promote_types(a.dtype, b.dtype)
    T = a.shape[0]
    out = torch.empty((T, a.shape[1] + b.shape[1], 3), dtype=dt, device=a.device)
    if T and a.shape[1] and b.shape[1]:
        check(lib().aggf_concat_sites(ptr(a), a.shape[1], dtype_code(a.dtype), ptr(b), b.shape[1], dtype_code(b.dtype), T,
                                      ptr(out), dtype_code(dt), stream_ptr()), "aggf_concat_sites")
    elif T:
        out.copy_(a if a.shape[1] else b)
    return out


def scale(x: torch.Tensor, alpha: float) -> torch.Tensor:
    """alpha * x as a product (aggf_scale): NaN / inf behave as in NumPy's ``alpha * x``."""
    x = x.contiguous()
    out = torch.empty_like(x)
    if x.numel():
        check(lib().aggf_scale(ptr(x), x.numel(), dtype_code(x.dtype), float(alpha), ptr(out), stream_ptr()), "aggf_scale")
    return out


def scaled(x, alpha):
    """``alpha * x`` for a trajectory array: device tensors through :func:`scale`, host arrays as they are (NumPy)."""
    if is_torch(x) and x.is_cuda and x.dtype in (torch.float32, torch.float64):
        return scale(x, float(alpha))
    return alpha * x


def synth_normal(T: int, N: int, dtype: torch.dtype, seed: int, frame_offset: int = 0, mean: float = 0.0,
                 sigma: float = 1.0, lattice: float = 0.0, device=None) -> torch.Tensor:
    l = lib()
    dev = device or default_device()
    out = torch.empty((T, N, 3), dtype=dtype, device=dev)
    check(
        l.aggf_synth_normal(ptr(out), T, N, dtype_code(dtype), int(seed), int(frame_offset), float(mean),
                            float(sigma), float(lattice), stream_ptr()),
        "aggf_synth_normal",
    )
    return out


# ------------------------------------------------------------------ K4 gb_feat


def group_reduce(x: torch.Tensor, grp_ptr: torch.Tensor, grp_atoms: torch.Tensor, n_groups: int, mean: bool,
                 out_dtype: torch.dtype) -> torch.Tensor:
    """(T, n_groups, 3): per-group sums (or means) of x (T, N, 3); see aggf_group_reduce."""
    l = lib()
    T, N, _ = x.shape
    out = torch.empty((T, n_groups, 3), dtype=out_dtype, device=x.device)
    if T == 0:
        return out
    check(
        l.aggf_group_reduce(ptr(x), T, N, dtype_code(x.dtype), ptr(grp_ptr), ptr(grp_atoms), n_groups,
                            1 if mean else 0, dtype_code(out_dtype), ptr(out), stream_ptr()),
        "aggf_group_reduce",
    )
    return out


def _gb_dtype(Pg, cg, centers) -> int:
    """Feature arithmetic type of the K4 calls: Pg, cg and centers must share it (float32 or float64)."""
    if not (Pg.dtype == cg.dtype == centers.dtype):
        raise TypeError(f"gb_feat operands differ in dtype: {Pg.dtype}, {cg.dtype}, {centers.dtype}")
    return dtype_code(Pg.dtype)


def _gb_box(name: str, box, Pg, near: bool):
    """(stride, images) of the ``box`` of a K4 function: stride as ``_box_arg`` gives it (None without a box), images
    None for lengths (the ``_pbc`` entry) and IMAGES_BRICK / IMAGES_NEAREST for the (T, 9) rows of a cell (the ``_cell``
    entry)."""
    if box is None:
        return None, None
    stride = _box_arg(name, box, Pg, cell=True, near=near)
    return stride, ((IMAGES_NEAREST if near else IMAGES_BRICK) if stride == 9 else None)


def gb_channels(Pg, cg, site: int, sizes, n_ch: int, centers, width: float, clip: float,
                box: Optional[torch.Tensor] = None, near: bool = False):
    """(gauss (T, n_ch, n_basis), grad (T, n_ch, n_basis, 3)) of one cg site; see aggf_gb_channels.  ``box`` ((3,) or
    (T, 3), the feature dtype; the same for every K4 function that takes one): distances and directions are those of
    the minimum image under that orthorhombic box (aggf_gb_channels_pbc); a frame whose box is bad is NaN.  (T, 9): the
    rows of a triclinic cell (``pbc.Cell.rows``), the brick image or, with ``near``, the nearest image
    (aggf_gb_channels_cell)."""
    stride, images = _gb_box("gb_channels", box, Pg, near)
    l = lib()
    T, G, _ = Pg.shape
    nb = centers.numel()
    gd = _gb_dtype(Pg, cg, centers)
    gauss = torch.empty((T, n_ch, nb), dtype=Pg.dtype, device=Pg.device)
    grad = torch.empty((T, n_ch, nb, 3), dtype=Pg.dtype, device=Pg.device)
    if T == 0 or n_ch == 0:
        return gauss, grad
    if box is None:
        check(
            l.aggf_gb_channels(ptr(Pg), ptr(cg), gd, T, G, cg.shape[1], site, ptr(sizes), n_ch, ptr(centers), nb,
                               float(width), float(clip), ptr(gauss), ptr(grad), stream_ptr()),
            "aggf_gb_channels",
        )
    elif images is not None:
        check(
            l.aggf_gb_channels_cell(ptr(Pg), ptr(cg), gd, T, G, cg.shape[1], site, ptr(sizes), n_ch, ptr(centers), nb,
                                    float(width), float(clip), ptr(box), ptr(gauss), ptr(grad), stream_ptr(), images),
            "aggf_gb_channels_cell",
        )
    else:
        check(
            l.aggf_gb_channels_pbc(ptr(Pg), ptr(cg), gd, T, G, cg.shape[1], site, ptr(sizes), n_ch, ptr(centers), nb,
                                   float(width), float(clip), ptr(box), stride, ptr(gauss), ptr(grad), stream_ptr()),
            "aggf_gb_channels_pbc",
        )
    return gauss, grad


def gb_regmat(Fg, Pg, cg, site: int, sizes, n_id: int, n_ch: int, centers, width: float, clip: float, kbt: float,
              out: torch.Tensor) -> torch.Tensor:
    """Fill out (T, ld_feat, 3) with the regression matrix of one cg site; see aggf_gb_regmat."""
    l = lib()
    T, G, _ = Fg.shape
    with _timed("gb_regmat"):
        check(
            l.aggf_gb_regmat(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg), _gb_dtype(Pg, cg, centers), T, G,
                             cg.shape[1], site, ptr(sizes),
                             n_id, n_ch, ptr(centers), centers.numel(), float(width), float(clip), float(kbt),
                             out.shape[1], ptr(out), dtype_code(out.dtype), stream_ptr()),
            "aggf_gb_regmat",
        )
    return out


def gb_apply(Fg, Pg, cg, sizes, n_id: int, n_ch: int, centers, width: float, clip: float, coef: torch.Tensor,
             box: Optional[torch.Tensor] = None, near: bool = False):
    """(T, n_cg, 3) float64: the [id | gb] feature-linear map applied; see aggf_gb_apply, and aggf_gb_apply_pbc /
    aggf_gb_apply_cell for ``box`` and ``near`` (as ``gb_channels``)."""
    stride, images = _gb_box("gb_apply", box, Pg, near)
    l = lib()
    T, G, _ = Fg.shape
    n_cg = cg.shape[1]
    out = torch.empty((T, n_cg, 3), dtype=torch.float64, device=Fg.device)
    if T == 0:
        return out
    with _timed("gb_apply"):
        if box is None:
            check(
                l.aggf_gb_apply(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg), _gb_dtype(Pg, cg, centers), T, G, n_cg,
                                ptr(sizes), n_id, n_ch,
                                ptr(centers), centers.numel(), float(width), float(clip), ptr(coef), coef.shape[1],
                                ptr(out), stream_ptr()),
                "aggf_gb_apply",
            )
        elif images is not None:
            check(
                l.aggf_gb_apply_cell(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg), _gb_dtype(Pg, cg, centers), T, G,
                                     n_cg, ptr(sizes), n_id, n_ch, ptr(centers), centers.numel(), float(width),
                                     float(clip), ptr(coef), coef.shape[1], ptr(box), ptr(out), stream_ptr(), images),
                "aggf_gb_apply_cell",
            )
        else:
            check(
                l.aggf_gb_apply_pbc(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg), _gb_dtype(Pg, cg, centers), T, G,
                                    n_cg, ptr(sizes), n_id, n_ch, ptr(centers), centers.numel(), float(width),
                                    float(clip), ptr(coef), coef.shape[1], ptr(box), stride, ptr(out), stream_ptr()),
                "aggf_gb_apply_pbc",
            )
    return out


def gb_compact_coefficients(coef: np.ndarray, n_id: int, device):
    """(coef_id (n_cg, n_id), col_ptr, col_idx, col_val) on the device for :func:`gb_apply_cols`: the non-zero
    Gaussian coefficients of every site as compressed rows."""
    coef = np.asarray(coef, dtype=np.float64)
    gauss = coef[:, n_id:]
    rows, cols = np.nonzero(gauss)
    ptr_h = np.zeros(coef.shape[0] + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=coef.shape[0]), out=ptr_h[1:])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return (to(coef[:, :n_id]) if n_id else None, to(ptr_h), to(cols.astype(np.int32)), to(gauss[rows, cols]))


def gb_apply_cols(Fg, Pg, cg, sizes, n_id: int, centers, width: float, clip: float, compact,
                  box: Optional[torch.Tensor] = None, near: bool = False):
    """gb_apply from the compact coefficient list of :func:`gb_compact_coefficients`; see aggf_gb_apply_cols, and
    aggf_gb_apply_cols_pbc / aggf_gb_apply_cols_cell for ``box`` and ``near`` (as ``gb_channels``)."""
    coef_id, col_ptr, col_idx, col_val = compact
    T, G, _ = Fg.shape
    n_cg = cg.shape[1]
    stride, images = _gb_box("gb_apply_cols", box, Pg, near)
    out = torch.empty((T, n_cg, 3), dtype=torch.float64, device=Fg.device)
    if T == 0:
        return out
    with _timed("gb_apply"):
        if box is None:
            check(
                lib().aggf_gb_apply_cols(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg), _gb_dtype(Pg, cg, centers), T,
                                         G, n_cg, ptr(sizes), n_id, ptr(coef_id), ptr(col_ptr), ptr(col_idx),
                                         ptr(col_val), ptr(centers), centers.numel(), float(width), float(clip),
                                         ptr(out), stream_ptr()),
                "aggf_gb_apply_cols",
            )
        elif images is not None:
            check(
                lib().aggf_gb_apply_cols_cell(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg),
                                              _gb_dtype(Pg, cg, centers), T, G, n_cg, ptr(sizes), n_id, ptr(coef_id),
                                              ptr(col_ptr), ptr(col_idx), ptr(col_val), ptr(centers), centers.numel(),
                                              float(width), float(clip), ptr(box), ptr(out), stream_ptr(), images),
                "aggf_gb_apply_cols_cell",
            )
        else:
            check(
                lib().aggf_gb_apply_cols_pbc(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg), _gb_dtype(Pg, cg, centers),
                                             T, G, n_cg, ptr(sizes), n_id, ptr(coef_id), ptr(col_ptr), ptr(col_idx),
                                             ptr(col_val), ptr(centers), centers.numel(), float(width), float(clip),
                                             ptr(box), stride, ptr(out), stream_ptr()),
                "aggf_gb_apply_cols_pbc",
            )
    return out


# ------------------------------------------------------------------ K3c / K4b / K4c per-frame contractions


def trjdot_frames(points: torch.Tensor, factor: torch.Tensor, trans: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[t,c,d] = sum_f factor[t,c,f] points[t,f,d] (+ trans[t,c,d]); see aggf_trjdot_frames."""
    T, N, D = points.shape
    if D != 3 or factor.dim() != 3 or factor.shape[0] != T or factor.shape[2] != N:
        raise ValueError(f"shape mismatch: points {tuple(points.shape)}, factor {tuple(factor.shape)}")
    n_cg = factor.shape[1]
    out_dtype = torch.promote_types(points.dtype, factor.dtype)
    if trans is not None:
        if tuple(trans.shape) != (T, n_cg, 3):
            raise ValueError(f"shape mismatch: trans {tuple(trans.shape)}, expected {(T, n_cg, 3)}")
        out_dtype = torch.promote_types(out_dtype, trans.dtype)
        if out_dtype == torch.float64 and points.dtype == factor.dtype == torch.float32:
            points = points.to(torch.float64)  # the kernel's out dtype is the promoted input dtype
        trans = trans.to(out_dtype).contiguous()
    out = torch.empty((T, n_cg, 3), dtype=out_dtype, device=points.device)
    if T == 0 or n_cg == 0:
        return out
    with _timed("trjdot_frames"):
        check(lib().aggf_trjdot_frames(ptr(points), dtype_code(points.dtype), ptr(factor), dtype_code(factor.dtype), T, N,
                                       n_cg, ptr(trans), ptr(out), dtype_code(out_dtype), stream_ptr()),
              "aggf_trjdot_frames")
    return out


def feat_contract(forces: torch.Tensor, feat: torch.Tensor, div: Optional[torch.Tensor], alpha: float,
                  ld: Optional[int] = None) -> torch.Tensor:
    """out (T, ld, 3): sum_a feat[t,a,f] F[t,a,d] + alpha div[t,f,d]; see aggf_feat_contract."""
    T, N, _ = forces.shape
    if feat.dim() != 3 or feat.shape[0] != T or feat.shape[1] != N:
        raise ValueError(f"shape mismatch: forces {tuple(forces.shape)}, feats {tuple(feat.shape)}")
    n_feat = feat.shape[2]
    if div is not None:
        if tuple(div.shape) != (T, n_feat, 3):
            raise ValueError(f"shape mismatch: feats {tuple(feat.shape)}, divs {tuple(div.shape)}")
        xdt = torch.promote_types(feat.dtype, div.dtype)
        feat, div = feat.to(xdt).contiguous(), div.to(xdt).contiguous()
    ld = n_feat if ld is None else int(ld)
    out_dtype = torch.promote_types(forces.dtype, feat.dtype)
    out = torch.empty((T, ld, 3), dtype=out_dtype, device=forces.device)
    if T == 0:
        return out
    with _timed("feat_contract"):
        check(lib().aggf_feat_contract(ptr(forces), dtype_code(forces.dtype), ptr(feat), ptr(div), dtype_code(feat.dtype),
                                       float(alpha), T, N, n_feat, ld, ptr(out), dtype_code(out_dtype), stream_ptr()),
              "aggf_feat_contract")
    return out


def feat_constraint_rows(feat: torch.Tensor, frame_idx: np.ndarray, M: torch.Tensor, site: int):
    """(A (S*n_cg, n_feat), b (S*n_cg, 1)) float64 for one cg site; see aggf_feat_constraint_rows."""
    T, N, n_feat = feat.shape
    idx = np.asarray(frame_idx, dtype=np.int64).reshape(-1)
    if idx.size == 0 or idx.min() < -T or idx.max() >= T:
        raise IndexError("constraint frame index outside the trajectory")
    idx = np.where(idx < 0, idx + T, idx)
    n_cg = M.shape[0]
    S = idx.size
    idx_dev = index_to_device(idx, feat.device)
    A = torch.empty((S * n_cg, n_feat), dtype=torch.float64, device=feat.device)
    b = torch.empty((S * n_cg, 1), dtype=torch.float64, device=feat.device)
    check(lib().aggf_feat_constraint_rows(ptr(feat), dtype_code(feat.dtype), T, N, n_feat, ptr(idx_dev), S, ptr(M), n_cg,
                                          int(site), ptr(A), ptr(b), stream_ptr()), "aggf_feat_constraint_rows")
    return A, b


def gb_constraint_rows(Mg: torch.Tensor, gauss: Optional[torch.Tensor], S: int, n_id: int, n_ch: int, n_basis: int,
                       site: int, out_A: Optional[torch.Tensor] = None, out_b: Optional[torch.Tensor] = None,
                       cols: Optional[torch.Tensor] = None):
    """Constraint rows of the fused [id | gb] features; see aggf_gb_constraint_rows.  ``cols`` (int32 device
    array of kept Gaussian columns ch*n_basis + k) gives the compacted layout; ``out_A`` may be wider than
    the feature count (trailing columns are zeroed)."""
    n_cg, G = Mg.shape
    n_cols = n_ch * n_basis if cols is None else int(cols.numel())
    n_feat = n_id + n_cols
    A = out_A if out_A is not None else torch.empty((S * n_cg, n_feat), dtype=torch.float64, device=Mg.device)
    b = out_b if out_b is not None else torch.empty((S * n_cg, 1), dtype=torch.float64, device=Mg.device)
    ld = A.shape[-1]
    gd = _lib.F32 if gauss is None else dtype_code(gauss.dtype)
    check(lib().aggf_gb_constraint_rows(ptr(Mg), ptr(gauss), gd, S, n_cg, G, n_id, n_ch, n_basis, ptr(cols), n_cols, ld,
                                        int(site), ptr(A), ptr(b), stream_ptr()), "aggf_gb_constraint_rows")
    return A, b


def gb_group_overlap(Mg: torch.Tensor) -> torch.Tensor:
    """Mg' Mg (G, G) float64; see aggf_gb_group_overlap."""
    n_cg, G = Mg.shape
    M2 = torch.empty((G, G), dtype=torch.float64, device=Mg.device)
    check(lib().aggf_gb_group_overlap(ptr(Mg), n_cg, G, ptr(M2), stream_ptr()), "aggf_gb_group_overlap")
    return M2


def gb_constraint_gram(M2: torch.Tensor, gauss: Optional[torch.Tensor], S: int, n_id: int, n_ch: int, n_basis: int,
                       out: torch.Tensor, cols: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A'A of gb_constraint_rows' rows into the lower triangle of ``out`` (ld, ld); see aggf_gb_constraint_gram."""
    G = M2.shape[0]
    n_cols = n_ch * n_basis if cols is None else int(cols.numel())
    if out.dim() != 2 or out.shape[0] != out.shape[1] or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("out must be a contiguous square float64 matrix")
    gd = _lib.F32 if gauss is None else dtype_code(gauss.dtype)
    check(lib().aggf_gb_constraint_gram(ptr(M2), ptr(gauss), gd, S, G, n_id, n_ch, n_basis, ptr(cols), n_cols,
                                        out.shape[0], ptr(out), stream_ptr()), "aggf_gb_constraint_gram")
    return out


def gb_distance_range(Pg: torch.Tensor, cg: torch.Tensor, n_ch: int, box: Optional[torch.Tensor] = None,
                      near: bool = False):
    """(rmin, rmax) (n_cg, G) float32: range over frames of every channel's distance to every cg site
    (evaluated in float32 whatever the feature dtype: the caller applies a safety margin).  ``box`` (as
    ``gb_channels``, in the dtype of ``Pg``): the range of the minimum-image distances (aggf_gb_distance_range_pbc),
    none of which exceeds half the cell's diagonal; the rows of a cell and ``near``: of the brick- or nearest-image
    distances (aggf_gb_distance_range_cell)."""
    stride, images = _gb_box("gb_distance_range", box, Pg, near)
    if Pg.dtype != torch.float32:
        Pg, cg = Pg.to(torch.float32), cg.to(torch.float32)
        box = None if box is None else box.to(torch.float32)
    T, G, _ = Pg.shape
    n_cg = cg.shape[1]
    rmin = torch.full((n_cg, G), float("inf"), dtype=torch.float32, device=Pg.device)
    rmax = torch.zeros((n_cg, G), dtype=torch.float32, device=Pg.device)
    if T and n_ch:
        if box is None:
            check(lib().aggf_gb_distance_range(ptr(Pg), ptr(cg), T, G, n_cg, n_ch, ptr(rmin), ptr(rmax), stream_ptr()),
                  "aggf_gb_distance_range")
        elif images is not None:
            check(lib().aggf_gb_distance_range_cell(ptr(Pg), ptr(cg), T, G, n_cg, n_ch, ptr(box), ptr(rmin), ptr(rmax),
                                                    stream_ptr(), images), "aggf_gb_distance_range_cell")
        else:
            check(lib().aggf_gb_distance_range_pbc(ptr(Pg), ptr(cg), T, G, n_cg, n_ch, ptr(box), stride, ptr(rmin),
                                                   ptr(rmax), stream_ptr()), "aggf_gb_distance_range_pbc")
    return rmin, rmax


def gb_regmat_cols(Fg, Pg, cg, site: int, sizes, n_id: int, cols: torch.Tensor, centers, width: float, clip: float,
                   kbt: float, out: torch.Tensor, box: Optional[torch.Tensor] = None, near: bool = False) -> torch.Tensor:
    """Compact regression matrix of one cg site (listed Gaussian columns only); see aggf_gb_regmat_cols, and
    aggf_gb_regmat_cols_pbc / aggf_gb_regmat_cols_cell for ``box`` and ``near`` (as ``gb_channels``)."""
    T, G, _ = Fg.shape
    stride, images = _gb_box("gb_regmat_cols", box, Pg, near)
    with _timed("gb_regmat"):
        if box is None:
            check(
                lib().aggf_gb_regmat_cols(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg), _gb_dtype(Pg, cg, centers), T,
                                          G, cg.shape[1], site,
                                          ptr(sizes), n_id, ptr(cols), int(cols.numel()), ptr(centers), centers.numel(),
                                          float(width), float(clip), float(kbt), out.shape[1], ptr(out),
                                          dtype_code(out.dtype), stream_ptr()),
                "aggf_gb_regmat_cols",
            )
        elif images is not None:
            check(
                lib().aggf_gb_regmat_cols_cell(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg),
                                               _gb_dtype(Pg, cg, centers), T, G, cg.shape[1], site, ptr(sizes), n_id,
                                               ptr(cols), int(cols.numel()), ptr(centers), centers.numel(),
                                               float(width), float(clip), float(kbt), out.shape[1], ptr(box), ptr(out),
                                               dtype_code(out.dtype), stream_ptr(), images),
                "aggf_gb_regmat_cols_cell",
            )
        else:
            check(
                lib().aggf_gb_regmat_cols_pbc(ptr(Fg), dtype_code(Fg.dtype), ptr(Pg), ptr(cg),
                                              _gb_dtype(Pg, cg, centers), T, G, cg.shape[1], site, ptr(sizes), n_id,
                                              ptr(cols), int(cols.numel()), ptr(centers), centers.numel(), float(width),
                                              float(clip), float(kbt), out.shape[1], ptr(box), stride, ptr(out),
                                              dtype_code(out.dtype), stream_ptr()),
                "aggf_gb_regmat_cols_pbc",
            )
    return out


def feat_weights(feat: torch.Tensor, coef: torch.Tensor, out: torch.Tensor, site: int) -> None:
    """out[:, site, :] (T, n_cg, N float64) = feat (T, N, n_feat) . coef (n_feat); see aggf_feat_weights."""
    T, N, n_feat = feat.shape
    n_cg = out.shape[1]
    if T == 0:
        return
    view = out[:, site, :]
    check(lib().aggf_feat_weights(ptr(feat), dtype_code(feat.dtype), T, N, n_feat, ptr(coef), n_cg * N, view.data_ptr(),
                                  stream_ptr()), "aggf_feat_weights")


# ------------------------------------------------------------------ K6 pair-distance variance


def pair_dist_var(x: torch.Tensor, box: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(N, N) float64 population variance over frames of every pair distance; see aggf_pair_dist_var.  ``box`` ((3,)
    or (T, 3), x's dtype and device): the distances are those of the minimum image under that orthorhombic box
    (aggf_pair_dist_var_pbc); a frame whose box is bad makes every off-diagonal element NaN.  (T, 9): the rows of a
    triclinic cell (``pbc.Cell.rows``), the brick image."""
    l = lib()
    T, N, _ = x.shape
    stride = None if box is None else _box_arg("pair_dist_var", box, x, cell=True)
    var = torch.empty((N, N), dtype=torch.float64, device=x.device)
    need = l.aggf_pair_dist_var_workspace_bytes(T, N)
    ws = workspace(need, x.device, "pairs")
    with _timed("pair_var"):
        if box is None:
            check(l.aggf_pair_dist_var(ptr(x), T, N, dtype_code(x.dtype), ptr(var), ptr(ws), need, stream_ptr()),
                  "aggf_pair_dist_var")
        else:
            check(l.aggf_pair_dist_var_pbc(ptr(x), T, N, dtype_code(x.dtype), ptr(box), stride, ptr(var), ptr(ws), need,
                                           stream_ptr()), "aggf_pair_dist_var_pbc")
    return var


def pair_dist_moments(x: torch.Tensor, box: Optional[torch.Tensor] = None):
    """(mean, var) (N, N) float64 of every pair distance over the frames; see aggf_pair_dist_moments.  ``box``: as
    ``pair_dist_var`` (aggf_pair_dist_moments_pbc)."""
    l = lib()
    T, N, _ = x.shape
    stride = None if box is None else _box_arg("pair_dist_moments", box, x, cell=True)
    mean = torch.empty((N, N), dtype=torch.float64, device=x.device)
    var = torch.empty((N, N), dtype=torch.float64, device=x.device)
    need = l.aggf_pair_dist_var_workspace_bytes(T, N)
    ws = workspace(need, x.device, "pairs")
    with _timed("pair_var"):
        if box is None:
            check(l.aggf_pair_dist_moments(ptr(x), T, N, dtype_code(x.dtype), ptr(mean), ptr(var), ptr(ws), need,
                                           stream_ptr()), "aggf_pair_dist_moments")
        else:
            check(l.aggf_pair_dist_moments_pbc(ptr(x), T, N, dtype_code(x.dtype), ptr(box), stride, ptr(mean), ptr(var),
                                               ptr(ws), need, stream_ptr()), "aggf_pair_dist_moments_pbc")
    return mean, var


def pair_pool_term(var_r: torch.Tensor, mean_r: torch.Tensor, mean: torch.Tensor, weight: float) -> torch.Tensor:
    """weight * (var_r + (mean_r - mean)^2), in place of var_r; see aggf_pair_pool_term."""
    check(lib().aggf_pair_pool_term(ptr(var_r), ptr(mean_r), ptr(mean), float(weight), var_r.numel(), ptr(var_r),
                                    stream_ptr()), "aggf_pair_pool_term")
    return var_r


# ------------------------------------------------------------------ K7 map validation


def gauss_pair_forces(x: torch.Tensor, offset: float, width: float, want_forces: bool = True,
                      want_energies: bool = False, box: Optional[torch.Tensor] = None, near: bool = False):
    """(G (T, n, 3) or None, E (T,) or None) in x's dtype for one squared-distance Gaussian; see aggf_gauss_pair_forces.
    ``box`` ((3,), (T, 3) or the (T, 9) rows of a cell, in x's dtype): every r_i - r_j is its image under it.  ``near``
    (with the rows of a cell): the nearest image instead of the brick image (aggf_gauss_pair_forces_cell)."""
    l = lib()
    T, n, _ = x.shape
    stride = 0 if box is None else _box_arg("gauss_pair_forces", box, x, cell=True, near=near)
    G = torch.empty_like(x) if want_forces else None
    E = torch.empty(T, dtype=x.dtype, device=x.device) if want_energies else None
    if x.numel() == 0:
        return G, E
    need = l.aggf_gauss_pair_forces_workspace_bytes(T, n) if want_energies else 0
    ws = workspace(need, x.device, "mapval") if want_energies else None
    with _timed("gauss_forces"):
        if near:
            check(l.aggf_gauss_pair_forces_cell(ptr(x), T, n, dtype_code(x.dtype), float(offset), float(width), ptr(box),
                                                ptr(G), ptr(E), ptr(ws), need, stream_ptr(), IMAGES_NEAREST),
                  "aggf_gauss_pair_forces_cell")
            return G, E
        check(l.aggf_gauss_pair_forces(ptr(x), T, n, dtype_code(x.dtype), float(offset), float(width), ptr(box), stride,
                                       ptr(G), ptr(E), ptr(ws), need, stream_ptr()), "aggf_gauss_pair_forces")
    return G, E


def gauss_proj(x: torch.Tensor, f: torch.Tensor, offsets: torch.Tensor, width: float,
               box: Optional[torch.Tensor] = None, near: bool = False) -> torch.Tensor:
    """(S,) float64: sum over frames and sites of F . G_s for every offset; see aggf_gauss_proj.  ``box``, ``near``:
    as ``gauss_pair_forces`` (aggf_gauss_proj_cell)."""
    l = lib()
    T, n, _ = x.shape
    stride = 0 if box is None else _box_arg("gauss_proj", box, x, cell=True, near=near)
    S = offsets.numel()
    out = torch.empty(S, dtype=torch.float64, device=x.device)
    need = l.aggf_gauss_proj_workspace_bytes(T, n, S)
    ws = workspace(need, x.device, "mapval")
    with _timed("gauss_proj"):
        if near:
            check(l.aggf_gauss_proj_cell(ptr(x), dtype_code(x.dtype), ptr(f), dtype_code(f.dtype), T, n, ptr(offsets), S,
                                         float(width), ptr(box), ptr(out), ptr(ws), need, stream_ptr(), IMAGES_NEAREST),
                  "aggf_gauss_proj_cell")
            return out
        check(l.aggf_gauss_proj(ptr(x), dtype_code(x.dtype), ptr(f), dtype_code(f.dtype), T, n, ptr(offsets), S,
                                float(width), ptr(box), stride, ptr(out), ptr(ws), need, stream_ptr()),
              "aggf_gauss_proj")
    return out


def gauss_shift(x: torch.Tensor, f: torch.Tensor, offsets: torch.Tensor, width: float,
                box: Optional[torch.Tensor] = None, near: bool = False):
    """((S,), (S,)) float64: sum F . G_s and sum |G_s|^2 for every offset, one pass; see aggf_gauss_shift.  ``box``,
    ``near``: as ``gauss_pair_forces`` (aggf_gauss_shift_cell)."""
    l = lib()
    T, n, _ = x.shape
    stride = 0 if box is None else _box_arg("gauss_shift", box, x, cell=True, near=near)
    S = offsets.numel()
    ip = torch.empty(S, dtype=torch.float64, device=x.device)
    gsq = torch.empty(S, dtype=torch.float64, device=x.device)
    need = l.aggf_gauss_shift_workspace_bytes(T, n, S)
    ws = workspace(need, x.device, "mapval")
    with _timed("gauss_shift"):
        if near:
            check(l.aggf_gauss_shift_cell(ptr(x), dtype_code(x.dtype), ptr(f), dtype_code(f.dtype), T, n, ptr(offsets),
                                          S, float(width), ptr(box), ptr(ip), ptr(gsq), ptr(ws), need, stream_ptr(), IMAGES_NEAREST),
                  "aggf_gauss_shift_cell")
            return ip, gsq
        check(l.aggf_gauss_shift(ptr(x), dtype_code(x.dtype), ptr(f), dtype_code(f.dtype), T, n, ptr(offsets), S,
                                 float(width), ptr(box), stride, ptr(ip), ptr(gsq), ptr(ws), need, stream_ptr()),
              "aggf_gauss_shift")
    return ip, gsq


def dot(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Device scalar (shape (1,), float64): sum a * b over equally sized arrays, fixed summation order."""
    l = lib()
    assert a.numel() == b.numel() and a.is_contiguous() and b.is_contiguous()
    out = torch.zeros(1, dtype=torch.float64, device=a.device)
    if a.numel() == 0:
        return out
    need = l.aggf_dot_workspace_bytes()
    ws = workspace(need, a.device, "dot")
    check(l.aggf_dot(ptr(a), dtype_code(a.dtype), ptr(b), dtype_code(b.dtype), a.numel(), ptr(out), ptr(ws), need,
                     stream_ptr()), "aggf_dot")
    return out


# ------------------------------------------------------------------ K8 backward contractions (aggforce_amd/_autograd.py)


def trjdot_cross(a: torch.Tensor, b: torch.Tensor, out_dtype: torch.dtype, out: Optional[torch.Tensor] = None,
                 accumulate: bool = False) -> torch.Tensor:
    """(n_a, n_b) in out_dtype: sum over frames and dimensions of a[t,i,d] b[t,j,d] (aggf_trjdot_cross; ``accumulate``
    adds to ``out``).  a and b must share a dtype: widen one of them first."""
    l = lib()
    T, n_a, _ = a.shape
    n_b = b.shape[1]
    if a.dtype != b.dtype or tuple(b.shape) != (T, n_b, 3) or a.shape[2] != 3:
        raise ValueError(f"trjdot_cross: operands {tuple(a.shape)} {a.dtype}, {tuple(b.shape)} {b.dtype}")
    if out is None:
        out = (torch.zeros if accumulate else torch.empty)((n_a, n_b), dtype=out_dtype, device=a.device)
    if T == 0 or n_a == 0 or n_b == 0:
        if not accumulate:
            out.zero_()
        return out
    need = l.aggf_trjdot_cross_workspace_bytes(T, n_a, n_b, dtype_code(a.dtype))
    ws = workspace(need, a.device, "trjgrad")
    with _timed("trjdot_cross"):
        check(l.aggf_trjdot_cross(ptr(a), ptr(b), T, n_a, n_b, dtype_code(a.dtype), ptr(out), dtype_code(out.dtype),
                                  int(accumulate), ptr(ws), need, stream_ptr()), "aggf_trjdot_cross")
    return out


def trjdot_frames_t(g: torch.Tensor, f: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """out[t,a,d] = sum_c f[t,c,a] g[t,c,d] -> (T, N, 3) in out_dtype (aggf_trjdot_frames_t); g and f share a dtype
    at least as wide as out_dtype."""
    T, n_cg, N = f.shape
    if tuple(g.shape) != (T, n_cg, 3) or g.dtype != f.dtype:
        raise ValueError(f"trjdot_frames_t: operands {tuple(g.shape)} {g.dtype}, {tuple(f.shape)} {f.dtype}")
    out = torch.empty((T, N, 3), dtype=out_dtype, device=g.device)
    if n_cg == 0:
        return out.zero_()
    if T == 0 or N == 0:
        return out
    with _timed("trjdot_frames_t"):
        check(lib().aggf_trjdot_frames_t(ptr(g), ptr(f), dtype_code(g.dtype), T, n_cg, N, ptr(out),
                                         dtype_code(out_dtype), stream_ptr()), "aggf_trjdot_frames_t")
    return out


def trjdot_frames_outer(g: torch.Tensor, p: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """out[t,c,a] = sum_d g[t,c,d] p[t,a,d] -> (T, n_cg, N) in out_dtype (aggf_trjdot_frames_outer); g and p share a
    dtype at least as wide as out_dtype."""
    T, n_cg, _ = g.shape
    N = p.shape[1]
    if tuple(p.shape) != (T, N, 3) or g.shape[2] != 3 or g.dtype != p.dtype:
        raise ValueError(f"trjdot_frames_outer: operands {tuple(g.shape)} {g.dtype}, {tuple(p.shape)} {p.dtype}")
    out = torch.empty((T, n_cg, N), dtype=out_dtype, device=g.device)
    if T == 0 or n_cg == 0 or N == 0:
        return out
    with _timed("trjdot_frames_outer"):
        check(lib().aggf_trjdot_frames_outer(ptr(g), ptr(p), dtype_code(g.dtype), T, n_cg, N, ptr(out),
                                             dtype_code(out_dtype), stream_ptr()), "aggf_trjdot_frames_outer")
    return out


# ------------------------------------------------------------------ K9 pair distances (aggforce_amd/_autograd.py)
PAIR_DIST, PAIR_SQDIST, PAIR_DOT = 0, 1, 2
IMAGES_BRICK, IMAGES_NEAREST = 0, 1  # AGGF_IMAGES_*: the image selector of the ``_cell`` entries


def _pair_sites(name: str, x: torch.Tensor, c: torch.Tensor):
    """(T, m, n) of X (T, n, 3) and C (T, m, 3), which must share a float dtype and be contiguous."""
    if (x.dim() != 3 or c.dim() != 3 or x.shape[2] != 3 or c.shape[2] != 3 or x.shape[0] != c.shape[0]
            or x.dtype != c.dtype or x.dtype not in (torch.float32, torch.float64)):
        raise ValueError(f"{name}: operands {tuple(x.shape)} {x.dtype}, {tuple(c.shape)} {c.dtype}")
    if not (x.is_contiguous() and c.is_contiguous()):
        raise ValueError(f"{name}: operands must be contiguous")
    return x.shape[0], c.shape[1], x.shape[1]


def pair_dist(x: torch.Tensor, c: torch.Tensor, mode: int = PAIR_DIST, v: Optional[torch.Tensor] = None,
              y: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(T, m, n) in the operands' dtype over u[t,i,j] = x[t,j] - c[t,i] (aggf_pair_dist): |u| (PAIR_DIST), u.u
    (PAIR_SQDIST) or (v[t,j] - y[t,i]).u (PAIR_DOT, v shaped as x and y as c).  All operands share a dtype."""
    T, m, n = _pair_sites("pair_dist", x, c)
    if mode not in (PAIR_DIST, PAIR_SQDIST, PAIR_DOT):
        raise ValueError(f"pair_dist: mode {mode}")
    if mode == PAIR_DOT:
        if v is None or y is None or (T, m, n) != _pair_sites("pair_dist", v, y) or v.dtype != x.dtype:
            raise ValueError("pair_dist: PAIR_DOT needs v shaped as x and y shaped as c, in their dtype")
    else:
        v = y = None
    out = torch.empty((T, m, n), dtype=x.dtype, device=x.device)
    if out.numel() == 0:
        return out
    with _timed("pair_dist"):
        check(lib().aggf_pair_dist(ptr(x), ptr(c), ptr(v), ptr(y), T, m, n, dtype_code(x.dtype), mode, ptr(out),
                                   stream_ptr()), "aggf_pair_dist")
    return out


def pair_pull(w: torch.Tensor, x: torch.Tensor, c: torch.Tensor, dv: Optional[torch.Tensor] = None,
              want_a: bool = True, want_b: bool = True, out_dtype: Optional[torch.dtype] = None):
    """(A, B): A[t,j,:] = sum_i w_ij u_ij (T, n, 3) and B[t,i,:] = -sum_j w_ij u_ij (T, m, 3) over u[t,i,j] =
    x[t,j] - c[t,i], with the weights w (T, m, n) or, given ``dv``, (dv > 0 ? w / dv : 0) (aggf_pair_pull: one pass
    over w for both).  An output that is not wanted is None and costs nothing.  All operands share a dtype at least
    as wide as out_dtype (default: theirs)."""
    T, m, n = _pair_sites("pair_pull", x, c)
    out_dtype = out_dtype or x.dtype
    for name, arr in (("w", w), ("dv", dv)):
        if arr is not None and (tuple(arr.shape) != (T, m, n) or arr.dtype != x.dtype or not arr.is_contiguous()):
            raise ValueError(f"pair_pull: {name} {tuple(arr.shape)} {arr.dtype} for sites {tuple(x.shape)} "
                             f"{tuple(c.shape)} {x.dtype} (contiguous arrays of one dtype)")
    if x.dtype == torch.float32 and out_dtype == torch.float64:
        raise ValueError("pair_pull: float32 operands with float64 outputs: widen the operands")
    a = torch.empty((T, n, 3), dtype=out_dtype, device=x.device) if want_a else None
    b = torch.empty((T, m, 3), dtype=out_dtype, device=x.device) if want_b else None
    if T * m * n == 0:  # empty sums
        return (a.zero_() if want_a else None), (b.zero_() if want_b else None)
    if not (want_a or want_b):
        return None, None
    l = lib()
    need = l.aggf_pair_pull_workspace_bytes(T, m, n, dtype_code(x.dtype)) if want_b else 0
    ws = workspace(need, x.device, "pairdist") if need else None
    with _timed("pair_pull"):
        check(l.aggf_pair_pull(ptr(w), ptr(dv), ptr(x), ptr(c), T, m, n, dtype_code(x.dtype), ptr(a), ptr(b),
                               dtype_code(out_dtype), ptr(ws), need, stream_ptr()), "aggf_pair_pull")
    return a, b


# ------------------------------------------------------------------ K9c / K9d pair lists (aggforce_amd/_autograd.py)
class PairTables:
    """A pair list on one device (built by ``jaxutil.PairList``): ``pairs`` (P, 2) int32, row p = (i_p, j_p), and the
    two incidence tables in CSR form, by j over ``n`` sites (``a_ptr`` (n + 1,), ``a_idx`` (P,)) and by i over ``m``
    sites (``b_ptr``, ``b_idx``), entries in ascending pair index; ``max_deg_a`` / ``max_deg_b``: their longest runs."""

    def __init__(self, pairs, a_ptr, a_idx, b_ptr, b_idx, max_deg_a: int, max_deg_b: int, m: int, n: int):
        self.pairs, self.a_ptr, self.a_idx, self.b_ptr, self.b_idx = pairs, a_ptr, a_idx, b_ptr, b_idx
        self.max_deg_a, self.max_deg_b, self.m, self.n = int(max_deg_a), int(max_deg_b), int(m), int(n)
        self.n_pairs = int(pairs.shape[0])


def _pair_list_sites(name: str, x: torch.Tensor, c: torch.Tensor, tab: PairTables):
    T, m, n = _pair_sites(name, x, c)
    if (m, n) != (tab.m, tab.n) or tab.pairs.device != x.device:
        raise ValueError(f"{name}: a pair list for ({tab.m}, {tab.n}) sites on {tab.pairs.device} with operands "
                         f"{tuple(x.shape)}, {tuple(c.shape)} on {x.device}")
    return T, m, n, tab.n_pairs


def _box_arg(name: str, box: torch.Tensor, x: torch.Tensor, cell: bool = False, near: bool = False) -> int:
    """The element stride between the frames of ``box`` (the ``box_stride`` of include/aggf.h): 3 for (T, 3), 0 for
    (3,); a contiguous tensor in the dtype and on the device of ``x``.  ``cell``: the entry also takes (T, 9), a
    row-major 3 x 3 triclinic cell per frame (``pbc.Cell.rows``), stride 9.  ``near`` (the
    nearest image of a cell, the ``_cell`` entries with AGGF_IMAGES_NEAREST): ``box`` must be those (T, 9) rows."""
    T = x.shape[0]
    if near and (not isinstance(box, torch.Tensor) or tuple(box.shape) != (T, 9)):
        raise ValueError(f"{name}: the nearest image needs the ({T}, 9) rows of a cell; got "
                         f"{tuple(box.shape) if hasattr(box, 'shape') else type(box)}")
    shapes = ((3,), (T, 3), (T, 9)) if cell else ((3,), (T, 3))
    if (not isinstance(box, torch.Tensor) or box.dtype != x.dtype or box.device != x.device or not box.is_contiguous()
            or tuple(box.shape) not in shapes):
        raise ValueError(f"{name}: box must be a contiguous {x.dtype} tensor of shape (3,) or ({T}, 3)"
                         f"{f' or ({T}, 9)' if cell else ''} on {x.device}; "
                         f"got {tuple(box.shape) if hasattr(box, 'shape') else type(box)} "
                         f"{getattr(box, 'dtype', '')} on {getattr(box, 'device', '')}")
    return int(box.shape[1]) if box.dim() == 2 else 0


def pair_list_dist(x: torch.Tensor, c: torch.Tensor, tab: PairTables, mode: int = PAIR_DIST,
                   v: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None,
                   box: Optional[torch.Tensor] = None, near: bool = False) -> torch.Tensor:
    """(T, P) in the operands' dtype over u[t,p] = x[t,j_p] - c[t,i_p] (aggf_pair_list_dist): |u|, u.u or
    (v[t,j_p] - y[t,i_p]).u by ``mode``, as ``pair_dist``.  ``box`` ((3,) or (T, 3), the operands' dtype): u is its
    minimum image under that orthorhombic box (aggf_pair_list_dist_pbc); v - y is never wrapped.  (T, 9): the rows of
    a triclinic cell (``pbc.Cell.rows``), u is its brick image or, with ``near``, its nearest image
    (aggf_pair_list_dist_cell)."""
    T, m, n, P = _pair_list_sites("pair_list_dist", x, c, tab)
    stride = None if box is None else _box_arg("pair_list_dist", box, x, cell=True, near=near)
    if mode not in (PAIR_DIST, PAIR_SQDIST, PAIR_DOT):
        raise ValueError(f"pair_list_dist: mode {mode}")
    if mode == PAIR_DOT:
        if v is None or y is None or (T, m, n) != _pair_sites("pair_list_dist", v, y) or v.dtype != x.dtype:
            raise ValueError("pair_list_dist: PAIR_DOT needs v shaped as x and y shaped as c, in their dtype")
    else:
        v = y = None
    out = torch.empty((T, P), dtype=x.dtype, device=x.device)
    if out.numel() == 0:
        return out
    with _timed("pair_list_dist"):
        if near:
            check(lib().aggf_pair_list_dist_cell(ptr(x), ptr(c), ptr(v), ptr(y), ptr(tab.pairs), T, m, n, P,
                                                 dtype_code(x.dtype), mode, ptr(box), ptr(out), stream_ptr(), IMAGES_NEAREST),
                  "aggf_pair_list_dist_cell")
        elif box is None:
            check(lib().aggf_pair_list_dist(ptr(x), ptr(c), ptr(v), ptr(y), ptr(tab.pairs), T, m, n, P,
                                            dtype_code(x.dtype), mode, ptr(out), stream_ptr()), "aggf_pair_list_dist")
        else:
            check(lib().aggf_pair_list_dist_pbc(ptr(x), ptr(c), ptr(v), ptr(y), ptr(tab.pairs), T, m, n, P,
                                                dtype_code(x.dtype), mode, ptr(box), stride, ptr(out), stream_ptr()),
                  "aggf_pair_list_dist_pbc")
    return out


def pair_list_pull(w: torch.Tensor, x: torch.Tensor, c: torch.Tensor, tab: PairTables,
                   dv: Optional[torch.Tensor] = None, want_a: bool = True, want_b: bool = True,
                   out_dtype: Optional[torch.dtype] = None, box: Optional[torch.Tensor] = None,
                   near: bool = False):
    """(A, B): A[t,j,:] = sum_{p: j_p = j} w_p u_p (T, n, 3) and B[t,i,:] = -sum_{p: i_p = i} w_p u_p (T, m, 3) over
    u[t,p] = x[t,j_p] - c[t,i_p], with the weights w (T, P) or, given ``dv``, (dv > 0 ? w / dv : 0)
    (aggf_pair_list_pull).  An output that is not wanted is None and costs nothing.  All operands share a dtype at
    least as wide as out_dtype (default: theirs).  ``box``, ``near``: as ``pair_list_dist`` (aggf_pair_list_pull_pbc,
    aggf_pair_list_pull_cell)."""
    T, m, n, P = _pair_list_sites("pair_list_pull", x, c, tab)
    stride = None if box is None else _box_arg("pair_list_pull", box, x, cell=True, near=near)
    out_dtype = out_dtype or x.dtype
    for name, arr in (("w", w), ("dv", dv)):
        if arr is not None and (tuple(arr.shape) != (T, P) or arr.dtype != x.dtype or not arr.is_contiguous()):
            raise ValueError(f"pair_list_pull: {name} {tuple(arr.shape)} {arr.dtype} for {P} pairs of sites "
                             f"{tuple(x.shape)} {tuple(c.shape)} {x.dtype} (contiguous arrays of one dtype)")
    if x.dtype == torch.float32 and out_dtype == torch.float64:
        raise ValueError("pair_list_pull: float32 operands with float64 outputs: widen the operands")
    a = torch.empty((T, n, 3), dtype=out_dtype, device=x.device) if want_a else None
    b = torch.empty((T, m, 3), dtype=out_dtype, device=x.device) if want_b else None
    if T * P == 0 or T * m * n == 0:  # empty sums
        return (a.zero_() if want_a else None), (b.zero_() if want_b else None)
    if not (want_a or want_b):
        return None, None
    with _timed("pair_list_pull"):
        if near:
            check(lib().aggf_pair_list_pull_cell(ptr(w), ptr(dv), ptr(x), ptr(c), ptr(tab.pairs), ptr(tab.a_ptr),
                                                 ptr(tab.a_idx), ptr(tab.b_ptr), ptr(tab.b_idx), tab.max_deg_a,
                                                 tab.max_deg_b, T, m, n, P, dtype_code(x.dtype), ptr(box), ptr(a), ptr(b),
                                                 dtype_code(out_dtype), stream_ptr(), IMAGES_NEAREST), "aggf_pair_list_pull_cell")
        elif box is None:
            check(lib().aggf_pair_list_pull(ptr(w), ptr(dv), ptr(x), ptr(c), ptr(tab.pairs), ptr(tab.a_ptr),
                                            ptr(tab.a_idx), ptr(tab.b_ptr), ptr(tab.b_idx), tab.max_deg_a,
                                            tab.max_deg_b, T, m, n, P, dtype_code(x.dtype), ptr(a), ptr(b),
                                            dtype_code(out_dtype), stream_ptr()), "aggf_pair_list_pull")
        else:
            check(lib().aggf_pair_list_pull_pbc(ptr(w), ptr(dv), ptr(x), ptr(c), ptr(tab.pairs), ptr(tab.a_ptr),
                                                ptr(tab.a_idx), ptr(tab.b_ptr), ptr(tab.b_idx), tab.max_deg_a,
                                                tab.max_deg_b, T, m, n, P, dtype_code(x.dtype), ptr(box), stride,
                                                ptr(a), ptr(b), dtype_code(out_dtype), stream_ptr()),
                  "aggf_pair_list_pull_pbc")
    return a, b


def pair_min(x: torch.Tensor, c: torch.Tensor, square: bool = False, box: Optional[torch.Tensor] = None,
             near: bool = False) -> torch.Tensor:
    """(m, n) in the operands' dtype: out[i,j] = min_t |x[t,j] - c[t,i]| (``square``: squared), the minimum image
    under ``box`` if given (aggf_pair_min, K9e; ``near`` with the rows of a cell: the nearest image,
    aggf_pair_min_cell).  A NaN distance makes its pair NaN; without frames every minimum is +inf (the empty minimum)."""
    T, m, n = _pair_sites("pair_min", x, c)
    stride = 0 if box is None else _box_arg("pair_min", box, x, cell=True, near=near)
    if T == 0:
        return torch.full((m, n), float("inf"), dtype=x.dtype, device=x.device)
    out = torch.empty((m, n), dtype=x.dtype, device=x.device)
    if out.numel() == 0:
        return out
    l = lib()
    need = l.aggf_pair_min_workspace_bytes(T, m, n, dtype_code(x.dtype))
    ws = workspace(need, x.device, "pairmin") if need else None
    with _timed("pair_min"):
        if near:
            check(l.aggf_pair_min_cell(ptr(x), ptr(c), T, m, n, dtype_code(x.dtype), ptr(box), int(bool(square)),
                                       ptr(out), ptr(ws), need, stream_ptr(), IMAGES_NEAREST), "aggf_pair_min_cell")
            return out
        check(l.aggf_pair_min(ptr(x), ptr(c), T, m, n, dtype_code(x.dtype), ptr(box), stride, int(bool(square)),
                              ptr(out), ptr(ws), need, stream_ptr()), "aggf_pair_min")
    return out


# ------------------------------------------------------------------ K11 whole molecules (aggforce_amd/pbc.py)
WHOLE_AUTO, WHOLE_LDS, WHOLE_GLOBAL = 0, 1, 2
_WHOLE_WS_BYTES = 256 << 20  # the global form's count buffers: frames beyond this go in further calls


class TreeTables:
    """A spanning forest on one device (built by ``pbc.MoleculeTree``): ``parent`` (N,) int32, -1 a root, and
    ``jumps`` (rounds, N) int32, jumps[r][i] the 2^r-th ancestor of i or -1."""

    def __init__(self, parent: torch.Tensor, jumps: torch.Tensor):
        self.parent, self.jumps = parent, jumps
        self.n, self.rounds = int(parent.shape[0]), int(jumps.shape[0])


def whole_lds_max_sites() -> int:
    """The largest number of atoms the LDS form of K11 takes (no GPU needed)."""
    return int(_lib.load().aggf_make_whole_lds_max_sites())


def make_whole(x: torch.Tensor, box: torch.Tensor, tree: TreeTables, out: Optional[torch.Tensor] = None,
               images: Optional[torch.Tensor] = None, _form: int = WHOLE_AUTO) -> torch.Tensor:
    """(T, N, 3): x with every molecule of ``tree`` made whole under ``box`` ((3,) or (T, 3), or the (T, 9) rows of a
    triclinic cell; x's dtype), K11
    (aggf_make_whole).  ``out``: where to write (x itself: in place; default a new tensor); ``images``: a (T, N, 3)
    int32 tensor that receives the image counts.  ``_form`` (tests, benchmarks): WHOLE_LDS or WHOLE_GLOBAL instead of
    the library's choice."""
    if x.dim() != 3 or x.shape[2] != 3 or x.dtype not in (torch.float32, torch.float64) or not x.is_contiguous():
        raise ValueError(f"make_whole: x {tuple(x.shape)} {x.dtype} must be a contiguous (T, N, 3) float32/float64 tensor")
    stride = _box_arg("make_whole", box, x, cell=True)
    T, N = int(x.shape[0]), int(x.shape[1])
    if N != tree.n or tree.parent.device != x.device:
        raise ValueError(f"make_whole: a tree over {tree.n} atoms on {tree.parent.device} with x {tuple(x.shape)} on "
                         f"{x.device}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError("make_whole: out must match x in shape, dtype and device, and be contiguous")
    if images is not None and (tuple(images.shape) != tuple(x.shape) or images.dtype != torch.int32
                               or images.device != x.device or not images.is_contiguous()):
        raise ValueError("make_whole: images must be a contiguous int32 tensor of x's shape on x's device")
    if _form not in (WHOLE_AUTO, WHOLE_LDS, WHOLE_GLOBAL):
        raise ValueError(f"make_whole: form {_form}")
    if T == 0 or N == 0:
        return out
    l = lib()
    code = dtype_code(x.dtype)
    jumps = tree.jumps if tree.rounds else None
    # (a triclinic frame stages nine numbers in LDS where a box stages six: the LDS form takes one atom fewer)
    in_lds = _form == WHOLE_LDS or (_form == WHOLE_AUTO and N <= whole_lds_max_sites() - (1 if stride == 9 else 0))
    # frames per call: all of them, or what keeps the global form's counts within _WHOLE_WS_BYTES
    step = T if in_lds else max(1, min(T, _WHOLE_WS_BYTES // max(1, l.aggf_make_whole_workspace_bytes(1, N, tree.rounds, code))))
    need = 0 if in_lds else l.aggf_make_whole_workspace_bytes(step, N, tree.rounds, code)
    ws = workspace(need, x.device, "whole") if need else None
    with _timed("make_whole"):
        for t0 in range(0, T, step):
            n = min(step, T - t0)
            check(l.aggf_make_whole(ptr(x[t0:]), n, N, code, ptr(tree.parent), ptr(jumps), tree.rounds,
                                    ptr(box[t0:] if stride else box), stride, ptr(out[t0:]),
                                    None if images is None else ptr(images[t0:]), ptr(ws), need, _form, stream_ptr()),
                  "aggf_make_whole")
    return out


# ------------------------------------------------------------------ K10 Gaussian radial basis (aggforce_amd/_autograd.py)
GB_H_ELEM, GB_H_ROW, GB_H_SLOT = 0, 1, 2


class BasisSpec:
    """The constants of one Gaussian basis on one device: ``centers`` (n_basis,) in the dtype of the distances, ``width``
    and ``clip`` (None: no clipping, the arithmetic of clip = 0), and optionally the channel slots of the sites
    (``channels``: one integer per site; a channel outside [0, n_slots) is dropped).  ``order`` / ``start``: the kept
    sites sorted by slot and each slot's range in that list (what the channel sum walks)."""

    def __init__(self, centers: torch.Tensor, width: float, clip: Optional[float], channels=None,
                 n_slots: Optional[int] = None):
        if centers.dim() != 1 or centers.numel() < 1 or centers.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"BasisSpec: centers {tuple(centers.shape)} {centers.dtype}")
        self.centers = centers.contiguous()
        self.n_basis = int(centers.numel())
        self.width = float(width)
        self.clip = 0.0 if clip is None else float(clip)
        if not self.width > 0 or not self.clip >= 0:
            raise ValueError(f"BasisSpec: width {width} must be positive and clip {clip} non-negative")
        self.slot = self.order = self.start = None
        self.n_sites, self.n_slots, self.n_order = 1, 1, 0
        if channels is not None:
            ch = np.asarray(channels, dtype=np.int64).reshape(-1)
            self.n_sites, self.n_slots = int(ch.size), int(n_slots)
            if self.n_sites < 1 or self.n_slots < 1:
                raise ValueError(f"BasisSpec: {self.n_sites} sites in {self.n_slots} slots")
            kept = (ch >= 0) & (ch < self.n_slots)
            slot = np.where(kept, ch, -1).astype(np.int32)
            order = np.flatnonzero(kept)
            order = order[np.argsort(slot[order], kind="stable")].astype(np.int32)
            start = np.zeros(self.n_slots + 1, dtype=np.int32)
            start[1:] = np.cumsum(np.bincount(slot[order], minlength=self.n_slots))
            dev = centers.device
            self.slot = torch.from_numpy(slot).to(dev)
            self.order = torch.from_numpy(order if order.size else np.zeros(1, np.int32)).to(dev)
            self.n_order = int(order.size)
            self.start = torch.from_numpy(start).to(dev)

    @property
    def row(self) -> int:
        return self.n_slots * self.n_basis


def _basis_operand(name: str, x: Optional[torch.Tensor], spec: BasisSpec, shape=None) -> None:
    if x is None:
        return
    if x.dtype != spec.centers.dtype or x.device != spec.centers.device or not x.is_contiguous():
        raise ValueError(f"{name}: {tuple(x.shape)} {x.dtype} on {x.device} (contiguous, {spec.centers.dtype}, "
                         f"on {spec.centers.device})")
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(x.shape)}, expected {tuple(shape)}")


def _basis_sites(name: str, d: torch.Tensor, spec: BasisSpec) -> None:
    if spec.slot is not None and (d.dim() < 1 or d.shape[-1] != spec.n_sites):
        raise ValueError(f"{name}: distances {tuple(d.shape)} for {spec.n_sites} sites with channels")


def gbasis_expand(d: torch.Tensor, spec: BasisSpec, q: int = 0, s: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d.shape + (row,): out[e, col0(e) + k] = s[e] g_k^(q)(d[e]) (aggf_gbasis_expand); row = n_basis, or with slots
    n_slots * n_basis with zeros outside the site's block (the last axis of d is then the site axis)."""
    _basis_operand("gbasis_expand: d", d, spec)
    _basis_operand("gbasis_expand: s", s, spec, d.shape)
    _basis_sites("gbasis_expand", d, spec)
    out = torch.empty(tuple(d.shape) + (spec.row,), dtype=d.dtype, device=d.device)
    if out.numel() == 0:
        return out
    with _timed("gbasis_expand"):
        check(lib().aggf_gbasis_expand(ptr(d), ptr(s), ptr(spec.centers), ptr(spec.slot), d.numel(), spec.n_basis,
                                       spec.n_sites, spec.n_slots, spec.width, spec.clip, int(q),
                                       dtype_code(d.dtype), ptr(out), stream_ptr()), "aggf_gbasis_expand")
    return out


def gbasis_contract(h: torch.Tensor, d: torch.Tensor, spec: BasisSpec, q: int = 0, form: int = GB_H_ELEM) -> torch.Tensor:
    """d.shape: out[e] = sum_k h[e][k] g_k^(q)(d[e]) (aggf_gbasis_contract); h is d.shape + (n_basis,) (GB_H_ELEM),
    d.shape + (n_slots * n_basis,) (GB_H_ROW) or (n_slots, n_basis) (GB_H_SLOT)."""
    _basis_operand("gbasis_contract: d", d, spec)
    if form == GB_H_ELEM:
        want = tuple(d.shape) + (spec.n_basis,)
    elif form == GB_H_ROW and spec.slot is not None:
        want = tuple(d.shape) + (spec.row,)
    elif form == GB_H_SLOT:
        want = (spec.n_slots, spec.n_basis)
    else:
        raise ValueError(f"gbasis_contract: form {form}")
    _basis_operand("gbasis_contract: h", h, spec, want)
    if form != GB_H_ELEM:
        _basis_sites("gbasis_contract", d, spec)
    out = torch.empty_like(d)
    if out.numel() == 0:
        return out
    slot = None if form == GB_H_ELEM else spec.slot
    n_sites = spec.n_sites if slot is not None else 1
    with _timed("gbasis_contract"):
        check(lib().aggf_gbasis_contract(ptr(h), form, ptr(d), ptr(spec.centers), ptr(slot), d.numel(), spec.n_basis,
                                         n_sites, spec.n_slots, spec.width, spec.clip, int(q), dtype_code(d.dtype),
                                         ptr(out), stream_ptr()), "aggf_gbasis_contract")
    return out


def gbasis_sum(d: torch.Tensor, spec: BasisSpec, q: int = 0, s: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n_slots, n_basis): out[slot, k] = sum over the frames and the slot's sites of s g_k^(q)(d) (aggf_gbasis_sum);
    d (..., n_sites) with slots, any shape without (one slot).  The one-hot array is never formed."""
    _basis_operand("gbasis_sum: d", d, spec)
    _basis_operand("gbasis_sum: s", s, spec, d.shape)
    _basis_sites("gbasis_sum", d, spec)
    out = torch.empty((spec.n_slots, spec.n_basis), dtype=d.dtype, device=d.device)
    if spec.slot is not None:
        N = spec.n_sites
        T = d.numel() // N
        order, start, n_order = spec.order, spec.start, spec.n_order
    else:  # one slot of all elements
        N = d.shape[-1] if d.dim() else 1
        T = d.numel() // N if N else 0
        order = start = None
        n_order = 0
    l = lib()
    need = l.aggf_gbasis_sum_workspace_bytes(T, spec.n_slots, spec.n_basis)
    ws = workspace(need, d.device, "gbasis") if need else None
    with _timed("gbasis_sum"):
        check(l.aggf_gbasis_sum(ptr(d), ptr(s), ptr(spec.centers), ptr(order), ptr(start), n_order, T, N, spec.n_slots,
                                spec.n_basis, spec.width, spec.clip, int(q), dtype_code(d.dtype), ptr(out), ptr(ws),
                                need, stream_ptr()), "aggf_gbasis_sum")
    return out
