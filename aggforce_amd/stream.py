"""Out-of-core front end: host-resident (memory-mapped) trajectories through the hot path.

SURVEY 8(f) rank 4.  The reference consumes ``.npz`` files with keys ``coords`` and ``Fs``
(tests/test_forces.py:92-94, examples/gauss.py:61-68) and holds everything in host memory.  Here
a trajectory that does not fit in HBM (or that should not be uploaded whole) is streamed in frame
chunks: pinned staging buffers, host-to-device copies on a separate HIP stream overlapped with
the kernels, K1 accumulating into one Gram, then K2 once and K3 chunk by chunk.  The result equals
``project_forces`` on the same arrays (same kernels, chunked summation order).
"""
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, Iterator, Optional, Tuple, Union

import numpy as np

from . import _kernels as K
from .agg import (
    CONSTRAINTS_KNAME,
    PROJCOORDS_KNAME,
    PROJFORCES_KNAME,
    RESIDUAL_KNAME,
    TMAP_KNAME,
)
from .constraints import Constraints
from .distributed import all_reduce_sum_, all_reduce_sum_sym_
from .map import LinearMap
from .qp.qplinear import LinearProblem


def load_trajectory(path: str, coords_key: str = "coords", forces_key: str = "Fs") -> Tuple[np.ndarray, np.ndarray]:
    """(coords, forces) from the reference's ``.npz`` layout, or from a pair of ``.npy`` files.

    ``path`` ending in ``.npz``: arrays under ``coords_key`` / ``forces_key`` (read into host
    memory; NumPy cannot map members of an archive).  Otherwise ``path`` is a prefix:
    ``<path>_coords.npy`` and ``<path>_forces.npy`` are memory-mapped read-only, so frames are
    paged in only as the streamed pass touches them.
    """
    if path.endswith(".npz"):
        with np.load(path) as z:
            for key in (coords_key, forces_key):
                if key not in z.files:
                    raise KeyError(f"{path} has no array {key!r} (found {z.files})")
            return z[coords_key], z[forces_key]
    return (np.load(path + "_coords.npy", mmap_mode="r"), np.load(path + "_forces.npy", mmap_mode="r"))


def default_chunk_frames(n_sites: int, itemsize: int, budget_bytes: int = 8 << 30) -> int:
    """Frames per chunk so that the four device buffers (2 arrays x double buffer) fit the budget."""
    return max(1, int(budget_bytes // (4 * n_sites * 3 * itemsize)))


def _stage_threads() -> int:
    """Threads that copy a chunk out of the page cache into the pinned staging buffer: AGGF_STAGE_THREADS, else the
    CPUs this process may run on minus two (one for the Python thread, one for the driver), at most 16 -- a single
    thread moves ~6 GB/s, the PCIe link takes ~55."""
    env = os.environ.get("AGGF_STAGE_THREADS")
    if env:
        return max(1, int(env))
    try:
        avail = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        avail = os.cpu_count() or 2
    return max(1, min(16, avail - 2))


_STAGE_THREADS = _stage_threads()
_stage_pool: Optional[ThreadPoolExecutor] = None


def _parallel_copy(dst: np.ndarray, src: np.ndarray) -> None:
    """dst[:] = src with the frame axis split over a few threads (NumPy copies release the GIL);
    a single thread moves ~6 GB/s out of the page cache, far below the PCIe link."""
    global _stage_pool
    n = dst.shape[0]
    if _STAGE_THREADS == 1 or dst.nbytes < (32 << 20):
        np.copyto(dst, src, casting="same_kind")
        return
    if _stage_pool is None:
        _stage_pool = ThreadPoolExecutor(max_workers=_STAGE_THREADS, thread_name_prefix="aggf-stage")
    step = -(-n // _STAGE_THREADS)
    futs = [_stage_pool.submit(np.copyto, dst[b:b + step], src[b:b + step], "same_kind") for b in range(0, n, step)]
    for f in futs:
        f.result()


class _ChunkUploader:
    """Double-buffered host->device pipeline over one host array (frames on axis 0)."""

    def __init__(self, src: np.ndarray, chunk: int, device) -> None:
        import torch

        self.src = src
        self.chunk = chunk
        dt = torch.float64 if src.dtype == np.float64 else torch.float32
        self.np_dtype = np.float64 if src.dtype == np.float64 else np.float32
        shape = (chunk,) + tuple(src.shape[1:])
        self.host = [torch.empty(shape, dtype=dt, pin_memory=True) for _ in range(2)]
        self.dev = [torch.empty(shape, dtype=dt, device=device) for _ in range(2)]
        self.ready = [torch.cuda.Event() for _ in range(2)]
        self.free = [torch.cuda.Event() for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(device=device)
        # the device buffers come from the allocator's pool of the caller's current stream: a block it hands out again may
        # still be read by work queued there, so the uploads start behind everything already on that stream
        self.copy_stream.wait_stream(torch.cuda.current_stream(device))
        self._n = 0

    def stage(self, begin: int, end: int):
        """Start the upload of frames [begin, end); returns a handle for ``wait``."""
        import torch

        s = self._n & 1
        self._n += 1
        n = end - begin
        self.free[s].synchronize()  # kernels reading dev[s] (and thus the copy out of host[s]) are done
        _parallel_copy(self.host[s][:n].numpy(), self.src[begin:end])
        with torch.cuda.stream(self.copy_stream):
            self.dev[s][:n].copy_(self.host[s][:n], non_blocking=True)
            self.ready[s].record(self.copy_stream)
        return s, n

    def wait(self, handle):
        """Device view of a staged chunk, ordered after its upload on the current stream."""
        import torch

        s, n = handle
        torch.cuda.current_stream().wait_event(self.ready[s])
        return self.dev[s][:n]

    def release(self, handle) -> None:
        """Mark the chunk's device buffer reusable once the work queued so far has run."""
        import torch

        self.free[handle[0]].record(torch.cuda.current_stream())


def _chunks(n_frames: int, chunk: int) -> Iterator[Tuple[int, int]]:
    for b in range(0, n_frames, chunk):
        yield b, min(n_frames, b + chunk)


def project_forces_streamed(
    coords: np.ndarray,
    forces: np.ndarray,
    coord_map: LinearMap,
    constrained_inds: Union[Constraints, None] = None,
    l2_regularization: float = 0.0,
    chunk_frames: Optional[int] = None,
    gram_dtype=None,
    comm=None,
) -> Dict[str, Any]:
    """``project_forces`` with the linear optimiser for host arrays streamed in frame chunks.

    coords, forces: (n_frames, n_sites, 3) NumPy arrays or memory maps on the host (this rank's
    frames when ``comm`` is given).  ``constrained_inds`` must be explicit (a set of frozensets or
    None): guessing constraints needs the whole trajectory (use ``guess_pairwise_constraints`` on
    a subset beforehand).  Two passes over the data: (1) K1 accumulates the Gram chunk by chunk
    while the next chunk uploads, (2) after the K2 solve the map is applied chunk by chunk (K3)
    and the mapped arrays are collected on the host.  Returns the dict of ``project_forces``.
    """
    import torch

    if isinstance(constrained_inds, str):
        raise ValueError("project_forces_streamed needs explicit constraints (a set of frozensets or None).")
    if coords.shape != forces.shape or forces.ndim != 3 or forces.shape[2] != 3:
        raise ValueError("coords and forces must both have shape (n_frames, n_sites, 3)")
    T, N, _ = forces.shape
    if T == 0:
        raise ValueError("empty trajectory")
    dev = K.default_device()
    item = 8 if forces.dtype == np.float64 else 4
    chunk = int(chunk_frames) if chunk_frames else default_chunk_frames(N, item)
    chunk = max(1, min(chunk, T))
    prob = LinearProblem(coord_map, constrained_inds, dev)

    # pass 1: Gram
    up_f = _ChunkUploader(forces, chunk, dev)
    G = torch.zeros((prob.n_red, prob.n_red), dtype=torch.float64, device=dev)
    spans = list(_chunks(T, chunk))
    pending = up_f.stage(*spans[0])
    nan_seen = False
    for i in range(len(spans)):
        cur = pending
        f = up_f.wait(cur)
        nan_seen = nan_seen or K.has_nan(f)
        prob.gram(f, gram_dtype, out=G, accumulate=True)
        up_f.release(cur)
        if i + 1 < len(spans):
            pending = up_f.stage(*spans[i + 1])
    if nan_seen:
        raise ValueError("NaN forces: the streamed path does not fit maps on trajectories with NaNs.")
    all_reduce_sum_sym_(G, comm)
    tmap = prob.tmap(prob.solve(G, l2_regularization))
    del G

    # pass 2: apply
    up_c = _ChunkUploader(coords, chunk, dev)
    n_cg = coord_map.standard_matrix.shape[0]
    mapped_c = mapped_f = None
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    pend = (up_c.stage(*spans[0]), up_f.stage(*spans[0]))
    for i, (b, e) in enumerate(spans):
        hc, hf = pend
        mc, mf = tmap.map_arrays(up_c.wait(hc), up_f.wait(hf))
        K.axpby(1.0, acc, 1.0, K.sumsq(mf), out=acc)
        up_c.release(hc)
        up_f.release(hf)
        if i + 1 < len(spans):  # next uploads overlap the kernels queued above
            pend = (up_c.stage(*spans[i + 1]), up_f.stage(*spans[i + 1]))
        # download on its own stream into PINNED host arrays: the copy of chunk i overlaps the kernels of
        # chunk i+1 (a pageable `.cpu()` per chunk blocked the host for every chunk: 21.9 GB/s of a 63 GB/s link)
        if mapped_c is None:
            mapped_c = torch.empty((T, n_cg, 3), dtype=mc.dtype, pin_memory=True)
            mapped_f = torch.empty((T, n_cg, 3), dtype=mf.dtype, pin_memory=True)
            down = torch.cuda.Stream(device=dev)
        down.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(down):
            mapped_c[b:e].copy_(mc, non_blocking=True)
            mapped_f[b:e].copy_(mf, non_blocking=True)
        mc.record_stream(down)
        mf.record_stream(down)
    down.synchronize()
    mapped_c, mapped_f = mapped_c.numpy(), mapped_f.numpy()
    cnt = torch.tensor([float(T) * n_cg * 3], dtype=torch.float64, device=dev)
    both = torch.cat([acc, cnt])
    all_reduce_sum_(both, comm)
    s, n = both.tolist()
    return {
        PROJCOORDS_KNAME: mapped_c,
        PROJFORCES_KNAME: mapped_f,
        TMAP_KNAME: tmap,
        RESIDUAL_KNAME: float(s / n),
        CONSTRAINTS_KNAME: constrained_inds,
    }
