// K9e: the minimum over frames of every pair distance (jaxutil.min_distances, from which PairList.from_cutoff builds a
// static list):  out[i,j] = min_t |X[t,j] - C[t,i]|,  X (T, n, 3), C (T, m, 3), out (m, n); under a box the displacement
// is its minimum image (min_image, aggf_common.h).  The element is pair_element<SQDIST> of K9a / K9c: the minimum is
// taken over the squared distances and one sqrt is applied at the end -- a correctly rounded sqrt is monotone, so the
// bits are those of the minimum of the distances (`square` skips the sqrt).
//
// The kernel reads coordinates only (3 (n + m) values per frame, cache-resident) and is VALU-bound.  A lane owns one j
// and PM_ROWS consecutive i: per frame it loads its X[t,j] once, the PM_ROWS rows of C are wave-uniform (scalar loads),
// and the PM_ROWS running minima stay in registers.  A workgroup is 4 waves = 256 consecutive j of one row block and one
// block of frames.  When the (m, n) tiles alone leave the chip short of workgroups the frames are split: partial minima
// (still squared) go to the workspace, split-major, and pairmin_reduce_kernel takes their minimum in split order.  No
// atomics; element offsets are 64-bit.  A NaN squared distance replaces the running minimum and stays (torch.amin's
// rule, not fmin's), so a NaN coordinate makes every pair of its site NaN.
#include "aggf_common.h"

namespace aggf {

constexpr int PM_ROWS = 8;
constexpr int PM_COLS = 256;
constexpr int64_t PM_TARGET_BLOCKS = 1024;  // 4 workgroups per CU
constexpr int64_t PM_MIN_FRAMES = 64;       // at most ceil(T / 64) splits: a full split holds more than 32 frames
constexpr int64_t PM_MAX_SPLITS = 256;

// min with torch.amin's NaN rule: a NaN candidate is taken, a NaN minimum is kept
template <typename T>
__device__ __forceinline__ T nan_min(T acc, T s) {
  return (s < acc || s != s) ? s : acc;
}

struct PairMinPlan {
  int64_t jblocks, iblocks, splits, frames;  // frames per split; no split is empty
};

// a function of the shape alone, shared by the workspace query and the call
static PairMinPlan pairmin_plan(int64_t T, int32_t m, int32_t n, int dtype) {
  (void)dtype;  // (one tile shape for both dtypes; the workspace is in the operands' dtype)
  PairMinPlan p;
  p.jblocks = ceil_div(n, PM_COLS);
  p.iblocks = ceil_div(m, PM_ROWS);
  int64_t s = ceil_div(PM_TARGET_BLOCKS, p.jblocks * p.iblocks);
  const int64_t s_cap = (T - 1) / PM_MIN_FRAMES + 1;  // (T >= 1; no T + m - 1: T may be any int64)
  if (s > s_cap) s = s_cap;
  if (s > PM_MAX_SPLITS) s = PM_MAX_SPLITS;
  if (s < 1) s = 1;
  p.frames = (T - 1) / s + 1;
  p.splits = (T - 1) / p.frames + 1;
  return p;
}

// dst: out when the plan has one split (root: the sqrt is applied here), else the (splits, m, n) partials
// (one body for the four forms: CELL_OPEN, CELL_BOX -- min_image --, CELL_TRI -- box is (T, 9), a triclinic cell per
// frame, brick_image -- and CELL_NEAR -- the same cell, nearest_image)
template <typename T, int CELL>
__device__ __forceinline__ void pairmin_body(const T* __restrict__ X, const T* __restrict__ C, int64_t nT, int32_t m,
                                             int32_t n, int64_t jblocks, int64_t iblocks, int64_t frames,
                                             const T* __restrict__ box, int32_t bstride, int root,
                                             T* __restrict__ dst) {
  const int64_t tiles = jblocks * iblocks;
  const int64_t split = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x - split * tiles;
  const int64_t ib = tile / jblocks, jb = tile - ib * jblocks;
  const int64_t j = jb * PM_COLS + threadIdx.x;
  const int64_t i0 = ib * PM_ROWS;
  const int64_t jc = j < n ? j : n - 1;  // (lanes and rows past the end recompute the last one and store nothing)
  const int64_t t0 = split * frames, t1 = t0 + frames < nT ? t0 + frames : nT;
  const int64_t xs = 3 * (int64_t)n, cs = 3 * (int64_t)m;
  int64_t coff[PM_ROWS];
#pragma unroll
  for (int r = 0; r < PM_ROWS; ++r) coff[r] = 3 * (i0 + r < m ? i0 + r : (int64_t)m - 1);
  T acc[PM_ROWS];
#pragma unroll
  for (int r = 0; r < PM_ROWS; ++r) acc[r] = (T)__builtin_inf();
  const T* x = X + t0 * xs + 3 * jc;
  const T* c = C + t0 * cs;
  T L[3] = {0, 0, 0}, iL[3] = {0, 0, 0};
  CellFrame<T> h = {};
  if (CELL == CELL_BOX && bstride == 0) box_lengths(box, L, iL);
  for (int64_t t = t0; t < t1; ++t, x += xs, c += cs) {
    const T x0 = x[0], x1 = x[1], x2 = x[2];
    if (CELL == CELL_BOX && bstride != 0) box_lengths(box + t * bstride, L, iL);
    if (CELL == CELL_TRI || CELL == CELL_NEAR) cell_frame(box + t * 9, h);
#pragma unroll
    for (int r = 0; r < PM_ROWS; ++r) {
      const T* cr = c + coff[r];
      T d0 = x0 - cr[0], d1 = x1 - cr[1], d2 = x2 - cr[2];
      if (CELL == CELL_BOX) d0 = min_image(d0, L[0], iL[0]), d1 = min_image(d1, L[1], iL[1]), d2 = min_image(d2, L[2], iL[2]);
      if (CELL == CELL_TRI || CELL == CELL_NEAR) cell_image<CELL>(d0, d1, d2, h);
      acc[r] = nan_min(acc[r], pair_element<T, AGGF_PAIR_SQDIST>(d0, d1, d2, (T)0, (T)0, (T)0));
    }
  }
  if (j >= n) return;
  T* o = dst + split * (int64_t)m * n + i0 * n + j;
#pragma unroll
  for (int r = 0; r < PM_ROWS; ++r)
    if (i0 + r < m) o[(int64_t)r * n] = root ? sqrt(acc[r]) : acc[r];
}

template <typename T, bool PBC>
__global__ __launch_bounds__(256) void pairmin_kernel(const T* __restrict__ X, const T* __restrict__ C, int64_t nT,
                                                      int32_t m, int32_t n, int64_t jblocks, int64_t iblocks,
                                                      int64_t frames, const T* __restrict__ box, int32_t bstride,
                                                      int root, T* __restrict__ dst) {
  pairmin_body<T, PBC ? CELL_BOX : CELL_OPEN>(X, C, nT, m, n, jblocks, iblocks, frames, box, bstride, root, dst);
}

// (the triclinic forms: an overload with a third template argument, CELL_TRI or CELL_NEAR)
template <typename T, bool PBC, int CELL>
__global__ __launch_bounds__(256) void pairmin_kernel(const T* __restrict__ X, const T* __restrict__ C, int64_t nT,
                                                      int32_t m, int32_t n, int64_t jblocks, int64_t iblocks,
                                                      int64_t frames, const T* __restrict__ cell, int root,
                                                      T* __restrict__ dst) {
  static_assert(PBC && (CELL == CELL_TRI || CELL == CELL_NEAR), "a triclinic form");
  pairmin_body<T, CELL>(X, C, nT, m, n, jblocks, iblocks, frames, cell, 9, root, dst);
}

template <typename T>
__global__ __launch_bounds__(256) void pairmin_reduce_kernel(const T* __restrict__ part, int64_t splits, int64_t count,
                                                             int root, T* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (int64_t)gridDim.x * 256) {
    T acc = part[e];
    for (int64_t s = 1; s < splits; ++s) acc = nan_min(acc, part[s * count + e]);
    out[e] = root ? sqrt(acc) : acc;
  }
}

// m n and splits m n as element counts that fit a 64-bit byte offset; 0: they do not
static int64_t pairmin_ws_elems(const PairMinPlan& p, int32_t m, int32_t n) {
  int64_t e = 0;
  if (__builtin_mul_overflow((int64_t)m * n, p.splits, &e) || e > INT64_MAX / 8) return 0;
  return e;
}

template <typename T>
static void launch_pairmin(const PairMinPlan& p, hipStream_t stream, const void* X, const void* C, int64_t nT,
                           int32_t m, int32_t n, const void* box, int32_t bstride, bool near, int square, void* out,
                           void* ws) {
  const dim3 grid((unsigned)(p.jblocks * p.iblocks * p.splits)), block(256);
  const bool split = p.splits > 1;
  const int root = !split && !square;
  T* dst = (T*)(split ? ws : out);
  if (box && bstride == 9 && near)
    AGGF_LAUNCH((pairmin_kernel<T, true, CELL_NEAR>), grid, block, 0, stream, (const T*)X, (const T*)C, nT, m, n, p.jblocks,
                p.iblocks, p.frames, (const T*)box, root, dst);
  else if (box && bstride == 9)
    AGGF_LAUNCH((pairmin_kernel<T, true, CELL_TRI>), grid, block, 0, stream, (const T*)X, (const T*)C, nT, m, n, p.jblocks,
                p.iblocks, p.frames, (const T*)box, root, dst);
  else if (box)
    AGGF_LAUNCH((pairmin_kernel<T, true>), grid, block, 0, stream, (const T*)X, (const T*)C, nT, m, n, p.jblocks,
                p.iblocks, p.frames, (const T*)box, bstride, root, dst);
  else
    AGGF_LAUNCH((pairmin_kernel<T, false>), grid, block, 0, stream, (const T*)X, (const T*)C, nT, m, n, p.jblocks,
                p.iblocks, p.frames, (const T*)nullptr, 0, root, dst);
  if (split) {
    const int64_t count = (int64_t)m * n;
    int64_t blocks = ceil_div(count, 256);
    if (blocks > 65536) blocks = 65536;
    AGGF_LAUNCH((pairmin_reduce_kernel<T>), dim3((unsigned)blocks), block, 0, stream, (const T*)ws, p.splits, count,
                !square, (T*)out);
  }
}

}  // namespace aggf

using namespace aggf;

extern "C" size_t aggf_pair_min_workspace_bytes(int64_t T, int32_t m, int32_t n, int dtype) {
  if (T <= 0 || m <= 0 || n <= 0) return 0;
  const PairMinPlan p = pairmin_plan(T, m, n, dtype);
  if (p.splits <= 1) return 0;
  return (size_t)pairmin_ws_elems(p, m, n) * (dtype == AGGF_F64 ? 8 : 4);
}

static int pair_min(const char* who, const void* X, const void* C, int64_t T, int32_t m, int32_t n, int dtype,
                    const void* box, int32_t box_stride, bool near, int square, void* out, void* ws, size_t ws_bytes,
                    void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (T < 0 || m < 0 || n < 0) return fail(AGGF_ERR_ARG, "%s: negative shape", who);
  if (dtype != AGGF_F32 && dtype != AGGF_F64) return fail(AGGF_ERR_ARG, "%s: bad dtype", who);
  if (box_stride != 0 && box_stride != 3 && box_stride != 9)
    return fail(AGGF_ERR_ARG, "%s: box_stride %d is none of 0, 3 and 9", who, box_stride);
  if (box_stride == 9 && !box) return fail(AGGF_ERR_ARG, "%s: box_stride 9 without a cell", who);
  if (T == 0 || m == 0 || n == 0) return AGGF_OK;
  int64_t sites = 0;
  if (__builtin_mul_overflow(T, 3 * (int64_t)(m > n ? m : n), &sites) || sites > INT64_MAX / 8)
    return fail(AGGF_ERR_ARG, "%s: T n does not fit a 64-bit byte offset", who);
  if (!X || !C || !out) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  const PairMinPlan p = pairmin_plan(T, m, n, dtype);
  const int64_t elems = pairmin_ws_elems(p, m, n);
  if (elems == 0) return fail(AGGF_ERR_ARG, "%s: m n does not fit a 64-bit byte offset", who);
  if (p.jblocks * p.iblocks * p.splits > 0x7fffffff) return fail(AGGF_ERR_ARG, "%s: too many output tiles", who);
  if (p.splits > 1) {
    const size_t esz = dtype == AGGF_F64 ? 8 : 4;
    if (!ws || ws_bytes < (size_t)elems * esz) return fail(AGGF_ERR_WORKSPACE, "%s: workspace too small", who);
    if ((uintptr_t)ws % esz) return fail(AGGF_ERR_WORKSPACE, "%s: workspace is not element-aligned", who);
  }
  if (dtype == AGGF_F64)
    launch_pairmin<double>(p, stream, X, C, T, m, n, box, box_stride, near, square, out, ws);
  else
    launch_pairmin<float>(p, stream, X, C, T, m, n, box, box_stride, near, square, out, ws);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

extern "C" int aggf_pair_min(const void* X, const void* C, int64_t T, int32_t m, int32_t n, int dtype, const void* box,
                             int32_t box_stride, int square, void* out, void* ws, size_t ws_bytes, void* stream_v) {
  return pair_min("aggf_pair_min", X, C, T, m, n, dtype, box, box_stride, false, square, out, ws, ws_bytes, stream_v);
}

extern "C" int aggf_pair_min_cell(const void* X, const void* C, int64_t T, int32_t m, int32_t n, int dtype,
                                  const void* cell, int square, void* out, void* ws, size_t ws_bytes, void* stream_v,
                                  int images) {
  if (!cell) return fail(AGGF_ERR_ARG, "aggf_pair_min_cell: NULL cell");
  if (images != AGGF_IMAGES_BRICK && images != AGGF_IMAGES_NEAREST)
    return fail(AGGF_ERR_ARG, "aggf_pair_min_cell: images %d is neither AGGF_IMAGES_BRICK nor AGGF_IMAGES_NEAREST", images);
  return pair_min("aggf_pair_min_cell", X, C, T, m, n, dtype, cell, 9, images == AGGF_IMAGES_NEAREST, square, out, ws,
                  ws_bytes, stream_v);
}
