// K7: map validation with random Gaussian pair-potential force fields (reference jaxmapval.py).
//
// One Gaussian of the SQUARED pair distance, g(x) = exp(-((x - o) / w)^2), x = |r_i - r_j|^2, summed over the full
// n x n matrix of a frame (sq_gaussian_energies, jaxmapval.py:365-392), has the forces (the diagonal drops out)
//     G_i = (8 / w^2) sum_j (x_ij - o) g(x_ij) (r_i - r_j).
// The reference materialises G (T, n, 3) once per random offset o_s and reduces it against the mapped forces.  Here:
//   * gauss_site_forces_kernel: G and the frame energies for ONE offset (sq_gaussian_forces / _energies);
//   * gauss_proj_kernel:  P_s = sum_t sum_i F_i . G_s,i for S offsets in one pass, in the pair form
//         sum_{i<j} (x - o_s) g_s(x) u,   u = (r_i - r_j) . (F_i - F_j)   (times 8 / w^2):
//     a workgroup takes a range of (frame, pair) entries, forms (x, u) once per entry into LDS, and every thread runs
//     its MV_SC offsets (registers) over the staged list -- all lanes read the same LDS word (broadcast);
//   * gauss_shift_kernel: sum F . G_s and sum |G_s|^2 for S offsets in one pass, in the per-site form (|G_s|^2 needs
//     the per-site sums): a workgroup walks its frames and sites i, accumulates G_s,i over j from the frame's
//     coordinates in LDS (tiled over j above MV_JT sites), and folds F_i . G_s,i and |G_s,i|^2 into per-sample sums.
//     Each thread owns a chunk of samples, so those sums need no cross-lane reduction;
//   * dot_kernel: sum a * b in a fixed order (mscg_ip and the generic loop of random_force_proj / _residual_shift).
// Precision: float64 when either input is float64, float32 with the hardware exp2 when both are float32; every sum
// over pairs, sites and frames is float64.  Partial sums go to slabs (one per workgroup) and are combined in a fixed
// order: two runs are bit-identical.  x is formed from the differences r_i - r_j.
// Periodic forms (template argument PBC of the three gauss kernels; the open forms keep their arithmetic and bits): every
// displacement d = r_i - r_j is replaced by its image under the frame's cell before x = |d|^2 is formed, so
// E_t = sum_{i,j} g(|d_ij|^2) (the diagonal is d = 0) and G_i = (8 / w^2) sum_j (x_ij - o) g(x_ij) d_ij.  The image is
// exactly odd, so the pair form of the projection stands: u = d . (F_i - F_j).  There is ONE periodic form: it holds a
// CellFrame per frame and takes the brick image (aggf_common.h); the lengths of an orthorhombic box are loaded as a
// cell without off-diagonal entries, which is min_image bit for bit (fma(-k, 0, d) == d).  A frame whose box or cell
// is bad (box_lengths, cell_good) has NaN images: its G and E are NaN, and so is every sample of a fused reduction.
// The nearest-image forms (a further template argument CELL_NEAR on overloads of the three kernels; aggf_*_cell with
// AGGF_IMAGES_NEAREST) take the same (T, 9) cells and replace brick_image by nearest_image.  The kernels' text is in
// aggf_mapval_kernels.inc, included twice, so that the open and periodic kernels are compiled from the tokens they have
// always had: their names, instructions and bits are unchanged.  The products of the sums (u = d . (F_i - F_j), c d) are
// fused as the compiler chooses per instantiation, so the nearest form's sums agree with the brick form's only to
// rounding even where the two images are the same numbers (K9's agree bit for bit).
#include "aggf_common.h"

namespace aggf {

constexpr int MV_THREADS = 256;
constexpr int MV_SC = 4;                         // offsets per thread (registers)
constexpr int MV_SCHUNK = MV_THREADS * MV_SC;    // offsets per workgroup (grid y)
constexpr int MV_JT = 1024;                      // sites per LDS stage of the per-site kernels (24 KiB in float64)
constexpr int MV_PL = 1024;                      // (x, u) entries per LDS stage of the projection kernel
constexpr int64_t MV_TARGET_WGS = 2048;          // workgroups a split plan aims for (8 per CU)
constexpr int64_t MV_SLAB_MAX = (int64_t)1 << 26;  // slab doubles at most (512 MiB)
constexpr int MV_DOT_BLOCKS = 1024;
constexpr int64_t MV_MAX_GRID = 65536;

template <typename A, typename B>
struct Promote {
  typedef double type;
};
template <>
struct Promote<float, float> {
  typedef float type;
};

// g = exp(-(tt^2) / w^2) with k = coef(w): float32 uses v_exp_f32 (exp2, log2(e) folded into k), float64 the libm exp
template <typename C>
struct Gauss;
template <>
struct Gauss<float> {
  __host__ __device__ static float coef(double width) { return (float)(1.4426950408889634074 / (width * width)); }
  __device__ static __forceinline__ float g(float tt, float k) { return __builtin_amdgcn_exp2f(-(tt * tt) * k); }
};
template <>
struct Gauss<double> {
  __host__ __device__ static double coef(double width) { return 1.0 / (width * width); }
  __device__ static __forceinline__ double g(double tt, double k) { return exp(-(tt * tt) * k); }
};

// x = |d|^2 summed left to right with no fused multiply-add: x - o cancels near the offset, and this is the
// rounding of the float64 restatement the tests compare with
template <typename C>
__device__ __forceinline__ C sq_norm3(C d0, C d1, C d2) {
#pragma clang fp contract(off)
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// The cell of frame t in the compute type C.  `box` is in X's dtype: (T, 9) row-major cells (bstride 9), or the lengths
// of an orthorhombic box, (T, 3) (bstride 3) or (3,) (bstride 0), as a cell with zero off-diagonal entries.
template <typename C, typename TX>
__device__ __forceinline__ void mv_cell(const TX* __restrict__ box, int32_t bstride, int64_t t, CellFrame<C>& h) {
  const bool tri = bstride == 9;
  const TX* m = box + t * bstride;
  const TX zero = (TX)0, inf = (TX)__builtin_inf();
  const TX ax = m[0], by = m[tri ? 4 : 1], cz = m[tri ? 8 : 2];
  const TX bx = tri ? m[3] : zero, cx = tri ? m[6] : zero, cy = tri ? m[7] : zero;
  // cell_good's rule, which for a box is box_lengths': positive finite lengths (the whole frame is NaN otherwise)
  const bool ok = ax > zero && ax < inf && by > zero && by < inf && cz > zero && cz < inf && __builtin_fabs(bx) < inf &&
                  __builtin_fabs(cx) < inf && __builtin_fabs(cy) < inf;
  const C nan = (C)__builtin_nan("");
  h.ax = ok ? (C)ax : nan, h.bx = ok ? (C)bx : nan, h.by = ok ? (C)by : nan;
  h.cx = ok ? (C)cx : nan, h.cy = ok ? (C)cy : nan, h.cz = ok ? (C)cz : nan;
  h.iax = (C)1 / h.ax, h.iby = (C)1 / h.by, h.icz = (C)1 / h.cz;
}

// pair index p in [0, n (n - 1) / 2) -> (i, j), i < j, row by row of the strict upper triangle
__device__ __forceinline__ int64_t pair_row_start(int64_t i, int64_t n) { return i * (n - 1) - i * (i - 1) / 2; }
__device__ __forceinline__ void pair_of(int64_t p, int64_t n, int64_t* pi, int64_t* pj) {
  const double b = (double)(2 * n - 1);
  int64_t i = (int64_t)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
  if (i < 0) i = 0;
  if (i > n - 2) i = n - 2;
  while (i > 0 && pair_row_start(i, n) > p) --i;
  while (i < n - 2 && pair_row_start(i + 1, n) <= p) ++i;
  *pi = i;
  *pj = i + 1 + (p - pair_row_start(i, n));
}

#define AGGF_MV_FORM_PARAM
#define AGGF_MV_IMAGE brick_image
#include "aggf_mapval_kernels.inc"
#undef AGGF_MV_FORM_PARAM
#undef AGGF_MV_IMAGE
// (the nearest-image forms: overloads with a further template argument, CELL_NEAR the only value instantiated)
#define AGGF_MV_FORM_PARAM , int CELL
#define AGGF_MV_IMAGE nearest_image
#include "aggf_mapval_kernels.inc"
#undef AGGF_MV_FORM_PARAM
#undef AGGF_MV_IMAGE

// E[t] = sum_ib eslab[t][ib], in order
template <typename TX>
__global__ __launch_bounds__(256) void gauss_energy_finish_kernel(const double* __restrict__ eslab, int64_t T,
                                                                  int32_t n_iblk, TX* __restrict__ E) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < T; t += (int64_t)gridDim.x * 256) {
    double s = 0.0;
    for (int ib = 0; ib < n_iblk; ++ib) s += eslab[t * n_iblk + ib];
    E[t] = (TX)s;
  }
}

// out_w[s] = scale_w * sum_k slabs[k][s][w] (w < W), k ascending
__global__ __launch_bounds__(256) void mapval_slab_reduce_kernel(const double* __restrict__ slabs, int64_t K, int64_t S,
                                                                 int W, double scale0, double scale1,
                                                                 double* __restrict__ out0, double* __restrict__ out1) {
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < S; s += (int64_t)gridDim.x * 256) {
    double a = 0.0, b = 0.0;
    for (int64_t k = 0; k < K; ++k) {
      a += slabs[(k * S + s) * W];
      if (W == 2) b += slabs[(k * S + s) * W + 1];
    }
    out0[s] = scale0 * a;
    if (W == 2) out1[s] = scale1 * b;
  }
}

// ---- fixed-order dot product: workgroup w takes elements w*256 + tid + m * (MV_DOT_BLOCKS * 256), four accumulators
template <typename TA, typename TB>
__global__ __launch_bounds__(256) void dot_kernel(const TA* __restrict__ a, const TB* __restrict__ b, int64_t n,
                                                  double* __restrict__ partials) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (; i + 3 * stride < n; i += 4 * stride) {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += (double)a[i + u * stride] * (double)b[i + u * stride];
  }
  for (; i < n; i += stride) acc[0] += (double)a[i] * (double)b[i];
  double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ double w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
}

__global__ __launch_bounds__(256) void dot_finish_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ double w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (w[0] + w[1]) + (w[2] + w[3]);
}

// ---- host: shapes and launch plans
static bool mv_dtype_ok(int d) { return d == AGGF_F32 || d == AGGF_F64; }

// T * n * n fits in int64 with room (every index of the kernels is below it)
static bool mv_shape_ok(int64_t T, int32_t n) {
  if (T <= 0 || n <= 0) return false;
  return T <= ((int64_t)1 << 60) / ((int64_t)n * n);
}

struct SitePlan {
  int32_t fpb, iblk, n_iblk;
  int64_t n_blocks;
};
static SitePlan site_plan(int64_t T, int32_t n) {
  SitePlan p;
  p.fpb = n <= MV_THREADS ? MV_THREADS / n : 1;
  p.iblk = n <= MV_THREADS ? n : MV_THREADS;
  p.n_iblk = (int32_t)ceil_div(n, p.iblk);
  p.n_blocks = ceil_div(T, p.fpb) * p.n_iblk;
  return p;
}

struct SplitPlan {
  int64_t K, per_split, n_sch;
};
// split `units` (pair entries or frames) into K ranges; at least `min_units` per range
static SplitPlan split_plan(int64_t units, int64_t min_units, int64_t S, int W) {
  SplitPlan p;
  p.n_sch = ceil_div(S, MV_SCHUNK);
  int64_t k = ceil_div(MV_TARGET_WGS, p.n_sch);
  const int64_t k_units = ceil_div(units, min_units);
  if (k > k_units) k = k_units;
  const int64_t k_mem = MV_SLAB_MAX / (S * W);
  if (k > k_mem) k = k_mem;
  if (k < 1) k = 1;
  p.per_split = units > 0 ? ceil_div(units, k) : 1;
  p.K = units > 0 ? ceil_div(units, p.per_split) : 1;
  return p;
}

// box NULL: the open kernels; else (T, 9) cells, (T, 3) or (3,) lengths by its stride
static int mv_box(const char* who, const void* box, int32_t box_stride) {
  if (box && box_stride != 0 && box_stride != 3 && box_stride != 9)
    return fail(AGGF_ERR_ARG, "%s: box_stride %d is none of 0, 3 and 9", who, box_stride);
  return AGGF_OK;
}

// the cell of a `_cell` entry and its image selector: AGGF_IMAGES_BRICK (the form of box_stride 9) or AGGF_IMAGES_NEAREST
static int mv_cell_arg(const char* who, const void* cell, int images) {
  if (!cell) return fail(AGGF_ERR_ARG, "%s: NULL cell", who);
  if (images != AGGF_IMAGES_BRICK && images != AGGF_IMAGES_NEAREST)
    return fail(AGGF_ERR_ARG, "%s: images %d is neither AGGF_IMAGES_BRICK nor AGGF_IMAGES_NEAREST", who, images);
  return AGGF_OK;
}

static bool mv_samples_ok(int64_t S) { return S > 0 && ceil_div(S, MV_SCHUNK) <= 65535; }

static size_t proj_ws(int64_t T, int32_t n, int64_t S) {
  const SplitPlan p = split_plan(T * ((int64_t)n * (n - 1) / 2), MV_PL, S, 1);
  return (size_t)(p.K * S) * sizeof(double) + 256;
}
static size_t shift_ws(int64_t T, int64_t S) {
  const SplitPlan p = split_plan(T, 1, S, 2);
  return (size_t)(p.K * S * 2) * sizeof(double) + 256;
}

}  // namespace aggf

using namespace aggf;

extern "C" size_t aggf_gauss_pair_forces_workspace_bytes(int64_t T, int32_t n) {
  if (!mv_shape_ok(T, n)) return 0;
  const SitePlan p = site_plan(T, n);
  return (size_t)(T * p.n_iblk) * sizeof(double) + 256;
}

template <typename TX>
static void launch_site(dim3 grid, hipStream_t stream, const void* X, int64_t T, int32_t n, const SitePlan& p,
                        double offset, double width, void* G, double* eslab, const void* box, int32_t bstride,
                        bool near) {
  const TX k = Gauss<TX>::coef(width);
  const double scale = 8.0 / (width * width);
  if (box && near)
    AGGF_LAUNCH((gauss_site_forces_kernel<TX, true, CELL_NEAR>), grid, dim3(MV_THREADS), 0, stream, (const TX*)X, T, n,
                p.fpb, p.iblk, p.n_iblk, p.n_blocks, (TX)offset, k, scale, (TX*)G, eslab, (const TX*)box, bstride);
  else if (box)
    AGGF_LAUNCH((gauss_site_forces_kernel<TX, true>), grid, dim3(MV_THREADS), 0, stream, (const TX*)X, T, n, p.fpb,
                p.iblk, p.n_iblk, p.n_blocks, (TX)offset, k, scale, (TX*)G, eslab, (const TX*)box, bstride);
  else
    AGGF_LAUNCH((gauss_site_forces_kernel<TX, false>), grid, dim3(MV_THREADS), 0, stream, (const TX*)X, T, n, p.fpb,
                p.iblk, p.n_iblk, p.n_blocks, (TX)offset, k, scale, (TX*)G, eslab, (const TX*)nullptr, 0);
}

static int gauss_pair_forces(const char* who, const void* X, int64_t T, int32_t n, int dtype, double offset,
                            double width, const void* box, int32_t box_stride, bool near, void* G, void* E, void* ws,
                            size_t ws_bytes, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!X || (!G && !E)) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (!mv_dtype_ok(dtype)) return fail(AGGF_ERR_ARG, "%s: bad dtype", who);
  if (!mv_shape_ok(T, n)) return fail(AGGF_ERR_ARG, "%s: bad shape (T=%lld, n=%d)", who, (long long)T, n);
  if (!(width > 0.0)) return fail(AGGF_ERR_ARG, "%s: width must be positive", who);
  const int rcb = mv_box(who, box, box_stride);
  if (rcb != AGGF_OK) return rcb;
  const SitePlan p = site_plan(T, n);
  double* eslab = nullptr;
  if (E) {
    if (!ws) return fail(AGGF_ERR_ARG, "%s: NULL workspace", who);
    if (ws_bytes < (size_t)(T * p.n_iblk) * sizeof(double))
      return fail(AGGF_ERR_WORKSPACE, "%s: workspace too small", who);
    eslab = (double*)ws;
  }
  const dim3 grid((unsigned)(p.n_blocks < MV_MAX_GRID ? p.n_blocks : MV_MAX_GRID));
  const int64_t fg = ceil_div(T, 256) < 4096 ? ceil_div(T, 256) : 4096;
  if (dtype == AGGF_F64) {
    launch_site<double>(grid, stream, X, T, n, p, offset, width, G, eslab, box, box_stride, near);
    AGGF_LAUNCH_OK();
    if (E) AGGF_LAUNCH(gauss_energy_finish_kernel<double>, dim3((unsigned)fg), dim3(256), 0, stream, eslab, T, p.n_iblk,
                       (double*)E);
  } else {
    launch_site<float>(grid, stream, X, T, n, p, offset, width, G, eslab, box, box_stride, near);
    AGGF_LAUNCH_OK();
    if (E) AGGF_LAUNCH(gauss_energy_finish_kernel<float>, dim3((unsigned)fg), dim3(256), 0, stream, eslab, T, p.n_iblk,
                       (float*)E);
  }
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

extern "C" int aggf_gauss_pair_forces(const void* X, int64_t T, int32_t n, int dtype, double offset, double width,
                                      const void* box, int32_t box_stride, void* G, void* E, void* ws, size_t ws_bytes,
                                      void* stream_v) {
  return gauss_pair_forces("aggf_gauss_pair_forces", X, T, n, dtype, offset, width, box, box_stride, false, G, E, ws,
                           ws_bytes, stream_v);
}

extern "C" int aggf_gauss_pair_forces_cell(const void* X, int64_t T, int32_t n, int dtype, double offset, double width,
                                           const void* cell, void* G, void* E, void* ws, size_t ws_bytes,
                                           void* stream_v, int images) {
  const int rc = mv_cell_arg("aggf_gauss_pair_forces_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return gauss_pair_forces("aggf_gauss_pair_forces_cell", X, T, n, dtype, offset, width, cell, 9,
                           images == AGGF_IMAGES_NEAREST, G, E, ws, ws_bytes, stream_v);
}

extern "C" size_t aggf_gauss_proj_workspace_bytes(int64_t T, int32_t n, int64_t S) {
  if (!mv_shape_ok(T, n) || !mv_samples_ok(S)) return 0;
  return proj_ws(T, n, S);
}

extern "C" size_t aggf_gauss_shift_workspace_bytes(int64_t T, int32_t n, int64_t S) {
  if (!mv_shape_ok(T, n) || !mv_samples_ok(S)) return 0;
  return shift_ws(T, S);
}

// (box NULL: the open instantiation; near: the nearest-image one)
#define AGGF_MV_LAUNCH(KERNEL, TF, PBC, BOX, STRIDE)                                                               \
  AGGF_LAUNCH((KERNEL<TX, TF, PBC>), grid, dim3(MV_THREADS), 0, stream, X, (const TF*)F, T, n, offsets, S, width,  \
              p.per_split, slabs, BOX, STRIDE)
#define AGGF_MV_LAUNCH_NEAR(KERNEL, TF)                                                                            \
  AGGF_LAUNCH((KERNEL<TX, TF, true, CELL_NEAR>), grid, dim3(MV_THREADS), 0, stream, X, (const TF*)F, T, n, offsets, \
              S, width, p.per_split, slabs, (const TX*)box, bstride)
#define AGGF_MV_LAUNCH_X(NAME, KERNEL)                                                                             \
  template <typename TX>                                                                                           \
  static void NAME(const TX* X, const void* F, int f_dtype, int64_t T, int32_t n, const double* offsets, int64_t S, \
                   double width, const SplitPlan& p, double* slabs, const void* box, int32_t bstride, bool near,   \
                   hipStream_t stream) {                                                                           \
    const dim3 grid((unsigned)p.K, (unsigned)p.n_sch);                                                             \
    if (box && near && f_dtype == AGGF_F64)                                                                        \
      AGGF_MV_LAUNCH_NEAR(KERNEL, double);                                                                         \
    else if (box && near)                                                                                          \
      AGGF_MV_LAUNCH_NEAR(KERNEL, float);                                                                          \
    else if (box && f_dtype == AGGF_F64)                                                                           \
      AGGF_MV_LAUNCH(KERNEL, double, true, (const TX*)box, bstride);                                               \
    else if (box)                                                                                                  \
      AGGF_MV_LAUNCH(KERNEL, float, true, (const TX*)box, bstride);                                                \
    else if (f_dtype == AGGF_F64)                                                                                  \
      AGGF_MV_LAUNCH(KERNEL, double, false, (const TX*)nullptr, 0);                                                \
    else                                                                                                           \
      AGGF_MV_LAUNCH(KERNEL, float, false, (const TX*)nullptr, 0);                                                 \
  }
AGGF_MV_LAUNCH_X(launch_proj_x, gauss_proj_kernel)
AGGF_MV_LAUNCH_X(launch_shift_x, gauss_shift_kernel)
#undef AGGF_MV_LAUNCH_X
#undef AGGF_MV_LAUNCH_NEAR
#undef AGGF_MV_LAUNCH

static int mv_check(const char* who, const void* X, int x_dtype, const void* F, int f_dtype, int64_t T, int32_t n,
                    const double* offsets, int64_t S, double width, const void* box, int32_t box_stride,
                    const void* out0, const void* out1, const void* ws, size_t ws_bytes, size_t need) {
  if (!X || !F || !offsets || !out0 || !out1 || !ws) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (!mv_dtype_ok(x_dtype) || !mv_dtype_ok(f_dtype)) return fail(AGGF_ERR_ARG, "%s: bad dtype", who);
  if (!mv_shape_ok(T, n)) return fail(AGGF_ERR_ARG, "%s: bad shape (T=%lld, n=%d)", who, (long long)T, n);
  if (!mv_samples_ok(S)) return fail(AGGF_ERR_ARG, "%s: bad sample count %lld", who, (long long)S);
  if (!(width > 0.0)) return fail(AGGF_ERR_ARG, "%s: width must be positive", who);
  if (ws_bytes < need - 256) return fail(AGGF_ERR_WORKSPACE, "%s: workspace too small", who);
  return mv_box(who, box, box_stride);
}

static int gauss_proj(const char* who, const void* X, int x_dtype, const void* F, int f_dtype, int64_t T, int32_t n,
                      const double* offsets, int64_t S, double width, const void* box, int32_t box_stride,
                      bool near, double* out, void* ws, size_t ws_bytes, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const size_t need = mv_shape_ok(T, n) && mv_samples_ok(S) ? proj_ws(T, n, S) : 256;
  const int rc = mv_check(who, X, x_dtype, F, f_dtype, T, n, offsets, S, width, box, box_stride, out, out,
                          ws, ws_bytes, need);
  if (rc != AGGF_OK) return rc;
  const SplitPlan p = split_plan(T * ((int64_t)n * (n - 1) / 2), MV_PL, S, 1);
  double* slabs = (double*)ws;
  if (x_dtype == AGGF_F64)
    launch_proj_x((const double*)X, F, f_dtype, T, n, offsets, S, width, p, slabs, box, box_stride, near, stream);
  else
    launch_proj_x((const float*)X, F, f_dtype, T, n, offsets, S, width, p, slabs, box, box_stride, near, stream);
  AGGF_LAUNCH_OK();
  const int64_t g = ceil_div(S, 256) < 1024 ? ceil_div(S, 256) : 1024;
  AGGF_LAUNCH(mapval_slab_reduce_kernel, dim3((unsigned)g), dim3(256), 0, stream, slabs, p.K, S, 1,
              8.0 / (width * width), 0.0, out, (double*)nullptr);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

static int gauss_shift(const char* who, const void* X, int x_dtype, const void* F, int f_dtype, int64_t T, int32_t n,
                      const double* offsets, int64_t S, double width, const void* box, int32_t box_stride,
                      bool near, double* ip, double* gsq, void* ws, size_t ws_bytes, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const size_t need = mv_shape_ok(T, n) && mv_samples_ok(S) ? shift_ws(T, S) : 256;
  const int rc = mv_check(who, X, x_dtype, F, f_dtype, T, n, offsets, S, width, box, box_stride, ip, gsq,
                          ws, ws_bytes, need);
  if (rc != AGGF_OK) return rc;
  const SplitPlan p = split_plan(T, 1, S, 2);
  double* slabs = (double*)ws;
  if (x_dtype == AGGF_F64)
    launch_shift_x((const double*)X, F, f_dtype, T, n, offsets, S, width, p, slabs, box, box_stride, near, stream);
  else
    launch_shift_x((const float*)X, F, f_dtype, T, n, offsets, S, width, p, slabs, box, box_stride, near, stream);
  AGGF_LAUNCH_OK();
  const double sc = 8.0 / (width * width);
  const int64_t g = ceil_div(S, 256) < 1024 ? ceil_div(S, 256) : 1024;
  AGGF_LAUNCH(mapval_slab_reduce_kernel, dim3((unsigned)g), dim3(256), 0, stream, slabs, p.K, S, 2, sc, sc * sc, ip,
              gsq);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

extern "C" int aggf_gauss_proj(const void* X, int x_dtype, const void* F, int f_dtype, int64_t T, int32_t n,
                               const double* offsets, int64_t S, double width, const void* box, int32_t box_stride,
                               double* out, void* ws, size_t ws_bytes, void* stream_v) {
  return gauss_proj("aggf_gauss_proj", X, x_dtype, F, f_dtype, T, n, offsets, S, width, box, box_stride, false, out, ws,
                    ws_bytes, stream_v);
}

extern "C" int aggf_gauss_proj_cell(const void* X, int x_dtype, const void* F, int f_dtype, int64_t T, int32_t n,
                                    const double* offsets, int64_t S, double width, const void* cell, double* out,
                                    void* ws, size_t ws_bytes, void* stream_v, int images) {
  const int rc = mv_cell_arg("aggf_gauss_proj_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return gauss_proj("aggf_gauss_proj_cell", X, x_dtype, F, f_dtype, T, n, offsets, S, width, cell, 9,
                    images == AGGF_IMAGES_NEAREST, out, ws, ws_bytes, stream_v);
}

extern "C" int aggf_gauss_shift(const void* X, int x_dtype, const void* F, int f_dtype, int64_t T, int32_t n,
                                const double* offsets, int64_t S, double width, const void* box, int32_t box_stride,
                                double* ip, double* gsq, void* ws, size_t ws_bytes, void* stream_v) {
  return gauss_shift("aggf_gauss_shift", X, x_dtype, F, f_dtype, T, n, offsets, S, width, box, box_stride, false, ip,
                     gsq, ws, ws_bytes, stream_v);
}

extern "C" int aggf_gauss_shift_cell(const void* X, int x_dtype, const void* F, int f_dtype, int64_t T, int32_t n,
                                     const double* offsets, int64_t S, double width, const void* cell, double* ip,
                                     double* gsq, void* ws, size_t ws_bytes, void* stream_v, int images) {
  const int rc = mv_cell_arg("aggf_gauss_shift_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return gauss_shift("aggf_gauss_shift_cell", X, x_dtype, F, f_dtype, T, n, offsets, S, width, cell, 9,
                     images == AGGF_IMAGES_NEAREST, ip, gsq, ws, ws_bytes, stream_v);
}

extern "C" size_t aggf_dot_workspace_bytes(void) { return MV_DOT_BLOCKS * sizeof(double); }

extern "C" int aggf_dot(const void* a, int a_dtype, const void* b, int b_dtype, int64_t count, double* out, void* ws,
                        size_t ws_bytes, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!a || !b || !out || !ws) return fail(AGGF_ERR_ARG, "aggf_dot: NULL pointer");
  if (!mv_dtype_ok(a_dtype) || !mv_dtype_ok(b_dtype)) return fail(AGGF_ERR_ARG, "aggf_dot: bad dtype");
  if (count < 0) return fail(AGGF_ERR_ARG, "aggf_dot: negative count");
  if (ws_bytes < MV_DOT_BLOCKS * sizeof(double)) return fail(AGGF_ERR_WORKSPACE, "aggf_dot: workspace too small");
  double* part = (double*)ws;
  const dim3 grid(MV_DOT_BLOCKS);
  if (a_dtype == AGGF_F64 && b_dtype == AGGF_F64)
    AGGF_LAUNCH((dot_kernel<double, double>), grid, dim3(256), 0, stream, (const double*)a, (const double*)b, count, part);
  else if (a_dtype == AGGF_F64)
    AGGF_LAUNCH((dot_kernel<double, float>), grid, dim3(256), 0, stream, (const double*)a, (const float*)b, count, part);
  else if (b_dtype == AGGF_F64)
    AGGF_LAUNCH((dot_kernel<float, double>), grid, dim3(256), 0, stream, (const float*)a, (const double*)b, count, part);
  else
    AGGF_LAUNCH((dot_kernel<float, float>), grid, dim3(256), 0, stream, (const float*)a, (const float*)b, count, part);
  AGGF_LAUNCH_OK();
  AGGF_LAUNCH(dot_finish_kernel, dim3(1), dim3(256), 0, stream, part, MV_DOT_BLOCKS, out);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}
