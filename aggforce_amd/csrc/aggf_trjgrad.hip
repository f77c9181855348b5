// K8: the backward contractions of map application (aggforce_amd/_autograd.py).  Every sum is accumulated in a fixed
// order, partial sums are combined in float64, there are no atomics: results are bit-identical run to run.
//
//   trjdot_cross_kernel      map gradient, out[i,j] = sum_{t,d} A[t,i,d] B[t,j,d]: 64 x 64 output tiles on
//                            v_mfma_*_16x16x4 (2 x 2 per wave), frames staged 16 at a time in LDS (register prefetch of
//                            the next block), split over frame blocks into float64 partial tiles
//   trjdot_cross_reduce      the splits summed in ascending order in float64 (out += when accumulating)
//   trjdot_frames_t_kernel   out[t,a,d] = sum_c F[t,c,a] G[t,c,d]     (transpose of K3c)
//   trjdot_frames_outer      out[t,c,a] = sum_d G[t,c,d] P[t,a,d]     (rank-3 gradient of a per-frame factor)
#include "aggf_common.h"

namespace aggf {

constexpr int XT = 64;         // output tile edge (rows of A and of B)
constexpr int XKF = 16;        // frames per LDS stage: 48 reduction steps, 12 MFMA k-steps
constexpr int XROW = XT * 3;   // one frame of a tile: 192 contiguous elements
constexpr int XPER = XKF * XROW / 256;  // staged elements per thread and operand
constexpr int64_t X_TARGET_BLOCKS = 2048;
constexpr int64_t X_MAX_SPLITS = 1024;
constexpr int X_MIN_FBLK_PER_SPLIT = 8;

struct CrossPlan {
  int64_t tiles_a, tiles_b, splits, frames_per_split;
};

// the one plan of aggf_trjdot_cross and of its workspace query: a function of the shape alone
static CrossPlan cross_plan(int64_t T, int32_t n_a, int32_t n_b) {
  CrossPlan p;
  p.tiles_a = ceil_div(n_a, XT);
  p.tiles_b = ceil_div(n_b, XT);
  const int64_t tiles = p.tiles_a * p.tiles_b;
  const int64_t fblk = ceil_div(T, XKF);
  int64_t s = ceil_div(X_TARGET_BLOCKS, tiles);
  const int64_t s_cap = ceil_div(fblk, X_MIN_FBLK_PER_SPLIT);
  if (s > s_cap) s = s_cap;
  if (s > X_MAX_SPLITS) s = X_MAX_SPLITS;
  if (s < 1) s = 1;
  p.frames_per_split = ceil_div(fblk, s) * XKF;
  p.splits = ceil_div(T, p.frames_per_split);  // no empty split
  return p;
}

static size_t cross_ws_bytes(const CrossPlan& p, int32_t n_a, int32_t n_b) {
  return (size_t)round_up(p.splits * (int64_t)n_a * n_b * (int64_t)sizeof(double), 256);
}

template <typename T>
__global__ __launch_bounds__(256) void trjdot_cross_kernel(const T* __restrict__ A, const T* __restrict__ B, int64_t nT,
                                                           int32_t n_a, int32_t n_b, int64_t tiles_b,
                                                           int64_t frames_per_split, double* __restrict__ part) {
  __shared__ T sA[XKF][XROW];
  __shared__ T sB[XKF][XROW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t ta = blockIdx.x / tiles_b, tb = blockIdx.x - ta * tiles_b;
  const int64_t i0 = ta * XT, j0 = tb * XT;
  const int64_t t_begin = (int64_t)blockIdx.y * frames_per_split;
  const int64_t t_end = t_begin + frames_per_split < nT ? t_begin + frames_per_split : nT;
  const int va = (int)((n_a - i0 < XT ? n_a - i0 : XT) * 3);  // valid elements of one frame row of the tile
  const int vb = (int)((n_b - j0 < XT ? n_b - j0 : XT) * 3);

  T ra[XPER], rb[XPER];
  auto fetch = [&](int64_t t0) {
#pragma unroll
    for (int r = 0; r < XPER; ++r) {
      const int e = tid + 256 * r, f = e / XROW, off = e - f * XROW;
      const int64_t t = t0 + f;
      ra[r] = (t < t_end && off < va) ? A[(t * n_a + i0) * 3 + off] : (T)0;
      rb[r] = (t < t_end && off < vb) ? B[(t * n_b + j0) * 3 + off] : (T)0;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int r = 0; r < XPER; ++r) {
      const int e = tid + 256 * r, f = e / XROW, off = e - f * XROW;
      sA[f][off] = ra[r];
      sB[f][off] = rb[r];
    }
  };

  typename Mfma<T>::acc_t acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = acc_zero<T>();
  const int wr = w >> 1, wc = w & 1, li = lane & 15, lk = lane >> 4;

  fetch(t_begin);
  for (int64_t t0 = t_begin; t0 < t_end; t0 += XKF) {
    __syncthreads();  // the previous stage has been read
    store();
    __syncthreads();
    if (t0 + XKF < t_end) fetch(t0 + XKF);  // next stage in flight during the MFMAs
#pragma unroll
    for (int s = 0; s < XKF * 3 / 4; ++s) {
      const int k = 4 * s + lk, f = k / 3, d = k - 3 * f;
      T a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = sA[f][(wr * 32 + m * 16 + li) * 3 + d];
#pragma unroll
      for (int n = 0; n < 2; ++n) b[n] = sB[f][(wc * 32 + n * 16 + li) * 3 + d];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = Mfma<T>::mma(a[m], b[n], acc[m][n]);
    }
  }

  double* dst = part + (int64_t)blockIdx.y * n_a * n_b;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + wr * 32 + m * 16 + Mfma<T>::row(lane, r);
        const int64_t j = j0 + wc * 32 + n * 16 + li;
        if (i < n_a && j < n_b) dst[i * n_b + j] = (double)acc[m][n][r];
      }
}

template <typename TO>
__global__ __launch_bounds__(256) void trjdot_cross_reduce(const double* __restrict__ part, int64_t splits, int64_t n,
                                                           int accumulate, TO* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    double s = accumulate ? (double)out[e] : 0.0;
    double v = 0.0;
    for (int64_t k = 0; k < splits; ++k) v += part[k * n + e];
    out[e] = (TO)(s + v);
  }
}

// ---------------------------------------------------------------------------
// K8b / K8c: one block = one frame x 256 consecutive fine sites a; G[t] is staged in LDS 256 cg rows at a time.
constexpr int FG_ROWS = 256;

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void trjdot_frames_t_kernel(const TI* __restrict__ G, const TI* __restrict__ F,
                                                              int64_t nT, int32_t n_cg, int32_t N,
                                                              TO* __restrict__ out) {
  __shared__ double sG[FG_ROWS * 3];
  const int64_t chunks = ((int64_t)N + 255) / 256;
  for (int64_t task = blockIdx.x; task < nT * chunks; task += gridDim.x) {
    const int64_t t = task / chunks;
    const int64_t a = (task - t * chunks) * 256 + threadIdx.x;
    const TI* g = G + t * n_cg * 3;
    const TI* f = F + t * n_cg * (int64_t)N;
    double x = 0.0, y = 0.0, z = 0.0;
    for (int c0 = 0; c0 < n_cg; c0 += FG_ROWS) {
      const int rows = n_cg - c0 < FG_ROWS ? n_cg - c0 : FG_ROWS;
      __syncthreads();
      for (int e = threadIdx.x; e < rows * 3; e += 256) sG[e] = (double)g[(int64_t)c0 * 3 + e];
      __syncthreads();
      if (a < N) {
        const TI* fc = f + (int64_t)c0 * N + a;
        for (int c = 0; c < rows; ++c) {
          const double v = (double)fc[(int64_t)c * N];
          x = fma(v, sG[3 * c + 0], x);
          y = fma(v, sG[3 * c + 1], y);
          z = fma(v, sG[3 * c + 2], z);
        }
      }
    }
    if (a < N) {
      TO* o = out + (t * N + a) * 3;
      o[0] = (TO)x;
      o[1] = (TO)y;
      o[2] = (TO)z;
    }
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void trjdot_frames_outer_kernel(const TI* __restrict__ G, const TI* __restrict__ P,
                                                                  int64_t nT, int32_t n_cg, int32_t N,
                                                                  TO* __restrict__ out) {
  __shared__ double sG[FG_ROWS * 3];
  const int64_t chunks = ((int64_t)N + 255) / 256;
  for (int64_t task = blockIdx.x; task < nT * chunks; task += gridDim.x) {
    const int64_t t = task / chunks;
    const int64_t a = (task - t * chunks) * 256 + threadIdx.x;
    const TI* g = G + t * n_cg * 3;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (a < N) {
      const TI* p = P + (t * N + a) * 3;
      px = (double)p[0];
      py = (double)p[1];
      pz = (double)p[2];
    }
    TO* o = out + t * n_cg * (int64_t)N + a;
    for (int c0 = 0; c0 < n_cg; c0 += FG_ROWS) {
      const int rows = n_cg - c0 < FG_ROWS ? n_cg - c0 : FG_ROWS;
      __syncthreads();
      for (int e = threadIdx.x; e < rows * 3; e += 256) sG[e] = (double)g[(int64_t)c0 * 3 + e];
      __syncthreads();
      if (a < N)
        for (int c = 0; c < rows; ++c)
          o[(int64_t)(c0 + c) * N] = (TO)fma(sG[3 * c + 2], pz, fma(sG[3 * c + 1], py, sG[3 * c] * px));
    }
  }
}

static inline dim3 grad_grid(int64_t blocks) {
  if (blocks > 65536) blocks = 65536;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

}  // namespace aggf

using namespace aggf;

extern "C" size_t aggf_trjdot_cross_workspace_bytes(int64_t T, int32_t n_a, int32_t n_b, int in_dtype) {
  (void)in_dtype;  // partial tiles are float64 for both input dtypes
  if (T <= 0 || n_a <= 0 || n_b <= 0) return 0;
  return cross_ws_bytes(cross_plan(T, n_a, n_b), n_a, n_b);
}

extern "C" int aggf_trjdot_cross(const void* A, const void* B, int64_t T, int32_t n_a, int32_t n_b, int in_dtype,
                                 void* out, int out_dtype, int accumulate, void* ws, size_t ws_bytes, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!A || !B || !out) return fail(AGGF_ERR_ARG, "aggf_trjdot_cross: NULL pointer");
  if (T <= 0 || n_a <= 0 || n_b <= 0) return fail(AGGF_ERR_ARG, "aggf_trjdot_cross: empty problem");
  if ((in_dtype != AGGF_F32 && in_dtype != AGGF_F64) || (out_dtype != AGGF_F32 && out_dtype != AGGF_F64))
    return fail(AGGF_ERR_ARG, "aggf_trjdot_cross: bad dtype");
  const CrossPlan p = cross_plan(T, n_a, n_b);
  if (p.tiles_a * p.tiles_b > 0x7fffffff) return fail(AGGF_ERR_ARG, "aggf_trjdot_cross: too many output tiles");
  if (!ws || ws_bytes < cross_ws_bytes(p, n_a, n_b)) return fail(AGGF_ERR_WORKSPACE, "aggf_trjdot_cross: workspace too small");
  const dim3 grid((unsigned)(p.tiles_a * p.tiles_b), (unsigned)p.splits), block(256);
  if (in_dtype == AGGF_F64)
    AGGF_LAUNCH((trjdot_cross_kernel<double>), grid, block, 0, stream, (const double*)A, (const double*)B, T, n_a, n_b,
                p.tiles_b, p.frames_per_split, (double*)ws);
  else
    AGGF_LAUNCH((trjdot_cross_kernel<float>), grid, block, 0, stream, (const float*)A, (const float*)B, T, n_a, n_b,
                p.tiles_b, p.frames_per_split, (double*)ws);
  AGGF_LAUNCH_OK();
  const int64_t n = (int64_t)n_a * n_b;
  const dim3 rgrid = grad_grid(ceil_div(n, 256));
  if (out_dtype == AGGF_F64)
    AGGF_LAUNCH((trjdot_cross_reduce<double>), rgrid, block, 0, stream, (const double*)ws, p.splits, n, accumulate,
                (double*)out);
  else
    AGGF_LAUNCH((trjdot_cross_reduce<float>), rgrid, block, 0, stream, (const double*)ws, p.splits, n, accumulate,
                (float*)out);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

// in_dtype: both inputs; out_dtype: float32 or float64, but not wider than the inputs (widen them instead)
static int frames_args(const char* who, const void* x, const void* y, const void* out, int64_t T, int32_t n_cg,
                       int32_t N, int in_dtype, int out_dtype) {
  if (!x || !y || !out) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (T <= 0 || n_cg <= 0 || N <= 0) return fail(AGGF_ERR_ARG, "%s: empty problem", who);
  if ((in_dtype != AGGF_F32 && in_dtype != AGGF_F64) || (out_dtype != AGGF_F32 && out_dtype != AGGF_F64))
    return fail(AGGF_ERR_ARG, "%s: bad dtype", who);
  if (in_dtype == AGGF_F32 && out_dtype == AGGF_F64)
    return fail(AGGF_ERR_ARG, "%s: float32 inputs with a float64 output: widen the inputs", who);
  return AGGF_OK;
}

extern "C" int aggf_trjdot_frames_t(const void* G, const void* F, int in_dtype, int64_t T, int32_t n_cg, int32_t N,
                                    void* out, int out_dtype, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const int rc = frames_args("aggf_trjdot_frames_t", G, F, out, T, n_cg, N, in_dtype, out_dtype);
  if (rc != AGGF_OK) return rc;
  const dim3 grid = grad_grid(T * ceil_div(N, 256)), block(256);
  if (in_dtype == AGGF_F32)
    AGGF_LAUNCH((trjdot_frames_t_kernel<float, float>), grid, block, 0, stream, (const float*)G, (const float*)F, T,
                n_cg, N, (float*)out);
  else if (out_dtype == AGGF_F32)
    AGGF_LAUNCH((trjdot_frames_t_kernel<double, float>), grid, block, 0, stream, (const double*)G, (const double*)F, T,
                n_cg, N, (float*)out);
  else
    AGGF_LAUNCH((trjdot_frames_t_kernel<double, double>), grid, block, 0, stream, (const double*)G, (const double*)F,
                T, n_cg, N, (double*)out);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

extern "C" int aggf_trjdot_frames_outer(const void* G, const void* P, int in_dtype, int64_t T, int32_t n_cg,
                                        int32_t N, void* out, int out_dtype, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const int rc = frames_args("aggf_trjdot_frames_outer", G, P, out, T, n_cg, N, in_dtype, out_dtype);
  if (rc != AGGF_OK) return rc;
  const dim3 grid = grad_grid(T * ceil_div(N, 256)), block(256);
  if (in_dtype == AGGF_F32)
    AGGF_LAUNCH((trjdot_frames_outer_kernel<float, float>), grid, block, 0, stream, (const float*)G, (const float*)P,
                T, n_cg, N, (float*)out);
  else if (out_dtype == AGGF_F32)
    AGGF_LAUNCH((trjdot_frames_outer_kernel<double, float>), grid, block, 0, stream, (const double*)G,
                (const double*)P, T, n_cg, N, (float*)out);
  else
    AGGF_LAUNCH((trjdot_frames_outer_kernel<double, double>), grid, block, 0, stream, (const double*)G,
                (const double*)P, T, n_cg, N, (double*)out);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}
