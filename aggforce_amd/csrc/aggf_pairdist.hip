// K9: differentiable pair distances (aggforce_amd/_autograd.py: PairDist, PairPull, PairDot).  With
// u[t,i,j] = X[t,j] - C[t,i] (X (T, n, 3), C (T, m, 3)), all arrays of one call in one dtype:
//
//   pairdist_kernel<T, MODE>   out[t,i,j] = sqrt(u.u) | u.u | (V[t,j] - Y[t,i]).u     the (T, m, n) array written once
//   pairpull_kernel            A[t,j,:] = sum_i w_ij u_ij,  B[t,i,:] = -sum_j w_ij u_ij, w = W or (Dv > 0 ? W / Dv : 0):
//                              W (and Dv) read once for both sums
//   pairpull_reduce_kernel     the column panels' partial row sums of B, added in ascending panel order
//
// No (T, m, n, 3) array exists anywhere.  Every sum has a fixed order and there are no atomics: results are
// bit-identical run to run.  Element offsets are 64-bit; base addresses need only element alignment.
#include "aggf_common.h"

namespace aggf {

// ---------------------------------------------------------------------------
// K9a.  One wave = one frame x `rows` rows x a panel of PD_COLS columns: a lane keeps the sites of its columns (lane,
// lane + 64, ...) in registers, the row's site has a wave-uniform address, and a row of the tile is PD_K stores of 64
// consecutive elements.  Waves walk the (frame, row block, panel) tasks in output order; `rows` is the launcher's
// choice (the whole frame unless that leaves too few tasks).
constexpr int PD_K = 4;
constexpr int PD_COLS = 64 * PD_K;
constexpr int PD_MIN_ROWS = 16;
constexpr int64_t PD_TARGET_TASKS = 16384;

template <typename T, int MODE>
__global__ __launch_bounds__(256) void pairdist_kernel(const T* __restrict__ X, const T* __restrict__ C,
                                                       const T* __restrict__ V, const T* __restrict__ Y, int64_t nT,
                                                       int32_t m, int32_t n, int32_t rows, T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t panels = ((int64_t)n + PD_COLS - 1) / PD_COLS, iblocks = ((int64_t)m + rows - 1) / rows;
  const int64_t ntask = nT * iblocks * panels;
  for (int64_t task = (int64_t)blockIdx.x * 4 + wave; task < ntask; task += (int64_t)gridDim.x * 4) {
    const int64_t r = task / panels, p = task - r * panels;
    const int64_t t = r / iblocks, ib = r - t * iblocks;
    const int64_t j0 = p * PD_COLS + lane;
    T x[PD_K][3], v[PD_K][3];
    bool live[PD_K];
#pragma unroll
    for (int k = 0; k < PD_K; ++k) {
      const int64_t j = j0 + 64 * k;
      live[k] = j < n;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        x[k][d] = live[k] ? X[(t * n + j) * 3 + d] : (T)0;
        v[k][d] = (MODE == AGGF_PAIR_DOT && live[k]) ? V[(t * n + j) * 3 + d] : (T)0;
      }
    }
    const int64_t i0 = ib * rows, i1 = i0 + rows < m ? i0 + rows : m;
    T* o = out + (t * m + i0) * n + j0;
    for (int64_t i = i0; i < i1; ++i, o += n) {
      const T* c = C + (t * m + i) * 3;
      const T c0 = c[0], c1 = c[1], c2 = c[2];
      T y0 = 0, y1 = 0, y2 = 0;
      if (MODE == AGGF_PAIR_DOT) {
        const T* y = Y + (t * m + i) * 3;
        y0 = y[0], y1 = y[1], y2 = y[2];
      }
#pragma unroll
      for (int k = 0; k < PD_K; ++k) {
        const T d0 = x[k][0] - c0, d1 = x[k][1] - c1, d2 = x[k][2] - c2;
        const T val = pair_element<T, MODE>(d0, d1, d2, v[k][0] - y0, v[k][1] - y1, v[k][2] - y2);
        if (live[k]) o[64 * k] = val;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// K9b.  One block = one frame x one panel of columns, all m rows; a panel is 1 KiB of a row of W (256 float32 or 128
// float64 columns: pp_cols).  A lane owns the panel's columns lane, lane + 64, ...: their column sums (A) stay in its
// registers over the rows its wave takes (PP_R consecutive rows at a time, the four waves side by side), summed in
// the input dtype over PP_FLUSH rows at a time and in float64 beyond; the four waves' sums are added in wave order
// through LDS.  A row's sum (B) over the panel is complete inside one wave: per lane over its columns, then over the
// lanes for PP_R rows at once (rows8_sum: three exchange steps halve the rows a lane carries, three more finish the
// one it is left with).  With one panel (n <= pp_cols) B is written directly, otherwise as float64 partials
// [frame][panel][row][3] that pairpull_reduce_kernel adds.  A panel with 64 or 128 columns left runs the same code
// with one or two chunks per lane; frames of at most PP_WAVE_ROWS rows go a frame per wave.
constexpr int PP_MAX_COLS = 256;
static constexpr int pp_cols(int dtype) { return dtype == AGGF_F32 ? 256 : 128; }
template <typename T>
struct PullPanel {
  static constexpr int K = sizeof(T) == 4 ? 4 : 2;  // 64-column chunks of a full panel
  static constexpr int COLS = 64 * K;
};
constexpr int PP_R = 8;
constexpr int PP_FLUSH = 16;
constexpr int PP_WAVE_ROWS = 128;

// v[r] of every lane summed over the wave's lanes, for the 8 rows r at once: 10 exchanges instead of 48.  On return
// v[0] of lane l holds the sum of row rows8_row(l).
template <int HALF, int DIST, typename T>
__device__ __forceinline__ void rows8_step(T (&v)[PP_R], bool hi) {
#pragma unroll
  for (int h = 0; h < HALF; ++h) {
    const T send = hi ? v[h] : v[h + HALF], keep = hi ? v[h + HALF] : v[h];
    v[h] = keep + __shfl_xor(send, DIST, 64);
  }
}
template <typename T>
__device__ __forceinline__ void rows8_sum(T (&v)[PP_R], int lane) {
  rows8_step<4, 1>(v, (lane & 1) != 0);
  rows8_step<2, 2>(v, (lane & 2) != 0);
  rows8_step<1, 4>(v, (lane & 4) != 0);
  v[0] += __shfl_xor(v[0], 8, 64);
  v[0] += __shfl_xor(v[0], 16, 64);
  v[0] += __shfl_xor(v[0], 32, 64);
}
__device__ __forceinline__ int rows8_row(int lane) { return ((lane >> 2) & 1) | (lane & 2) | ((lane & 1) << 2); }

// one (frame, panel) task with KC live 64-column chunks.  No branch on a lane's or a row's validity: a column beyond n
// or a row beyond m reads the last valid one and its term is replaced by 0 (a product with 0 would keep a NaN), so
// the loads of a whole batch of rows are in flight together.
// PER_WAVE (frames of at most PP_WAVE_ROWS rows): the wave takes all rows of the task, so A is complete in its
// registers and the block never synchronises; otherwise the block's four waves share the rows and add their sums in LDS.
template <typename TI, typename TO, bool HAS_DV, int KC, bool PER_WAVE>
__device__ __forceinline__ void pull_task(const TI* __restrict__ W, const TI* __restrict__ Dv,
                                          const TI* __restrict__ X, const TI* __restrict__ C, int64_t t, int64_t p,
                                          int32_t m, int32_t n, int64_t panels, TO* __restrict__ A,
                                          TO* __restrict__ B, double* __restrict__ partB, double (*sA)[PP_MAX_COLS * 3],
                                          int tid, int lane, int w) {
  constexpr bool WIDEN = sizeof(TI) < sizeof(double);  // float sums move to float64 every PP_FLUSH rows
  const int64_t j0 = p * PullPanel<TI>::COLS;
  TI x[KC][3], a[KC][3];
  double a64[KC][3];
  bool live[KC];
  int col[KC];  // the lane's columns within the panel
  const TI* wt = W + t * m * n + j0;
  const TI* dt = HAS_DV ? Dv + t * m * n + j0 : nullptr;
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    const int64_t j = j0 + 64 * k + lane;
    live[k] = j < n;
    const int64_t jc = live[k] ? j : n - 1;
    col[k] = (int)(jc - j0);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      x[k][d] = X[(t * n + jc) * 3 + d];
      a[k][d] = 0;
      a64[k][d] = 0.0;
    }
  }
  int pending = 0;
  for (int64_t ib = PER_WAVE ? 0 : (int64_t)w * PP_R; ib < m; ib += (PER_WAVE ? 1 : 4) * PP_R) {
    TI b[3][PP_R];
#pragma unroll
    for (int r = 0; r < PP_R; ++r) {
      b[0][r] = b[1][r] = b[2][r] = 0;
      const bool row = ib + r < m;  // (wave-uniform)
      const int64_t i = row ? ib + r : m - 1;
      const TI* c = C + (t * m + i) * 3;
      const TI c0 = c[0], c1 = c[1], c2 = c[2];
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        TI wv = wt[i * n + col[k]];
        if (HAS_DV) {
          const TI dv = dt[i * n + col[k]];
          const TI qv = wv / dv;  // (formed before the choice: a branch here would serialise the loads)
          wv = dv > (TI)0 ? qv : (TI)0;
        }
        const bool ok = row && live[k];
        const TI q0 = ok ? wv * (x[k][0] - c0) : (TI)0, q1 = ok ? wv * (x[k][1] - c1) : (TI)0,
                 q2 = ok ? wv * (x[k][2] - c2) : (TI)0;
        a[k][0] += q0, a[k][1] += q1, a[k][2] += q2;
        b[0][r] += q0, b[1][r] += q1, b[2][r] += q2;
      }
    }
    if (B != nullptr) {  // (block-uniform)
#pragma unroll
      for (int d = 0; d < 3; ++d) rows8_sum(b[d], lane);
      const int64_t i = ib + rows8_row(lane);
      if (lane < PP_R && i < m) {
        if (panels == 1) {
          TO* o = B + (t * m + i) * 3;
          o[0] = (TO)(-b[0][0]), o[1] = (TO)(-b[1][0]), o[2] = (TO)(-b[2][0]);
        } else {
          double* o = partB + ((t * panels + p) * m + i) * 3;
          o[0] = (double)b[0][0], o[1] = (double)b[1][0], o[2] = (double)b[2][0];
        }
      }
    }
    pending += PP_R;
    if (WIDEN && pending >= PP_FLUSH) {
      pending = 0;
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) a64[k][d] += (double)a[k][d], a[k][d] = 0;
    }
  }
  if (PER_WAVE) {
    if (A != nullptr)
#pragma unroll
      for (int k = 0; k < KC; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d)
          if (live[k]) A[(t * n + j0 + col[k]) * 3 + d] = (TO)(a64[k][d] + (double)a[k][d]);
  } else if (A != nullptr) {  // (block-uniform)
#pragma unroll
    for (int k = 0; k < KC; ++k)
#pragma unroll
      for (int d = 0; d < 3; ++d) sA[w][(64 * k + lane) * 3 + d] = a64[k][d] + (double)a[k][d];
    __syncthreads();
    const int64_t cols = n - j0 < 64 * KC ? n - j0 : 64 * KC;
    for (int e = tid; e < cols * 3; e += 256)
      A[(t * n + j0) * 3 + e] = (TO)(((sA[0][e] + sA[1][e]) + sA[2][e]) + sA[3][e]);
    __syncthreads();  // sA is free for the next task
  }
}

template <typename TI, typename TO, bool HAS_DV, bool PER_WAVE>
__device__ __forceinline__ void pull_tasks(const TI* __restrict__ W, const TI* __restrict__ Dv,
                                           const TI* __restrict__ X, const TI* __restrict__ C, int64_t nT, int32_t m,
                                           int32_t n, int64_t panels, TO* __restrict__ A, TO* __restrict__ B,
                                           double* __restrict__ partB, double (*sA)[PP_MAX_COLS * 3]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t first = PER_WAVE ? (int64_t)blockIdx.x * 4 + w : blockIdx.x;
  const int64_t step = PER_WAVE ? (int64_t)gridDim.x * 4 : gridDim.x;
  for (int64_t task = first; task < nT * panels; task += step) {
    const int64_t t = task / panels, p = task - t * panels;
    const int64_t left = n - p * PullPanel<TI>::COLS;  // the panel's live 64-column chunks: 1, 2 or a full panel's
    if (left <= 64)
      pull_task<TI, TO, HAS_DV, 1, PER_WAVE>(W, Dv, X, C, t, p, m, n, panels, A, B, partB, sA, tid, lane, w);
    else if (left <= 128 || PullPanel<TI>::K == 2)
      pull_task<TI, TO, HAS_DV, 2, PER_WAVE>(W, Dv, X, C, t, p, m, n, panels, A, B, partB, sA, tid, lane, w);
    else
      pull_task<TI, TO, HAS_DV, PullPanel<TI>::K, PER_WAVE>(W, Dv, X, C, t, p, m, n, panels, A, B, partB, sA, tid,
                                                            lane, w);
  }
}

template <typename TI, typename TO, bool HAS_DV>
__global__ __launch_bounds__(256) void pairpull_kernel(const TI* __restrict__ W, const TI* __restrict__ Dv,
                                                       const TI* __restrict__ X, const TI* __restrict__ C, int64_t nT,
                                                       int32_t m, int32_t n, int64_t panels, TO* __restrict__ A,
                                                       TO* __restrict__ B, double* __restrict__ partB) {
  __shared__ double sA[4][PP_MAX_COLS * 3];
  if (m <= PP_WAVE_ROWS)
    pull_tasks<TI, TO, HAS_DV, true>(W, Dv, X, C, nT, m, n, panels, A, B, partB, sA);
  else
    pull_tasks<TI, TO, HAS_DV, false>(W, Dv, X, C, nT, m, n, panels, A, B, partB, sA);
}

template <typename TO>
__global__ __launch_bounds__(256) void pairpull_reduce_kernel(const double* __restrict__ partB, int64_t nT, int64_t row,
                                                              int64_t panels, TO* __restrict__ B) {
  // row = 3 m values of one frame
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nT * row; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = e / row, r = e - t * row;
    const double* src = partB + t * panels * row + r;
    double s = 0.0;
    for (int64_t p = 0; p < panels; ++p) s += src[p * row];
    B[e] = (TO)(-s);
  }
}

static inline dim3 pair_grid(int64_t blocks) {
  if (blocks > 65536) blocks = 65536;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

// T m n as an element count; false if it does not fit int64
static bool pair_count(int64_t T, int32_t m, int32_t n, int64_t* count) {
  int64_t mn = (int64_t)m * n;
  return !__builtin_mul_overflow(T, mn, count);
}

// bytes of the float64 B partials (0 with a single column panel); false if they do not fit
static bool pull_ws_bytes(int64_t T, int32_t m, int32_t n, int in_dtype, size_t* bytes) {
  *bytes = 0;
  const int64_t panels = ceil_div(n, pp_cols(in_dtype));
  if (panels <= 1) return true;
  int64_t v;
  if (__builtin_mul_overflow(T, panels * m, &v) || __builtin_mul_overflow(v, (int64_t)(3 * sizeof(double)), &v) ||
      v > INT64_MAX - 256)
    return false;
  *bytes = (size_t)round_up(v, 256);
  return true;
}

static int pair_shape(const char* who, int64_t T, int32_t m, int32_t n, int64_t* count) {
  if (T < 0 || m < 0 || n < 0) return fail(AGGF_ERR_ARG, "%s: negative shape", who);
  if (!pair_count(T, m, n, count) || *count > INT64_MAX / 8)
    return fail(AGGF_ERR_ARG, "%s: T m n does not fit a 64-bit byte offset", who);
  return AGGF_OK;
}

template <typename T>
static void launch_pairdist(int mode, dim3 grid, hipStream_t stream, const void* X, const void* C, const void* V,
                            const void* Y, int64_t nT, int32_t m, int32_t n, int32_t rows, void* out) {
  const dim3 block(256);
  if (mode == AGGF_PAIR_DIST)
    AGGF_LAUNCH((pairdist_kernel<T, AGGF_PAIR_DIST>), grid, block, 0, stream, (const T*)X, (const T*)C, (const T*)V,
                (const T*)Y, nT, m, n, rows, (T*)out);
  else if (mode == AGGF_PAIR_SQDIST)
    AGGF_LAUNCH((pairdist_kernel<T, AGGF_PAIR_SQDIST>), grid, block, 0, stream, (const T*)X, (const T*)C, (const T*)V,
                (const T*)Y, nT, m, n, rows, (T*)out);
  else
    AGGF_LAUNCH((pairdist_kernel<T, AGGF_PAIR_DOT>), grid, block, 0, stream, (const T*)X, (const T*)C, (const T*)V,
                (const T*)Y, nT, m, n, rows, (T*)out);
}

template <typename TI, typename TO>
static void launch_pairpull(dim3 grid, hipStream_t stream, const void* W, const void* Dv, const void* X, const void* C,
                            int64_t nT, int32_t m, int32_t n, int64_t panels, void* A, void* B, double* part) {
  const dim3 block(256);
  if (Dv)
    AGGF_LAUNCH((pairpull_kernel<TI, TO, true>), grid, block, 0, stream, (const TI*)W, (const TI*)Dv, (const TI*)X,
                (const TI*)C, nT, m, n, panels, (TO*)A, (TO*)B, part);
  else
    AGGF_LAUNCH((pairpull_kernel<TI, TO, false>), grid, block, 0, stream, (const TI*)W, (const TI*)nullptr,
                (const TI*)X, (const TI*)C, nT, m, n, panels, (TO*)A, (TO*)B, part);
}

}  // namespace aggf

using namespace aggf;

extern "C" int aggf_pair_dist(const void* X, const void* C, const void* V, const void* Y, int64_t T, int32_t m,
                              int32_t n, int dtype, int mode, void* out, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  int64_t count = 0;
  const int rc = pair_shape("aggf_pair_dist", T, m, n, &count);
  if (rc != AGGF_OK) return rc;
  if (dtype != AGGF_F32 && dtype != AGGF_F64) return fail(AGGF_ERR_ARG, "aggf_pair_dist: bad dtype");
  if (mode != AGGF_PAIR_DIST && mode != AGGF_PAIR_SQDIST && mode != AGGF_PAIR_DOT)
    return fail(AGGF_ERR_ARG, "aggf_pair_dist: bad mode");
  if (count == 0) return AGGF_OK;
  if (!X || !C || !out) return fail(AGGF_ERR_ARG, "aggf_pair_dist: NULL pointer");
  if (mode == AGGF_PAIR_DOT && (!V || !Y)) return fail(AGGF_ERR_ARG, "aggf_pair_dist: DOT needs V and Y");
  // a wave takes a panel's whole column of rows unless that leaves the chip short of tasks
  const int64_t panels = ceil_div(n, PD_COLS);
  int32_t rows = m;
  while (rows > PD_MIN_ROWS && T * panels * ceil_div(m, rows) < PD_TARGET_TASKS) rows = (rows + 1) / 2;
  const int64_t waves = T * panels * ceil_div(m, rows);  // <= count
  const dim3 grid = pair_grid(ceil_div(waves, 4));
  if (dtype == AGGF_F64)
    launch_pairdist<double>(mode, grid, stream, X, C, V, Y, T, m, n, rows, out);
  else
    launch_pairdist<float>(mode, grid, stream, X, C, V, Y, T, m, n, rows, out);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

extern "C" size_t aggf_pair_pull_workspace_bytes(int64_t T, int32_t m, int32_t n, int in_dtype) {
  size_t bytes = 0;
  if (T <= 0 || m <= 0 || n <= 0 || !pull_ws_bytes(T, m, n, in_dtype, &bytes)) return 0;
  return bytes;
}

extern "C" int aggf_pair_pull(const void* W, const void* Dv, const void* X, const void* C, int64_t T, int32_t m,
                              int32_t n, int in_dtype, void* A, void* B, int out_dtype, void* ws, size_t ws_bytes,
                              void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  int64_t count = 0;
  const int rc = pair_shape("aggf_pair_pull", T, m, n, &count);
  if (rc != AGGF_OK) return rc;
  if ((in_dtype != AGGF_F32 && in_dtype != AGGF_F64) || (out_dtype != AGGF_F32 && out_dtype != AGGF_F64))
    return fail(AGGF_ERR_ARG, "aggf_pair_pull: bad dtype");
  if (in_dtype == AGGF_F32 && out_dtype == AGGF_F64)
    return fail(AGGF_ERR_ARG, "aggf_pair_pull: float32 inputs with float64 outputs: widen the inputs");
  if (count == 0 || (!A && !B)) return AGGF_OK;
  if (!W || !X || !C) return fail(AGGF_ERR_ARG, "aggf_pair_pull: NULL pointer");
  const int64_t panels = ceil_div(n, pp_cols(in_dtype));
  size_t need = 0;
  if (!pull_ws_bytes(T, m, n, in_dtype, &need)) return fail(AGGF_ERR_ARG, "aggf_pair_pull: workspace size overflows");
  const bool partials = B && panels > 1;
  if (partials && (!ws || ws_bytes < need || ((uintptr_t)ws & 7))) return fail(AGGF_ERR_WORKSPACE, "aggf_pair_pull: workspace too small");
  int64_t tasks = 0;
  if (__builtin_mul_overflow(T, panels, &tasks)) return fail(AGGF_ERR_ARG, "aggf_pair_pull: too many tasks");
  const dim3 grid = pair_grid(m <= PP_WAVE_ROWS ? ceil_div(tasks, 4) : tasks);  // a task per wave, or per block
  double* part = partials ? (double*)ws : nullptr;
  if (in_dtype == AGGF_F32)
    launch_pairpull<float, float>(grid, stream, W, Dv, X, C, T, m, n, panels, A, B, part);
  else if (out_dtype == AGGF_F32)
    launch_pairpull<double, float>(grid, stream, W, Dv, X, C, T, m, n, panels, A, B, part);
  else
    launch_pairpull<double, double>(grid, stream, W, Dv, X, C, T, m, n, panels, A, B, part);
  AGGF_LAUNCH_OK();
  if (partials) {
    const int64_t row = 3 * (int64_t)m;
    const dim3 rgrid = pair_grid(ceil_div(T * row, 256)), block(256);
    if (out_dtype == AGGF_F32)
      AGGF_LAUNCH((pairpull_reduce_kernel<float>), rgrid, block, 0, stream, (const double*)ws, T, row, panels, (float*)B);
    else
      AGGF_LAUNCH((pairpull_reduce_kernel<double>), rgrid, block, 0, stream, (const double*)ws, T, row, panels,
                  (double*)B);
    AGGF_LAUNCH_OK();
  }
  return AGGF_OK;
}
