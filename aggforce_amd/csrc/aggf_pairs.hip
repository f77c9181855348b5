// K6: pair-distance fluctuation statistics for guess_pairwise_constraints.
//
// Replaces constraints/constfinder.py:46-53 of the reference -- util.distances (util.py:65-72)
// materialises the (T, N, N) distance tensor and takes np.var over frames; here one streaming pass
// accumulates, for every pair i < j, sum_t (d_t - d_0) and sum_t (d_t - d_0)^2 with d_0 the
// distance in the first frame (shifted sums: no cancellation for rigid pairs), from which
//     var[i,j] = E[(d-d0)^2] - E[d-d0]^2.
// One workgroup = one 64x64 tile of pairs x one frame range; thread = 4x4 pairs in registers;
// 8 frames of the two 64-atom position blocks are staged in LDS per barrier.  Partial sums per
// frame range go to slabs and are combined in a fixed order (deterministic).
//
// pair_stats_pbc_kernel / pair_var_pbc_kernel: the same two under an orthorhombic box per frame (`box` (T, 3) with
// bstride 3, or (3,) with bstride 0, in the coordinates' dtype and widened as they are): every displacement component
// is replaced by its minimum image in float64 (min_image, aggf_common.h), d_0 included -- the minimum-image distance
// of frame 0 under frame 0's box.  L and 1/L of the 8 staged frames are formed once per stage (box_lengths) and kept
// in LDS beside the positions.  A frame whose box is bad is NaN, and with it every off-diagonal variance (the
// diagonal stays 0).  Each pair of kernels shares one __device__ body; the open ones keep their names, arguments and
// bits, and both forms share the plan, the slabs and the reduction order.
#include "aggf_common.h"

namespace aggf {

constexpr int PT = 64;   // pair tile edge
constexpr int PFB = 8;   // frames per LDS stage

// The roundings of K6, written out for the reason pair_dot3's are: left to the compiler's contraction, the 16 pairs of
// a thread do not all get the same fused form, and the two threads that hold (i, j) and (j, i) of a diagonal tile --
// or the open and the box kernel -- then differ in the last bit.  |u| = sqrt(fma(uz, uz, fma(ux, ux, uy uy))), the
// shifted sums s1 += dd, s2 = fma(dd, dd, s2), and var = fma(-m, m, q / T): the forms these kernels have always had.
__device__ __forceinline__ double pair_norm(double ux, double uy, double uz) {
  return sqrt(pair_dot3(ux, ux, uy, uy, uz, uz));
}

// the three widened lengths of one frame's box, and their inverses (box_lengths in float64)
template <typename TIn>
__device__ __forceinline__ bool box_lengths_wide(const TIn* __restrict__ box, double L[3], double invL[3]) {
  const double b[3] = {(double)box[0], (double)box[1], (double)box[2]};
  return box_lengths(b, L, invL);
}

// one displacement under the form's cell: L / iL for a box, h for a triclinic cell
template <int CELL>
__device__ __forceinline__ void pair_wrap(double& dx, double& dy, double& dz, const double L[3], const double iL[3],
                                          const CellFrame<double>& h) {
  if (CELL == CELL_BOX) dx = min_image(dx, L[0], iL[0]), dy = min_image(dy, L[1], iL[1]), dz = min_image(dz, L[2], iL[2]);
  if (CELL == CELL_TRI) brick_image(dx, dy, dz, h);
}

template <typename TIn, int CELL>
__device__ __forceinline__ void pair_stats_body(const TIn* __restrict__ X, int64_t T, int32_t N, int32_t nt1,
                                                int32_t n_tiles, int64_t frames_per_split,
                                                const TIn* __restrict__ box, int32_t bstride,
                                                double* __restrict__ slabs) {
  __shared__ double sp[2][PFB][PT][3];    // [i-block | j-block][frame][atom][xyz]
  __shared__ double sb[CELL == CELL_BOX ? PFB : 1][6];          // box: [frame][L xyz | 1/L xyz]
  __shared__ CellFrame<double> sc[CELL == CELL_TRI ? PFB : 1];  // triclinic: [frame] six entries and three inverses
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int ks = b / n_tiles;
  int idx = b - ks * n_tiles, ti = 0;
  {
    int rowlen = nt1;
    while (idx >= rowlen) {
      idx -= rowlen;
      --rowlen;
      ++ti;
    }
  }
  const int tj = ti + idx;
  const int tile_lin = b - ks * n_tiles;
  const int64_t t_begin = (int64_t)ks * frames_per_split;
  int64_t t_end = t_begin + frames_per_split;
  if (t_end > T) t_end = T;
  const int bi = (tid >> 4) * 4, bj = (tid & 15) * 4;  // this thread's 4x4 pairs inside the tile

  auto load_atom = [&](int64_t t, int a, double out[3]) {
    if (a < N) {
      const TIn* p = X + (t * N + a) * 3;
      out[0] = (double)p[0];
      out[1] = (double)p[1];
      out[2] = (double)p[2];
    } else {
      out[0] = out[1] = out[2] = 0.0;
    }
  };
  // reference distances d0 from frame 0
  double d0[4][4];
  {
    double pi[4][3], pj[4][3];
    for (int x = 0; x < 4; ++x) load_atom(0, ti * PT + bi + x, pi[x]);
    for (int y = 0; y < 4; ++y) load_atom(0, tj * PT + bj + y, pj[y]);
    double L[3] = {0, 0, 0}, iL[3] = {0, 0, 0};
    CellFrame<double> h = {};
    if (CELL == CELL_BOX) box_lengths_wide(box, L, iL);  // frame 0's box
    if (CELL == CELL_TRI) cell_frame(box, h);
    for (int x = 0; x < 4; ++x)
      for (int y = 0; y < 4; ++y) {
        double dx = pj[y][0] - pi[x][0], dy = pj[y][1] - pi[x][1], dz = pj[y][2] - pi[x][2];
        pair_wrap<CELL>(dx, dy, dz, L, iL, h);
        d0[x][y] = pair_norm(dx, dy, dz);
      }
  }
  double s1[4][4], s2[4][4];
  for (int x = 0; x < 4; ++x)
    for (int y = 0; y < 4; ++y) s1[x][y] = s2[x][y] = 0.0;

  for (int64_t t0 = t_begin; t0 < t_end; t0 += PFB) {
    __syncthreads();
    for (int e = tid; e < 2 * PFB * PT * 3; e += 256) {
      const int side = e / (PFB * PT * 3), r = e - side * (PFB * PT * 3);
      const int f = r / (PT * 3), q = r - f * (PT * 3);
      const int a = (side ? tj : ti) * PT + q / 3;
      const int64_t t = t0 + f;
      double v = 0.0;
      if (t < t_end && a < N) v = (double)X[(t * N + a) * 3 + q % 3];
      (&sp[side][f][0][0])[q] = v;
    }
    if (CELL != CELL_OPEN && tid < PFB) {  // (frames past t_end are staged but never read)
      const int64_t t = t0 + tid;
      if (CELL == CELL_BOX && t < t_end) box_lengths_wide(box + t * bstride, &sb[tid][0], &sb[tid][3]);
      if (CELL == CELL_TRI && t < t_end) cell_frame(box + t * 9, sc[tid]);
    }
    __syncthreads();
    const int nf = (int)((t_end - t0) < PFB ? (t_end - t0) : PFB);
    for (int f = 0; f < nf; ++f) {
      double L[3] = {0, 0, 0}, iL[3] = {0, 0, 0};
      CellFrame<double> h = {};
      if (CELL == CELL_BOX) {
#pragma unroll
        for (int k = 0; k < 3; ++k) L[k] = sb[f][k], iL[k] = sb[f][3 + k];
      }
      if (CELL == CELL_TRI) h = sc[f];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double ax = sp[0][f][bi + x][0], ay = sp[0][f][bi + x][1], az = sp[0][f][bi + x][2];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          double dx = sp[1][f][bj + y][0] - ax, dy = sp[1][f][bj + y][1] - ay, dz = sp[1][f][bj + y][2] - az;
          pair_wrap<CELL>(dx, dy, dz, L, iL, h);
          const double dd = pair_norm(dx, dy, dz) - d0[x][y];
          s1[x][y] += dd;
          s2[x][y] = __builtin_fma(dd, dd, s2[x][y]);
        }
      }
    }
  }
  const int ksplit = gridDim.x / n_tiles;
  double* slab = slabs + ((int64_t)tile_lin * ksplit + ks) * (2 * PT * PT);
  for (int x = 0; x < 4; ++x)
    for (int y = 0; y < 4; ++y) {
      slab[(bi + x) * PT + bj + y] = s1[x][y];
      slab[PT * PT + (bi + x) * PT + bj + y] = s2[x][y];
    }
}

template <typename TIn>
__global__ __launch_bounds__(256) void pair_stats_kernel(const TIn* __restrict__ X, int64_t T, int32_t N,
                                                         int32_t nt1, int32_t n_tiles,
                                                         int64_t frames_per_split,
                                                         double* __restrict__ slabs) {
  pair_stats_body<TIn, CELL_OPEN>(X, T, N, nt1, n_tiles, frames_per_split, nullptr, 0, slabs);
}

template <typename TIn>
__global__ __launch_bounds__(256) void pair_stats_pbc_kernel(const TIn* __restrict__ X, int64_t T, int32_t N,
                                                             int32_t nt1, int32_t n_tiles,
                                                             int64_t frames_per_split,
                                                             const TIn* __restrict__ box, int32_t bstride,
                                                             double* __restrict__ slabs) {
  pair_stats_body<TIn, CELL_BOX>(X, T, N, nt1, n_tiles, frames_per_split, box, bstride, slabs);
}

// cell: (T, 9), a row-major 3 x 3 triclinic cell per frame in the coordinates' dtype (brick_image in float64)
// (two workgroups per CU, the box form's occupancy: without the bound the nine cell numbers take it to one)
// The triclinic form is an overload with a second template argument (CELL_TRI, the only value instantiated).
template <typename TIn, int CELL>
__global__ __launch_bounds__(256, 2) void pair_stats_pbc_kernel(const TIn* __restrict__ X, int64_t T, int32_t N,
                                                                int32_t nt1, int32_t n_tiles,
                                                                int64_t frames_per_split,
                                                                const TIn* __restrict__ cell,
                                                                double* __restrict__ slabs) {
  static_assert(CELL == CELL_TRI, "the triclinic form");
  pair_stats_body<TIn, CELL>(X, T, N, nt1, n_tiles, frames_per_split, cell, 9, slabs);
}

// var[i,j] (N x N, symmetric, diagonal 0) from the slabs, fixed summation order
// mean (optional): mean distance over the frames = d0 + shifted mean, d0 recomputed from frame 0 of X (PBC: its
// minimum image under frame 0's box, as the statistics kernel formed it)
template <typename TIn, int CELL>
__device__ __forceinline__ void pair_var_body(const double* __restrict__ slabs, int32_t nt1, int32_t ksplit,
                                              int32_t N, int64_t T, double* __restrict__ var,
                                              const TIn* __restrict__ X, const TIn* __restrict__ box,
                                              double* __restrict__ mean) {
  int tile = blockIdx.x;
  const int tile_lin = tile;
  int ti = 0;
  {
    int rowlen = nt1;
    while (tile >= rowlen) {
      tile -= rowlen;
      --rowlen;
      ++ti;
    }
  }
  const int tj = ti + tile;
  const double* base = slabs + (int64_t)tile_lin * ksplit * (2 * PT * PT);
  double L[3] = {0, 0, 0}, iL[3] = {0, 0, 0};
  CellFrame<double> h = {};
  if (CELL == CELL_BOX && mean) box_lengths_wide(box, L, iL);  // frame 0's box
  if (CELL == CELL_TRI && mean) cell_frame(box, h);
  for (int e = threadIdx.x; e < PT * PT; e += 256) {
    const int i = ti * PT + e / PT, j = tj * PT + e % PT;
    if (i >= N || j >= N) continue;
    double a = 0.0, q = 0.0;
    for (int ks = 0; ks < ksplit; ++ks) {
      a += base[(int64_t)ks * (2 * PT * PT) + e];
      q += base[(int64_t)ks * (2 * PT * PT) + PT * PT + e];
    }
    const double m = a / (double)T;
    double v = __builtin_fma(-m, m, q / (double)T);
    if (v < 0.0) v = 0.0;
    if (i == j) v = 0.0;
    var[(int64_t)i * N + j] = v;
    var[(int64_t)j * N + i] = v;
    if (mean) {
      double dx = (double)X[(int64_t)j * 3 + 0] - (double)X[(int64_t)i * 3 + 0],
             dy = (double)X[(int64_t)j * 3 + 1] - (double)X[(int64_t)i * 3 + 1],
             dz = (double)X[(int64_t)j * 3 + 2] - (double)X[(int64_t)i * 3 + 2];
      pair_wrap<CELL>(dx, dy, dz, L, iL, h);
      // (from float64 coordinates the inner product here is ux ux and uy uy the fused one: the form this
      // instantiation has always had)
      const double mu = i == j ? 0.0 : (sizeof(TIn) == 8 ? pair_norm(dy, dx, dz) : pair_norm(dx, dy, dz)) + m;
      mean[(int64_t)i * N + j] = mu;
      mean[(int64_t)j * N + i] = mu;
    }
  }
}

template <typename TIn>
__global__ __launch_bounds__(256) void pair_var_kernel(const double* __restrict__ slabs, int32_t nt1,
                                                       int32_t ksplit, int32_t N, int64_t T,
                                                       double* __restrict__ var, const TIn* __restrict__ X,
                                                       double* __restrict__ mean) {
  pair_var_body<TIn, CELL_OPEN>(slabs, nt1, ksplit, N, T, var, X, nullptr, mean);
}

template <typename TIn>
__global__ __launch_bounds__(256) void pair_var_pbc_kernel(const double* __restrict__ slabs, int32_t nt1,
                                                           int32_t ksplit, int32_t N, int64_t T,
                                                           double* __restrict__ var, const TIn* __restrict__ X,
                                                           const TIn* __restrict__ box,
                                                           double* __restrict__ mean) {
  pair_var_body<TIn, CELL_BOX>(slabs, nt1, ksplit, N, T, var, X, box, mean);
}

template <typename TIn, int CELL>
__global__ __launch_bounds__(256) void pair_var_pbc_kernel(const double* __restrict__ slabs, int32_t nt1,
                                                           int32_t ksplit, int32_t N, int64_t T,
                                                           double* __restrict__ var, const TIn* __restrict__ X,
                                                           const TIn* __restrict__ cell, double* __restrict__ mean) {
  static_assert(CELL == CELL_TRI, "the triclinic form");
  pair_var_body<TIn, CELL>(slabs, nt1, ksplit, N, T, var, X, cell, mean);
}

// out = weight * (var_r + (mean_r - mean)^2): this rank's term of the pooled variance
__global__ __launch_bounds__(256) void pair_pool_kernel(const double* __restrict__ var_r, const double* __restrict__ mean_r,
                                                        const double* __restrict__ mean, double weight, int64_t n,
                                                        double* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const double d = mean_r[e] - mean[e];
    out[e] = weight * (var_r[e] + d * d);
  }
}

static void pair_plan(int64_t T, int32_t N, int* nt1, int* n_tiles, int* ksplit, int64_t* fps) {
  *nt1 = (int)ceil_div(N, PT);
  *n_tiles = *nt1 * (*nt1 + 1) / 2;
  int64_t k = ceil_div(2048, *n_tiles);
  const int64_t kmax_frames = ceil_div(T, PFB);
  if (k > kmax_frames) k = kmax_frames;
  const int64_t kmax_mem = (int64_t)(((size_t)1 << 31) / ((size_t)*n_tiles * 2 * PT * PT * 8));
  if (k > kmax_mem) k = kmax_mem;
  if (k < 1) k = 1;
  *ksplit = (int)k;
  *fps = round_up(ceil_div(T, k), PFB);
}

}  // namespace aggf

using namespace aggf;

extern "C" size_t aggf_pair_dist_var_workspace_bytes(int64_t T, int32_t N) {
  if (T <= 0 || N <= 0) return 0;
  int nt1, n_tiles, ksplit;
  int64_t fps;
  pair_plan(T, N, &nt1, &n_tiles, &ksplit, &fps);
  return (size_t)n_tiles * ksplit * 2 * PT * PT * sizeof(double) + 256;
}

// one dtype's two launches: box NULL, the open kernels with the arguments they have always had; else the box forms
template <typename TIn>
static int launch_pair_moments(dim3 grid, hipStream_t stream, const void* X, int64_t T, int32_t N, int nt1,
                               int n_tiles, int ksplit, int64_t fps, const void* box, int32_t bstride, double* slabs,
                               double* mean, double* var) {
  if (box && bstride == 9) {
    AGGF_LAUNCH((pair_stats_pbc_kernel<TIn, CELL_TRI>), grid, dim3(256), 0, stream, (const TIn*)X, T, N, nt1, n_tiles, fps,
                (const TIn*)box, slabs);
    AGGF_LAUNCH_OK();
    AGGF_LAUNCH((pair_var_pbc_kernel<TIn, CELL_TRI>), dim3(n_tiles), dim3(256), 0, stream, slabs, nt1, ksplit, N, T, var,
                (const TIn*)X, (const TIn*)box, mean);
  } else if (box) {
    AGGF_LAUNCH(pair_stats_pbc_kernel<TIn>, grid, dim3(256), 0, stream, (const TIn*)X, T, N, nt1, n_tiles, fps,
                (const TIn*)box, bstride, slabs);
    AGGF_LAUNCH_OK();
    AGGF_LAUNCH(pair_var_pbc_kernel<TIn>, dim3(n_tiles), dim3(256), 0, stream, slabs, nt1, ksplit, N, T, var,
                (const TIn*)X, (const TIn*)box, mean);
  } else {
    AGGF_LAUNCH(pair_stats_kernel<TIn>, grid, dim3(256), 0, stream, (const TIn*)X, T, N, nt1, n_tiles, fps, slabs);
    AGGF_LAUNCH_OK();
    AGGF_LAUNCH(pair_var_kernel<TIn>, dim3(n_tiles), dim3(256), 0, stream, slabs, nt1, ksplit, N, T, var,
                (const TIn*)X, mean);
  }
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

// K6, open (box NULL) or under a box: one plan, one workspace layout for both
static int pair_moments_impl(const void* X, int64_t T, int32_t N, int dtype, const void* box, int32_t bstride,
                             double* mean, double* var, void* ws, size_t ws_bytes, void* stream_v, const char* who) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!X || !var || !ws) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (T <= 0 || N <= 0) return fail(AGGF_ERR_ARG, "%s: empty problem", who);
  int nt1, n_tiles, ksplit;
  int64_t fps;
  pair_plan(T, N, &nt1, &n_tiles, &ksplit, &fps);
  if (ws_bytes < (size_t)n_tiles * ksplit * 2 * PT * PT * sizeof(double))
    return fail(AGGF_ERR_WORKSPACE, "%s: workspace too small", who);
  double* slabs = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)((int64_t)n_tiles * ksplit));
  if (dtype == AGGF_F64)
    return launch_pair_moments<double>(grid, stream, X, T, N, nt1, n_tiles, ksplit, fps, box, bstride, slabs, mean, var);
  if (dtype == AGGF_F32)
    return launch_pair_moments<float>(grid, stream, X, T, N, nt1, n_tiles, ksplit, fps, box, bstride, slabs, mean, var);
  return fail(AGGF_ERR_ARG, "%s: bad dtype", who);
}

// the box of a box form: (T, 3) or (3,) in the coordinates' dtype, or (T, 9): a triclinic cell per frame
static int pair_moments_box(const char* who, const void* box, int32_t box_stride) {
  if (!box) return fail(AGGF_ERR_ARG, "%s: NULL box", who);
  if (box_stride != 0 && box_stride != 3 && box_stride != 9)
    return fail(AGGF_ERR_ARG, "%s: box_stride %d is none of 0, 3 and 9", who, box_stride);
  return AGGF_OK;
}

extern "C" int aggf_pair_dist_var(const void* X, int64_t T, int32_t N, int dtype, double* var, void* ws,
                                  size_t ws_bytes, void* stream_v) {
  return pair_moments_impl(X, T, N, dtype, nullptr, 0, nullptr, var, ws, ws_bytes, stream_v, "aggf_pair_dist_var");
}

extern "C" int aggf_pair_dist_moments(const void* X, int64_t T, int32_t N, int dtype, double* mean, double* var,
                                      void* ws, size_t ws_bytes, void* stream_v) {
  if (!mean) return fail(AGGF_ERR_ARG, "aggf_pair_dist_moments: NULL pointer");
  return pair_moments_impl(X, T, N, dtype, nullptr, 0, mean, var, ws, ws_bytes, stream_v, "aggf_pair_dist_moments");
}

extern "C" int aggf_pair_dist_var_pbc(const void* X, int64_t T, int32_t N, int dtype, const void* box,
                                      int32_t box_stride, double* var, void* ws, size_t ws_bytes, void* stream_v) {
  const int rc = pair_moments_box("aggf_pair_dist_var_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  return pair_moments_impl(X, T, N, dtype, box, box_stride, nullptr, var, ws, ws_bytes, stream_v,
                           "aggf_pair_dist_var_pbc");
}

extern "C" int aggf_pair_dist_moments_pbc(const void* X, int64_t T, int32_t N, int dtype, const void* box,
                                          int32_t box_stride, double* mean, double* var, void* ws, size_t ws_bytes,
                                          void* stream_v) {
  const int rc = pair_moments_box("aggf_pair_dist_moments_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  if (!mean) return fail(AGGF_ERR_ARG, "aggf_pair_dist_moments_pbc: NULL pointer");
  return pair_moments_impl(X, T, N, dtype, box, box_stride, mean, var, ws, ws_bytes, stream_v,
                           "aggf_pair_dist_moments_pbc");
}

extern "C" int aggf_pair_pool_term(const double* var_r, const double* mean_r, const double* mean, double weight,
                                   int64_t n, double* out, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!var_r || !mean_r || !mean || !out) return fail(AGGF_ERR_ARG, "aggf_pair_pool_term: NULL pointer");
  if (n <= 0) return AGGF_OK;
  int64_t g = ceil_div(n, 256);
  if (g > 4096) g = 4096;
  AGGF_LAUNCH(pair_pool_kernel, dim3((unsigned)g), dim3(256), 0, stream, var_r, mean_r, mean, weight, n, out);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}
