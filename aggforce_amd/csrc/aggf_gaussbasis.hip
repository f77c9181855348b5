// K10: the clipped Gaussian radial basis of qp/jaxfeat.py and its derivatives of any order (aggforce_amd/_autograd.py:
// Basis, BasisDot).  With z = (r - c_k) / width and e_k = exp(-z^2), all arrays of one call in one dtype:
//
//   g_k^(0)(r) = max(e_k, clip) - clip
//   g_k^(q)(r) = (-1 / width)^q H_q(z) e_k  where e_k > clip, else 0        (q >= 1; H_q: physicists' Hermite polynomial,
//                                                                            H_{j+1} = 2 z H_j - 2 j H_{j-1}, q at run time)
//
//   gb_expand_kernel<T, SLOTTED>   out[e, col0(e) + k] = s[e] g_k^(q)(d[e])        the output written once, zeros included
//   gb_contract_kernel<T, FORM>    out[e] = sum_k H[., k] g_k^(q)(d[e])            H per element, per slotted row, per slot
//   gb_chansum_kernel<T>           part[chunk][slot, k] = sum_{t in chunk, a in slot} s[t,a] g_k^(q)(d[t,a])   (float64)
//   gb_chansum_reduce_kernel<T>    the frame chunks' partials added in ascending chunk order
//
// The centres are read from memory by a run-time loop (wave-uniform addresses): n_basis has no compiled-in cap.  Every
// sum has a fixed order and there are no atomics: results are bit-identical run to run.  Element offsets are 64-bit;
// base addresses need only element alignment.  A slot outside [0, n_slots) means "dropped": zeros.
#include "aggf_common.h"

namespace aggf {

// float: v_exp_f32 on x log2(e) (the argument is -z^2 <= 0; its rounding costs |x| 2^-24 relative, 4e-7 at the default
// clip).  double: the library routine -- never the float32 instruction.
__device__ __forceinline__ float gb_exp(float x) { return __expf(x); }
__device__ __forceinline__ double gb_exp(double x) { return exp(x); }

template <typename T>
struct BasisArgs {
  const T* cen;  // n_basis centres
  T inv_w, clip, qscale;  // 1 / width, clip (0: none), (-1 / width)^q
  int32_t nb, q;
};

template <typename T>
__device__ __forceinline__ T gb_value(T r, T c, const BasisArgs<T>& b) {
  const T z = (r - c) * b.inv_w;
  const T e = gb_exp(-z * z);
  if (b.q == 0) return (e < b.clip ? b.clip : e) - b.clip;  // (a NaN stays a NaN)
  T hm = 1, h = 2 * z;
  for (int j = 1; j < b.q; ++j) {
    const T hn = 2 * z * h - (T)(2 * j) * hm;
    hm = h, h = hn;
  }
  return e > b.clip ? b.qscale * h * e : (e != e ? e : (T)0);  // the tie e == clip: 0
}

// ---------------------------------------------------------------------------
// K10a.  One thread = GB_U elements of the flat output, 256 apart: a wave's store is 64 consecutive elements.  The
// (element, column) pair of a thread's first output costs one division; the following ones step by 256.
constexpr int GB_U = 8;

template <typename T, bool SLOTTED>
__global__ __launch_bounds__(256) void gb_expand_kernel(const T* __restrict__ d, const T* __restrict__ s,
                                                        const int32_t* __restrict__ slot, int64_t total, int32_t row,
                                                        int32_t n_sites, int32_t n_slots, BasisArgs<T> b,
                                                        T* __restrict__ out) {
  const int64_t chunk = 256 * GB_U;
  const int32_t step_e = 256 / row, step_c = 256 % row;
  const int32_t step_a = SLOTTED ? step_e % n_sites : 0;
  for (int64_t b0 = (int64_t)blockIdx.x * chunk; b0 < total; b0 += (int64_t)gridDim.x * chunk) {
    int64_t o = b0 + threadIdx.x;
    int64_t e = o / row;
    int32_t col = (int32_t)(o - e * row);
    int32_t a = SLOTTED ? (int32_t)(e % n_sites) : 0;
#pragma unroll
    for (int u = 0; u < GB_U; ++u) {
      if (o < total) {
        int32_t k = col;
        bool on = true;
        if (SLOTTED) {
          const int32_t sl = slot[a];
          on = (uint32_t)sl < (uint32_t)n_slots;
          k = on ? col - sl * b.nb : -1;
          on = on && k >= 0 && k < b.nb;
        }
        T val = 0;
        if (on) {
          val = gb_value(d[e], b.cen[k], b);
          if (s != nullptr) val *= s[e];
        }
        out[o] = val;
      }
      o += 256, col += step_c, e += step_e, a += step_a;
      if (col >= row) col -= row, ++e, ++a;
      if (SLOTTED && a >= n_sites) a -= n_sites;
    }
  }
}

// ---------------------------------------------------------------------------
// K10b.  One thread = one element: its n_basis coefficients are consecutive in memory (GB_H_ELEM: H (E, n_basis);
// GB_H_ROW: the element's block of a slotted row, H (E, n_slots n_basis); GB_H_SLOT: a row of the per-slot table
// H (n_slots, n_basis) shared by all frames).
template <typename T, int FORM>
__global__ __launch_bounds__(256) void gb_contract_kernel(const T* __restrict__ H, const T* __restrict__ d,
                                                          const int32_t* __restrict__ slot, int64_t E, int32_t n_sites,
                                                          int32_t n_slots, BasisArgs<T> b, T* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
    const T* h = H + e * b.nb;
    bool on = true;
    if (FORM != AGGF_GB_H_ELEM) {
      const int32_t sl = slot != nullptr ? slot[e % n_sites] : 0;
      on = (uint32_t)sl < (uint32_t)n_slots;
      const int64_t at = on ? (int64_t)sl * b.nb : 0;
      h = FORM == AGGF_GB_H_ROW ? H + e * ((int64_t)n_slots * b.nb) + at : H + at;
    }
    T acc = 0;
    if (on) {
      const T r = d[e];
      for (int32_t k = 0; k < b.nb; ++k) acc += h[k] * gb_value(r, b.cen[k], b);
    }
    out[e] = acc;
  }
}

// ---------------------------------------------------------------------------
// K10c.  One thread = one (slot, k) output of one chunk of frames (blockIdx.x: the chunk, blockIdx.y: 256 outputs): it
// walks the chunk's frames and the slot's sites (order[start[slot] .. start[slot + 1]), ascending) and sums in float64.
// No (T, N, n_slots n_basis) array exists.
template <typename T>
__global__ __launch_bounds__(256) void gb_chansum_kernel(const T* __restrict__ d, const T* __restrict__ s,
                                                         const int32_t* __restrict__ order,
                                                         const int32_t* __restrict__ start, int32_t n_order, int64_t nT,
                                                         int32_t N, int32_t n_slots, int64_t frames, BasisArgs<T> b,
                                                         double* __restrict__ part) {
  const int64_t P = (int64_t)n_slots * b.nb;
  const int64_t p = (int64_t)blockIdx.y * 256 + threadIdx.x;
  if (p >= P) return;
  const int32_t sl = (int32_t)(p / b.nb), k = (int32_t)(p - (int64_t)sl * b.nb);
  int32_t a0 = 0, a1 = N;
  if (start != nullptr) {
    a0 = start[sl], a1 = start[sl + 1];
    a0 = a0 < 0 ? 0 : a0;
    a1 = a1 > n_order ? n_order : a1;
  }
  const int64_t t0 = (int64_t)blockIdx.x * frames, t1 = t0 + frames < nT ? t0 + frames : nT;
  const T c = b.cen[k];
  double acc = 0.0;
  for (int64_t t = t0; t < t1; ++t)
    for (int32_t i = a0; i < a1; ++i) {
      const int32_t a = order != nullptr ? order[i] : i;
      if ((uint32_t)a >= (uint32_t)N) continue;
      T v = gb_value(d[t * N + a], c, b);
      if (s != nullptr) v *= s[t * N + a];
      acc += (double)v;
    }
  part[(int64_t)blockIdx.x * P + p] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void gb_chansum_reduce_kernel(const double* __restrict__ part, int64_t chunks,
                                                                int64_t P, T* __restrict__ out) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    double acc = 0.0;
    for (int64_t c = 0; c < chunks; ++c) acc += part[c * P + p];
    out[p] = (T)acc;
  }
}

// ---------------------------------------------------------------------------
static inline dim3 gb_grid(int64_t blocks) {
  if (blocks > 262144) blocks = 262144;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

template <typename T>
static BasisArgs<T> basis_args(const void* centers, int32_t n_basis, double width, double clip, int32_t q) {
  BasisArgs<T> b;
  b.cen = (const T*)centers;
  b.inv_w = (T)(1.0 / width);
  b.clip = (T)clip;
  double qs = 1.0;
  for (int j = 0; j < q; ++j) qs *= -1.0 / width;
  b.qscale = (T)qs;
  b.nb = n_basis, b.q = q;
  return b;
}

constexpr int32_t GB_MAX_Q = 64;

static int basis_check(const char* who, const void* centers, int32_t n_basis, double width, double clip, int32_t q,
                       int dtype) {
  if (dtype != AGGF_F32 && dtype != AGGF_F64) return fail(AGGF_ERR_ARG, "%s: bad dtype", who);
  if (n_basis < 1) return fail(AGGF_ERR_ARG, "%s: n_basis must be positive", who);
  if (!(width > 0.0) || !(width < 1e300)) return fail(AGGF_ERR_ARG, "%s: width must be positive and finite", who);
  if (!(clip >= 0.0) || !(clip < 1e300)) return fail(AGGF_ERR_ARG, "%s: clip must be non-negative and finite", who);
  if (q < 0 || q > GB_MAX_Q) return fail(AGGF_ERR_ARG, "%s: derivative order outside 0..%d", who, GB_MAX_Q);
  if (!centers) return fail(AGGF_ERR_ARG, "%s: NULL centres", who);
  return AGGF_OK;
}

// E rows of `row` values as an element count that fits a 64-bit byte offset
static bool gb_count(int64_t E, int64_t row, int64_t* total) {
  return !__builtin_mul_overflow(E, row, total) && *total <= INT64_MAX / 8;
}

// frame chunks of the channel sum: at most GB_MAX_CHUNKS, and partials of at most GB_PART_BYTES
constexpr int64_t GB_MAX_CHUNKS = 512;
constexpr int64_t GB_PART_BYTES = (int64_t)8 << 20;
static int64_t chansum_chunks(int64_t T, int64_t P) {
  int64_t chunks = GB_PART_BYTES / (P * (int64_t)sizeof(double));
  if (chunks > GB_MAX_CHUNKS) chunks = GB_MAX_CHUNKS;
  if (chunks > T) chunks = T;
  return chunks < 1 ? 1 : chunks;
}
static bool chansum_shape(int64_t T, int32_t n_slots, int32_t n_basis, int64_t* P) {
  if (T < 0 || n_slots < 1 || n_basis < 1) return false;
  *P = (int64_t)n_slots * n_basis;
  return *P <= (int64_t)65535 * 256;  // (grid.y)
}

}  // namespace aggf

using namespace aggf;

extern "C" int aggf_gbasis_expand(const void* d, const void* s, const void* centers, const int32_t* slot, int64_t E,
                                  int32_t n_basis, int32_t n_sites, int32_t n_slots, double width, double clip,
                                  int32_t q, int dtype, void* out, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const int rc = basis_check("aggf_gbasis_expand", centers, n_basis, width, clip, q, dtype);
  if (rc != AGGF_OK) return rc;
  if (E < 0) return fail(AGGF_ERR_ARG, "aggf_gbasis_expand: negative element count");
  int64_t row = n_basis, total = 0;
  if (slot) {
    if (n_sites < 1 || n_slots < 1) return fail(AGGF_ERR_ARG, "aggf_gbasis_expand: slots need n_sites, n_slots >= 1");
    if (E % n_sites) return fail(AGGF_ERR_ARG, "aggf_gbasis_expand: E is not a multiple of n_sites");
    row = (int64_t)n_slots * n_basis;
  }
  if (row > INT32_MAX - 256) return fail(AGGF_ERR_ARG, "aggf_gbasis_expand: row of %lld values", (long long)row);
  if (!gb_count(E, row, &total)) return fail(AGGF_ERR_ARG, "aggf_gbasis_expand: output does not fit a 64-bit byte offset");
  if (total == 0) return AGGF_OK;
  if (!d || !out) return fail(AGGF_ERR_ARG, "aggf_gbasis_expand: NULL pointer");
  const dim3 grid = gb_grid(ceil_div(total, 256 * GB_U)), block(256);
  if (dtype == AGGF_F32) {
    const BasisArgs<float> b = basis_args<float>(centers, n_basis, width, clip, q);
    if (slot)
      AGGF_LAUNCH((gb_expand_kernel<float, true>), grid, block, 0, stream, (const float*)d, (const float*)s, slot, total,
                  (int32_t)row, n_sites, n_slots, b, (float*)out);
    else
      AGGF_LAUNCH((gb_expand_kernel<float, false>), grid, block, 0, stream, (const float*)d, (const float*)s, slot,
                  total, (int32_t)row, 1, 1, b, (float*)out);
  } else {
    const BasisArgs<double> b = basis_args<double>(centers, n_basis, width, clip, q);
    if (slot)
      AGGF_LAUNCH((gb_expand_kernel<double, true>), grid, block, 0, stream, (const double*)d, (const double*)s, slot,
                  total, (int32_t)row, n_sites, n_slots, b, (double*)out);
    else
      AGGF_LAUNCH((gb_expand_kernel<double, false>), grid, block, 0, stream, (const double*)d, (const double*)s, slot,
                  total, (int32_t)row, 1, 1, b, (double*)out);
  }
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

template <typename T>
static void launch_contract(int form, dim3 grid, hipStream_t stream, const void* H, const void* d, const int32_t* slot,
                            int64_t E, int32_t n_sites, int32_t n_slots, const BasisArgs<T>& b, void* out) {
  const dim3 block(256);
  if (form == AGGF_GB_H_ELEM)
    AGGF_LAUNCH((gb_contract_kernel<T, AGGF_GB_H_ELEM>), grid, block, 0, stream, (const T*)H, (const T*)d, slot, E,
                n_sites, n_slots, b, (T*)out);
  else if (form == AGGF_GB_H_ROW)
    AGGF_LAUNCH((gb_contract_kernel<T, AGGF_GB_H_ROW>), grid, block, 0, stream, (const T*)H, (const T*)d, slot, E,
                n_sites, n_slots, b, (T*)out);
  else
    AGGF_LAUNCH((gb_contract_kernel<T, AGGF_GB_H_SLOT>), grid, block, 0, stream, (const T*)H, (const T*)d, slot, E,
                n_sites, n_slots, b, (T*)out);
}

extern "C" int aggf_gbasis_contract(const void* H, int form, const void* d, const void* centers, const int32_t* slot,
                                    int64_t E, int32_t n_basis, int32_t n_sites, int32_t n_slots, double width,
                                    double clip, int32_t q, int dtype, void* out, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const int rc = basis_check("aggf_gbasis_contract", centers, n_basis, width, clip, q, dtype);
  if (rc != AGGF_OK) return rc;
  if (form != AGGF_GB_H_ELEM && form != AGGF_GB_H_ROW && form != AGGF_GB_H_SLOT)
    return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: bad form");
  if (E < 0) return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: negative element count");
  int64_t row = n_basis, total = 0;
  if (form == AGGF_GB_H_ELEM) {
    n_sites = n_slots = 1, slot = nullptr;
  } else {
    if (n_sites < 1 || n_slots < 1) return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: slots need n_sites, n_slots >= 1");
    if (form == AGGF_GB_H_ROW && !slot) return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: the row form needs a slot table");
    if (!slot && n_slots != 1) return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: no slot table means one slot");
    if (E % n_sites) return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: E is not a multiple of n_sites");
    row = (int64_t)n_slots * n_basis;
    if (row > INT32_MAX - 256) return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: row of %lld values", (long long)row);
  }
  if (!gb_count(E, form == AGGF_GB_H_SLOT ? 1 : row, &total))
    return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: H does not fit a 64-bit byte offset");
  if (E == 0) return AGGF_OK;
  if (!H || !d || !out) return fail(AGGF_ERR_ARG, "aggf_gbasis_contract: NULL pointer");
  const dim3 grid = gb_grid(ceil_div(E, 256));
  if (dtype == AGGF_F32)
    launch_contract<float>(form, grid, stream, H, d, slot, E, n_sites, n_slots,
                           basis_args<float>(centers, n_basis, width, clip, q), out);
  else
    launch_contract<double>(form, grid, stream, H, d, slot, E, n_sites, n_slots,
                            basis_args<double>(centers, n_basis, width, clip, q), out);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

extern "C" size_t aggf_gbasis_sum_workspace_bytes(int64_t T, int32_t n_slots, int32_t n_basis) {
  int64_t P = 0;
  if (!chansum_shape(T, n_slots, n_basis, &P) || T == 0) return 0;
  return (size_t)round_up(chansum_chunks(T, P) * P * (int64_t)sizeof(double), 256);
}

extern "C" int aggf_gbasis_sum(const void* d, const void* s, const void* centers, const int32_t* order,
                               const int32_t* start, int32_t n_order, int64_t T, int32_t N, int32_t n_slots,
                               int32_t n_basis, double width, double clip, int32_t q, int dtype, void* out, void* ws,
                               size_t ws_bytes, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  const int rc = basis_check("aggf_gbasis_sum", centers, n_basis, width, clip, q, dtype);
  if (rc != AGGF_OK) return rc;
  int64_t P = 0, count = 0;
  if (N < 0 || !chansum_shape(T, n_slots, n_basis, &P)) return fail(AGGF_ERR_ARG, "aggf_gbasis_sum: bad shape");
  if (!gb_count(T, N, &count)) return fail(AGGF_ERR_ARG, "aggf_gbasis_sum: T N does not fit a 64-bit byte offset");
  if ((order == nullptr) != (start == nullptr) || (!order && n_slots != 1))
    return fail(AGGF_ERR_ARG, "aggf_gbasis_sum: order and start come together; without them there is one slot");
  if (order && (n_order < 0 || n_order > N)) return fail(AGGF_ERR_ARG, "aggf_gbasis_sum: n_order outside 0..N");
  if (!out) return fail(AGGF_ERR_ARG, "aggf_gbasis_sum: NULL output");
  const dim3 block(256), rgrid = gb_grid(ceil_div(P, 256));
  const int64_t chunks = count == 0 ? 0 : chansum_chunks(T, P);
  if (chunks > 0) {
    if (!d) return fail(AGGF_ERR_ARG, "aggf_gbasis_sum: NULL pointer");
    const size_t need = (size_t)round_up(chunks * P * (int64_t)sizeof(double), 256);
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 7)) return fail(AGGF_ERR_WORKSPACE, "aggf_gbasis_sum: workspace too small");
    const int64_t frames = ceil_div(T, chunks);
    const dim3 grid((unsigned)ceil_div(T, frames), (unsigned)ceil_div(P, 256));
    if (dtype == AGGF_F32)
      AGGF_LAUNCH((gb_chansum_kernel<float>), grid, block, 0, stream, (const float*)d, (const float*)s, order, start,
                  n_order, T, N, n_slots, frames, basis_args<float>(centers, n_basis, width, clip, q), (double*)ws);
    else
      AGGF_LAUNCH((gb_chansum_kernel<double>), grid, block, 0, stream, (const double*)d, (const double*)s, order, start,
                  n_order, T, N, n_slots, frames, basis_args<double>(centers, n_basis, width, clip, q), (double*)ws);
    AGGF_LAUNCH_OK();
    // (the reduce reads exactly the chunks the grid wrote)
    const int64_t written = ceil_div(T, frames);
    if (dtype == AGGF_F32)
      AGGF_LAUNCH((gb_chansum_reduce_kernel<float>), rgrid, block, 0, stream, (const double*)ws, written, P, (float*)out);
    else
      AGGF_LAUNCH((gb_chansum_reduce_kernel<double>), rgrid, block, 0, stream, (const double*)ws, written, P, (double*)out);
  } else {  // an empty sum: zeros (the reduce over no chunks)
    if (dtype == AGGF_F32)
      AGGF_LAUNCH((gb_chansum_reduce_kernel<float>), rgrid, block, 0, stream, (const double*)nullptr, (int64_t)0, P, (float*)out);
    else
      AGGF_LAUNCH((gb_chansum_reduce_kernel<double>), rgrid, block, 0, stream, (const double*)nullptr, (int64_t)0, P, (double*)out);
  }
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}
