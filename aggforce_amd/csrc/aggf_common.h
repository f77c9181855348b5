// Shared device/host helpers for libaggf (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>

#include "../../include/aggf.h"

namespace aggf {

// ---- error plumbing (thread-local last error string; see aggf_last_error) ----
void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);

#define AGGF_HIP_OK(expr)                                                         \
  do {                                                                            \
    hipError_t _e = (expr);                                                       \
    if (_e != hipSuccess)                                                         \
      return ::aggf::fail(AGGF_ERR_HIP, "%s failed: %s (%s:%d)", #expr,           \
                          hipGetErrorString(_e), __FILE__, __LINE__);             \
  } while (0)

#define AGGF_LAUNCH_OK()                                                          \
  do {                                                                            \
    hipError_t _e = hipGetLastError();                                            \
    if (_e != hipSuccess)                                                         \
      return ::aggf::fail(AGGF_ERR_HIP, "kernel launch failed: %s (%s:%d)",       \
                          hipGetErrorString(_e), __FILE__, __LINE__);             \
  } while (0)

// ---- launch coverage (aggf_coverage_dump): every kernel launch of the library goes through AGGF_LAUNCH, which counts
// the launch under the kernel's host handle -- the set of template instantiations a process actually executed, resolved
// to symbol names on request.  tests/test_gpu_zz_coverage.py compares it with the kernels the library contains.
void cover_hit(const void* kernel_handle);
#define AGGF_LAUNCH(kernel, ...)                                   \
  do {                                                             \
    ::aggf::cover_hit(reinterpret_cast<const void*>(kernel));      \
    hipLaunchKernelGGL(kernel, __VA_ARGS__);                       \
  } while (0)

// ---- adversarial dispatch order (TEST-ONLY build: `make order` -> build_order/libaggf_order.so, compiled with
// -DAGGF_ORDER_TEST; the shipped library contains none of this).  Launches that read and write one buffer from several
// workgroups (K2's step / panel / trailing / back-substitution products, the slab sums with `accumulate`, the triangle
// unpack, the pinned scatter: DESIGN.md section 5b lists them) are made through AGGF_LAUNCH_GATED; in the test build
// their workgroups then run STRICTLY ONE AFTER THE OTHER, in ascending (AGGF_ORDER=forward) or descending
// (AGGF_ORDER=reverse) block order: a result that depends on which workgroup runs first differs between the two
// orders and from the oracle -- deterministically, in one run, instead of once in a thousand.  A workgroup waits for
// its turn on a device counter (bounded spin: a grid larger than `limit` -- what is surely resident at once -- is
// not gated, a spin that runs out is counted and reported), the launch is followed by a synchronise + read-back of
// the time-outs.  aggf_order_note() (aggf_util.hip) keeps the process totals and prints them when the library unloads.
#ifdef AGGF_ORDER_TEST
struct OrderGate {
  unsigned int done, mode, timeouts, pad;
};
void order_note(int gated, int timeouts, const char* kernel);
int order_mode();  // 0 off, 1 forward, 2 reverse (AGGF_ORDER)
static __device__ OrderGate g_order_gate;  // one per translation unit (no relocatable device code)
static __global__ void order_arm_kernel(unsigned int mode) {
  g_order_gate.done = 0;
  g_order_gate.mode = mode;
  g_order_gate.timeouts = 0;
}
__device__ __forceinline__ void order_enter() {
  const unsigned mode = g_order_gate.mode;
  if (mode == 0) return;
  const unsigned nb = gridDim.x * gridDim.y * gridDim.z;
  const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const unsigned turn = mode == 1 ? lin : nb - 1 - lin;
  if (threadIdx.x == 0 && threadIdx.y == 0 && threadIdx.z == 0) {
    unsigned spins = 0;
    while (__hip_atomic_load(&g_order_gate.done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != turn) {
      __builtin_amdgcn_s_sleep(8);
      if (++spins > (1u << 20)) {  // ~0.25 s: never hang the GPU
        atomicAdd(&g_order_gate.timeouts, 1u);
        break;
      }
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
__device__ __forceinline__ void order_exit() {
  if (g_order_gate.mode == 0) return;
  __syncthreads();
  if (threadIdx.x == 0 && threadIdx.y == 0 && threadIdx.z == 0) {
    __threadfence();
    atomicAdd(&g_order_gate.done, 1u);
  }
}
static inline void order_arm(hipStream_t stream, dim3 grid, unsigned limit) {
  const uint64_t nb = (uint64_t)grid.x * grid.y * grid.z;
  const unsigned mode = nb <= limit ? (unsigned)order_mode() : 0u;
  hipLaunchKernelGGL(order_arm_kernel, dim3(1), dim3(1), 0, stream, mode);
}
static inline void order_collect(hipStream_t stream, dim3 grid, unsigned limit, const char* kernel) {
  const uint64_t nb = (uint64_t)grid.x * grid.y * grid.z;
  OrderGate g = {0, 0, 0, 0};
  if (order_mode() == 0) return;
  if (hipStreamSynchronize(stream) == hipSuccess) (void)hipMemcpyFromSymbol(&g, HIP_SYMBOL(g_order_gate), sizeof(g));
  order_note(nb <= limit ? 1 : 0, (int)g.timeouts, kernel);
}
// the kernel's body between the two macros runs as a lambda so that its early `return`s still reach the exit
#define AGGF_GATED_BODY_BEGIN ::aggf::order_enter(); [&]() {
#define AGGF_GATED_BODY_END }(); ::aggf::order_exit();
#define AGGF_LAUNCH_GATED(limit, kernel, grid, block, lds, stream, ...)      \
  do {                                                                       \
    const dim3 og_ = (grid);                                                 \
    ::aggf::order_arm(stream, og_, (limit));                                 \
    AGGF_LAUNCH(kernel, og_, block, lds, stream, __VA_ARGS__);               \
    ::aggf::order_collect(stream, og_, (limit), #kernel);                    \
  } while (0)
#else
#define AGGF_GATED_BODY_BEGIN
#define AGGF_GATED_BODY_END
#define AGGF_LAUNCH_GATED(limit, kernel, ...) AGGF_LAUNCH(kernel, __VA_ARGS__)
#endif

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
static inline int64_t ceil_div(int64_t x, int64_t m) { return (x + m - 1) / m; }
int device_cu_count();

// One flag per (call site, device): hipFuncSetAttribute applies to the CURRENT device only, so a
// process that drives several GPUs must repeat it on each of them.
struct PerDeviceOnce {
  bool done[64] = {};
  bool* flag() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    return &done[dev];
  }
};

typedef double __attribute__((ext_vector_type(4))) f64x4;
typedef float __attribute__((ext_vector_type(4))) f32x4;

// ---- MFMA 16x16x4 wrappers.  A: lane l holds A[i=l&15][k=l>>4]; B: B[k=l>>4][j=l&15].
//      C/D: col = l&15 for both; row = (l>>4)+4*r for f64, (l>>4)*4+r for f32
//      (cdna_hip_programming.md section 3, "Fragment layout").
template <typename T>
struct Mfma;

template <>
struct Mfma<double> {
  using acc_t = f64x4;
  __device__ static __forceinline__ acc_t mma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  __device__ static __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

template <>
struct Mfma<float> {
  using acc_t = f32x4;
  __device__ static __forceinline__ acc_t mma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  __device__ static __forceinline__ int row(int lane, int r) { return (lane >> 4) * 4 + r; }
};

template <typename T>
__device__ __forceinline__ typename Mfma<T>::acc_t acc_zero() {
  typename Mfma<T>::acc_t z = {0, 0, 0, 0};
  return z;
}

// 16-byte vector of T
template <typename T>
struct Vec16;
template <>
struct Vec16<double> {
  typedef double __attribute__((ext_vector_type(2))) type;
  static constexpr int N = 2;
};
template <>
struct Vec16<float> {
  typedef float __attribute__((ext_vector_type(4))) type;
  static constexpr int N = 4;
};

// ---- one element of a K9 pair array from the displacement d = X[t,j] - C[t,i] (and, in DOT mode, e = V[t,j] - Y[t,i]):
// the one expression of the matrix kernel (K9a) and the pair-list kernel (K9c), so that the two agree bit for bit.
// a0 b0 + a1 b1 + a2 b2 with its roundings written out: which products fuse into an FMA is otherwise the compiler's
// choice per kernel (it packs two float products of K9a into one v_pk_mul_f32, and fuses all three where it cannot),
// and two kernels that differ in it differ in the last bit.  These are the sequences K9a has had since it shipped.
__device__ __forceinline__ float pair_dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
#pragma clang fp contract(off)
  return __builtin_fmaf(a1, b1, a0 * b0) + a2 * b2;
}
__device__ __forceinline__ double pair_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
#pragma clang fp contract(off)
  return __builtin_fma(a2, b2, __builtin_fma(a0, b0, a1 * b1));
}
template <typename T, int MODE>
__device__ __forceinline__ T pair_element(T d0, T d1, T d2, T e0, T e1, T e2) {
  if (MODE == AGGF_PAIR_DOT) return pair_dot3(e0, d0, e1, d1, e2, d2);
  const T val = pair_dot3(d0, d0, d1, d1, d2, d2);
  return MODE == AGGF_PAIR_DIST ? sqrt(val) : val;
}

// ---- minimum image of one displacement component under an orthorhombic box of length L (invL = T(1) / L, formed once
// per frame and dimension by box_lengths): the one wrap of every box kernel (K9c / K9d box forms, K9e), its roundings
// written out for the reason pair_dot3's are.  k = rint(d invL), u = fma(-k, L, d).  rint rounds to nearest even (one
// v_rndne) and is odd, so min_image(-d) == -min_image(d) exactly; where |d| << L, k is 0 and u is d bit for bit.
__device__ __forceinline__ float min_image(float d, float L, float invL) {
#pragma clang fp contract(off)
  const float k = __builtin_rintf(d * invL);
  return __builtin_fmaf(-k, L, d);
}
__device__ __forceinline__ double min_image(double d, double L, double invL) {
#pragma clang fp contract(off)
  const double k = __builtin_rint(d * invL);
  return __builtin_fma(-k, L, d);
}
// The three lengths of one frame's box and their inverses.  A length that is not a positive finite number becomes NaN
// (and so does everything wrapped with it: the convention a bad pair index has, at no host synchronisation for a box
// that lives on the device); returns whether all three are good.
template <typename T>
__device__ __forceinline__ bool box_lengths(const T* __restrict__ box, T L[3], T invL[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const T l = box[k];
    const bool good = l > (T)0 && l < (T)__builtin_inf();
    L[k] = good ? l : (T)__builtin_nan("");
    invL[k] = (T)1 / L[k];
    ok = ok && good;
  }
  return ok;
}

// ---- triclinic cells.  A cell is three lattice vectors as rows a = (ax, 0, 0), b = (bx, by, 0), c = (cx, cy, cz) of a
// lower-triangular matrix (the GROMACS / MDTraj convention), ax, by, cz > 0.  The image of a displacement is obtained
// by BRICK REDUCTION, each line on the updated d, with min_image's roundings:
//   kc = rint(dz (1/cz));  dz = fma(-kc, cz, dz);  dy = fma(-kc, cy, dy);  dx = fma(-kc, cx, dx)
//   kb = rint(dy (1/by));  dy = fma(-kb, by, dy);  dx = fma(-kb, bx, dx)
//   ka = rint(dx (1/ax));  dx = fma(-ka, ax, dx)
// the unique lattice translate of d inside the brick |dx| <= ax/2, |dy| <= by/2, |dz| <= cz/2 -- the true minimum
// image wherever that is shorter than min(ax, by, cz) / 2, a periodic image that is never shorter than it beyond.
// With zero off-diagonal entries it is min_image component by component, bit for bit (fma(-k, 0, d) == d).
template <typename T>
struct CellFrame {
  T ax, bx, by, cx, cy, cz;  // the six lower-triangular entries
  T iax, iby, icz;           // 1 / ax, 1 / by, 1 / cz
};
__device__ __forceinline__ float cell_rint(float q) { return __builtin_rintf(q); }
__device__ __forceinline__ double cell_rint(double q) { return __builtin_rint(q); }
__device__ __forceinline__ float cell_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double cell_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
// One frame's cell from its row-major 3 x 3 matrix (nine values of TIn, of which the six lower-triangular ones are
// read), widened to T.  box_lengths' convention: a diagonal entry that is not positive and finite, or an off-diagonal
// one that is not finite, makes all nine numbers NaN (and with them everything of that frame); returns whether the
// cell is good.
template <typename TIn>
__device__ __forceinline__ bool cell_good(const TIn* __restrict__ m) {
  const TIn inf = (TIn)__builtin_inf();
  return m[0] > (TIn)0 && m[0] < inf && m[4] > (TIn)0 && m[4] < inf && m[8] > (TIn)0 && m[8] < inf &&
         __builtin_fabs(m[3]) < inf && __builtin_fabs(m[6]) < inf && __builtin_fabs(m[7]) < inf;
}
template <typename T, typename TIn>
__device__ __forceinline__ bool cell_frame(const TIn* __restrict__ m, CellFrame<T>& h) {
  const T ax = (T)m[0], bx = (T)m[3], by = (T)m[4], cx = (T)m[6], cy = (T)m[7], cz = (T)m[8];
  const bool ok = cell_good(m);
  const T nan = (T)__builtin_nan("");
  h.ax = ok ? ax : nan, h.bx = ok ? bx : nan, h.by = ok ? by : nan;
  h.cx = ok ? cx : nan, h.cy = ok ? cy : nan, h.cz = ok ? cz : nan;
  h.iax = (T)1 / h.ax, h.iby = (T)1 / h.by, h.icz = (T)1 / h.cz;
  return ok;
}
// brick reduction of (d0, d1, d2) in place
template <typename T>
__device__ __forceinline__ void brick_image(T& d0, T& d1, T& d2, const CellFrame<T>& h) {
#pragma clang fp contract(off)
  const T kc = cell_rint(d2 * h.icz);
  d2 = cell_fma(-kc, h.cz, d2), d1 = cell_fma(-kc, h.cy, d1), d0 = cell_fma(-kc, h.cx, d0);
  const T kb = cell_rint(d1 * h.iby);
  d1 = cell_fma(-kb, h.by, d1), d0 = cell_fma(-kb, h.bx, d0);
  const T ka = cell_rint(d0 * h.iax);
  d0 = cell_fma(-ka, h.ax, d0);
}
// ---- NEAREST IMAGE.  The brick image, then the shortest of its 27 translates d + i a + j b + k c, i, j, k in {-1, 0, 1},
// by squared length (cell_sq).  The candidates are visited in one fixed order: (0, 0, 0) -- the brick image itself --
// first, then k (of c) = -1, 0, 1 outermost, j (of b) inside it, i (of a) innermost, each from -1 to 1; a candidate
// replaces the best so far only if it is STRICTLY shorter, so a tie keeps the earlier one (the brick image before all)
// and the choice is a function of d alone.  A translate is formed like the brick image, c first:
//   x = fma(i, ax, fma(j, bx, fma(k, cx, d0)));  y = fma(j, by, fma(k, cy, d1));  z = fma(k, cz, d2)
// (a zero count leaves the component as it is).  For a REDUCED cell (|bx| <= ax/2, |cx| <= ax/2, |cy| <= by/2) the
// result is the true minimum image whenever that image is shorter than half the shortest of the 26 lattice vectors
// i a + j b + k c (pbc.Cell.image_radius); beyond that it is a periodic image that is never longer than the brick image.
// PRUNING: every lattice vector of a lower-triangular cell is at least min(ax, by, cz) long, so a brick image with
// |d|^2 <= min(ax, by, cz)^2 / 4 has no strictly shorter translate and the search is skipped: the same bits as the full
// search (a translate could round below the brick image only for a d that sits on a tie at exactly that length).
// A bad frame is NaN as in the brick form: every comparison with NaN is false, the NaN brick image stays.
__device__ __forceinline__ float cell_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double cell_min(double a, double b) { return __builtin_fmin(a, b); }
template <typename T>
__device__ __forceinline__ T cell_sq(T e0, T e1, T e2) {
#pragma clang fp contract(off)
  return cell_fma(e2, e2, cell_fma(e1, e1, e0 * e0));
}
// d + count * step for a count in {-1, 0, 1} that is a constant once the search is unrolled
template <typename T>
__device__ __forceinline__ T cell_step(int count, T step, T d) {
  return count == 0 ? d : cell_fma((T)count, step, d);
}
template <typename T>
__device__ __forceinline__ void nearest_image(T& d0, T& d1, T& d2, const CellFrame<T>& h) {
#pragma clang fp contract(off)
  brick_image(d0, d1, d2, h);
  const T m = cell_min(cell_min(h.ax, h.by), h.cz);
  T best = cell_sq(d0, d1, d2);
  if (best <= (T)0.25 * (m * m)) return;
  T b0 = d0, b1 = d1, b2 = d2;
#pragma unroll
  for (int k = -1; k <= 1; ++k) {
    const T z = cell_step(k, h.cz, d2), yk = cell_step(k, h.cy, d1), xk = cell_step(k, h.cx, d0);
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
      const T y = cell_step(j, h.by, yk), xj = cell_step(j, h.bx, xk);
#pragma unroll
      for (int i = -1; i <= 1; ++i) {
        if (i == 0 && j == 0 && k == 0) continue;
        const T x = cell_step(i, h.ax, xj);
        const T q = cell_sq(x, y, z);
        const bool shorter = q < best;
        best = shorter ? q : best, b0 = shorter ? x : b0, b1 = shorter ? y : b1, b2 = shorter ? z : b2;
      }
    }
  }
  d0 = b0, d1 = b1, d2 = b2;
}
// the form of a kernel body: no box, an orthorhombic box (min_image), a triclinic cell (brick_image), a triclinic cell
// with the nearest image (nearest_image; the same nine numbers per frame as CELL_TRI)
constexpr int CELL_OPEN = 0, CELL_BOX = 1, CELL_TRI = 2, CELL_NEAR = 3;
// the image of a displacement under a cell form that holds a CellFrame
template <int CELL, typename T>
__device__ __forceinline__ void cell_image(T& d0, T& d1, T& d2, const CellFrame<T>& h) {
  if (CELL == CELL_NEAR)
    nearest_image(d0, d1, d2, h);
  else
    brick_image(d0, d1, d2, h);
}

// ---- Philox4x32-10 (Salmon et al., SC'11): counter = 64-bit quad index, key = seed ----
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c[0];
    const uint64_t p1 = (uint64_t)M1 * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += W0; k1 += W1;
  }
}

// four standard normals for quad index q of stream `seed` (Box-Muller on 32-bit uniforms)
__device__ __forceinline__ void normal_quad(uint64_t seed, uint64_t stream, int64_t q, double z[4]) {
  uint32_t c[4] = {(uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const double u1 = ((double)c[2 * h] + 0.5) * (1.0 / 4294967296.0);
    const double u2 = ((double)c[2 * h + 1] + 0.5) * (1.0 / 4294967296.0);
    const double rad = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(6.283185307179586476925 * u2, &sn, &cs);
    z[2 * h] = rad * cs;
    z[2 * h + 1] = rad * sn;
  }
}

}  // namespace aggf
