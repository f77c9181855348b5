// K9c / K9d: pair distances over a static list of P pairs (i_p, j_p) shared by all frames
// (aggforce_amd/_autograd.py: PairListDist, PairListPull, PairListDot; jaxutil.pair_distances, and the upper triangles
// of jaxutil.distances, whose list is triu_indices).  With u[t,p] = X[t,j_p] - C[t,i_p] (X (T, n, 3), C (T, m, 3)):
//
//   pairlist_kernel<T, MODE>        out[t,p] = sqrt(u.u) | u.u | (V[t,j_p] - Y[t,i_p]).u   the (T, P) array written once
//   pairlist_pull_kernel<.., FORM>  S[t,s,:] = sum_{p incident to s} w[t,p] (Own[t,s] - Oth[t,o_p]): with the table by j
//                                   (Own = X, Oth = C) that is A[t,j,:] = sum w u, with the table by i (Own = C,
//                                   Oth = X) it is B[t,i,:] = -sum w u (-(a - b) is b - a exactly); w = W or
//                                   (Dv > 0 ? W / Dv : 0)
//   pairlist_pbc_kernel, pairlist_pull_pbc_kernel: the same two with u replaced by its minimum image under an
//                                   orthorhombic box per frame (min_image, aggf_common.h).  Each pair of kernels shares
//                                   one __device__ body; the open ones keep their names, arguments and bits.
//
// The arrays of a call are T P elements where K9a / K9b move T m n.  No atomics: a site's sum walks its entries of the
// incidence table (CSR: ptr, pair index, ascending pair index), so results are bit-identical run to run.  Element
// offsets are 64-bit; base addresses need only element alignment.  Every index read from a table is tested against the
// size of the array it addresses, so that no list a caller of the C ABI passes can make a kernel read outside X, C, W
// or the tables: a pair with a bad site writes NaN (K9c) or adds nothing (K9d).
#include "aggf_common.h"

namespace aggf {

// ---------------------------------------------------------------------------
// K9c.  One wave = 64 consecutive pairs x a block of `frames` frames: a lane loads its pair's two indices once and
// walks the frames, so a wave's store is 64 consecutive elements of a row of out whatever P is.  The two sites of an
// element are gathered from the frame's rows of X and C (3 n and 3 m values: cache-resident).  Waves take the
// (frame block, pair block) tasks in output order; `frames` is the launcher's choice (all frames unless that leaves
// too few tasks).
constexpr int PL_MIN_FRAMES = 8;
constexpr int64_t PL_TARGET_TASKS = 16384;

//
// PBC: u is wrapped to its minimum image under the frame's box (min_image; `box` (T, 3) with bstride 3, or (3,) with
// bstride 0: a frame's three lengths are wave-uniform and read once per frame, once per task for a constant box).  The
// tangent operands V - Y of DOT are never wrapped: the wrap is locally constant in X and C.
template <typename T, int MODE, int CELL>
__device__ __forceinline__ void pairlist_body(const T* __restrict__ X, const T* __restrict__ C,
                                              const T* __restrict__ V, const T* __restrict__ Y,
                                              const int32_t* __restrict__ pairs, int64_t nT, int32_t m, int32_t n,
                                              int64_t P, int64_t frames, const T* __restrict__ box, int32_t bstride,
                                              T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t pblocks = (P + 63) / 64, fblocks = (nT + frames - 1) / frames;
  const int64_t ntask = pblocks * fblocks;
  for (int64_t task = (int64_t)blockIdx.x * 4 + wave; task < ntask; task += (int64_t)gridDim.x * 4) {
    const int64_t fb = task / pblocks, pb = task - fb * pblocks;
    const int64_t p = pb * 64 + lane;
    if (p >= P) continue;
    const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
    const int64_t t0 = fb * frames, t1 = t0 + frames < nT ? t0 + frames : nT;
    T* o = out + t0 * P + p;
    if (!((uint32_t)i < (uint32_t)m && (uint32_t)j < (uint32_t)n)) {
      for (int64_t t = t0; t < t1; ++t, o += P) *o = (T)__builtin_nan("");
      continue;
    }
    const int64_t xs = 3 * (int64_t)n, cs = 3 * (int64_t)m;
    const int64_t xo = t0 * xs + 3 * (int64_t)j, co = t0 * cs + 3 * (int64_t)i;
    const T* x = X + xo;
    const T* c = C + co;
    const T* v = MODE == AGGF_PAIR_DOT ? V + xo : nullptr;
    const T* y = MODE == AGGF_PAIR_DOT ? Y + co : nullptr;
    T L[3] = {0, 0, 0}, iL[3] = {0, 0, 0};
    CellFrame<T> h = {};
    if (CELL == CELL_BOX && bstride == 0) box_lengths(box, L, iL);
#pragma unroll 4
    for (int64_t t = t0; t < t1; ++t, x += xs, c += cs, o += P) {
      T d0 = x[0] - c[0], d1 = x[1] - c[1], d2 = x[2] - c[2];
      if (CELL == CELL_BOX) {
        if (bstride != 0) box_lengths(box + t * bstride, L, iL);
        d0 = min_image(d0, L[0], iL[0]), d1 = min_image(d1, L[1], iL[1]), d2 = min_image(d2, L[2], iL[2]);
      }
      if (CELL == CELL_TRI || CELL == CELL_NEAR) {
        cell_frame(box + t * 9, h);
        cell_image<CELL>(d0, d1, d2, h);
      }
      T e0 = 0, e1 = 0, e2 = 0;
      if (MODE == AGGF_PAIR_DOT) {
        e0 = v[0] - y[0], e1 = v[1] - y[1], e2 = v[2] - y[2];
        v += xs, y += cs;
      }
      *o = pair_element<T, MODE>(d0, d1, d2, e0, e1, e2);
    }
  }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void pairlist_kernel(const T* __restrict__ X, const T* __restrict__ C,
                                                       const T* __restrict__ V, const T* __restrict__ Y,
                                                       const int32_t* __restrict__ pairs, int64_t nT, int32_t m,
                                                       int32_t n, int64_t P, int64_t frames, T* __restrict__ out) {
  pairlist_body<T, MODE, CELL_OPEN>(X, C, V, Y, pairs, nT, m, n, P, frames, nullptr, 0, out);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void pairlist_pbc_kernel(const T* __restrict__ X, const T* __restrict__ C,
                                                           const T* __restrict__ V, const T* __restrict__ Y,
                                                           const int32_t* __restrict__ pairs, int64_t nT, int32_t m,
                                                           int32_t n, int64_t P, int64_t frames,
                                                           const T* __restrict__ box, int32_t bstride,
                                                           T* __restrict__ out) {
  pairlist_body<T, MODE, CELL_BOX>(X, C, V, Y, pairs, nT, m, n, P, frames, box, bstride, out);
}

// The triclinic forms, an overload with a third template argument: cell is (T, 9), a row-major 3 x 3 cell per frame, and
// u its brick image (CELL_TRI) or its nearest image (CELL_NEAR; brick_image, nearest_image: aggf_common.h).
// pairlist_pbc_kernel<T, MODE> is the box form.
template <typename T, int MODE, int CELL>
__global__ __launch_bounds__(256) void pairlist_pbc_kernel(const T* __restrict__ X, const T* __restrict__ C,
                                                           const T* __restrict__ V, const T* __restrict__ Y,
                                                           const int32_t* __restrict__ pairs, int64_t nT, int32_t m,
                                                           int32_t n, int64_t P, int64_t frames,
                                                           const T* __restrict__ cell, T* __restrict__ out) {
  static_assert(CELL == CELL_TRI || CELL == CELL_NEAR, "a triclinic form");
  pairlist_body<T, MODE, CELL>(X, C, V, Y, pairs, nT, m, n, P, frames, cell, 9, out);
}

// ---------------------------------------------------------------------------
// K9d.  One launch per output: the sums of the sites of one incidence table.  Entry e of site s is the pair p = idx[e],
// ptr[s] <= e < ptr[s + 1], and the pair's other site is column `ocol` of `pairs`.  Every term is formed in the input
// dtype (as K9b forms it) and every sum is accumulated in float64 throughout, then narrowed once.
//   FORM 0, a lane per (frame, site): the lane walks its entries in ascending pair index.  Bonded lists, a few entries
//           per site; consecutive lanes are consecutive sites of one frame.
//   FORM 1, a wave per (frame, site): lane l takes entries l, l + 64, ... in ascending order, a fixed xor butterfly
//           adds the 64 lane sums.  The triangle, where a site has n - 1 entries, and any list with a long run.
// A site without entries gets zeros.  The launcher takes FORM 1 when the table's longest run exceeds PLP_LANE_DEG.
// PLP_LANE_DEG = 32 is NOT MEASURED yet: it is half a wave's lanes, the run at which a wave per site keeps at least
// half its lanes busy.  `tools/distgrad_bench.py --pairlist` times both forms on lists of 2 .. 128 entries per site
// (its form_sweep rows); the crossing it finds belongs here with the figure.
constexpr int PLP_LANE = 0, PLP_WAVE = 1;
constexpr int32_t PLP_LANE_DEG = 32;

template <typename TI, bool HAS_DV>
__device__ __forceinline__ TI pull_weight(const TI* __restrict__ W, const TI* __restrict__ Dv, int64_t e) {
  TI wv = W[e];
  if (HAS_DV) {
    const TI dv = Dv[e];
    const TI qv = wv / dv;  // (formed before the choice, as in K9b)
    wv = dv > (TI)0 ? qv : (TI)0;
  }
  return wv;
}

// PBC: Own - Oth is wrapped to its minimum image under the frame's box, as in K9c (min_image is odd, so B is still
// exactly the sum of -w u); a frame whose box is bad gets NaN sums, sites without entries included.
template <typename TI, typename TO, bool HAS_DV, int FORM, int CELL>
__device__ __forceinline__ void pairlist_pull_body(const TI* __restrict__ W, const TI* __restrict__ Dv,
                                                   const TI* __restrict__ Own, const TI* __restrict__ Oth,
                                                   const int32_t* __restrict__ pairs, int32_t ocol,
                                                   const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                   int64_t nT, int32_t ns, int32_t no, int64_t P,
                                                   const TI* __restrict__ box, int32_t bstride,
                                                   TO* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t ntask = nT * ns;
  const int64_t first = FORM == PLP_LANE ? (int64_t)blockIdx.x * 256 + threadIdx.x
                                         : (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t step = (int64_t)gridDim.x * (FORM == PLP_LANE ? 256 : 4);
  for (int64_t task = first; task < ntask; task += step) {
    const int64_t t = task / ns, s = task - t * ns;
    const TI* own = Own + task * 3;
    const TI o0 = own[0], o1 = own[1], o2 = own[2];
    const TI* oth = Oth + t * no * 3;
    const TI* w = W + t * P;
    const TI* dv = HAS_DV ? Dv + t * P : nullptr;
    int64_t beg = ptr[s], end = ptr[s + 1];  // (a run is clipped to the P entries the table has)
    beg = beg < 0 ? 0 : beg;
    end = end > P ? P : end;
    TI L[3] = {0, 0, 0}, iL[3] = {0, 0, 0};
    CellFrame<TI> h = {};
    const bool box_ok = CELL == CELL_BOX   ? box_lengths(box + t * bstride, L, iL)
                        : CELL == CELL_TRI || CELL == CELL_NEAR ? cell_frame(box + t * 9, h)
                                                                : true;
    const double zero = box_ok ? 0.0 : __builtin_nan("");
    double a0 = zero, a1 = zero, a2 = zero;
    for (int64_t e = FORM == PLP_LANE ? beg : beg + lane; e < end; e += FORM == PLP_LANE ? 1 : 64) {
      const int32_t p = idx[e];
      if (!((uint32_t)p < (uint64_t)P)) continue;
      const int32_t o = pairs[2 * (int64_t)p + ocol];
      if (!((uint32_t)o < (uint32_t)no)) continue;
      const TI wv = pull_weight<TI, HAS_DV>(w, dv, p);
      const TI* r = oth + 3 * (int64_t)o;
      TI u0 = o0 - r[0], u1 = o1 - r[1], u2 = o2 - r[2];
      if (CELL == CELL_BOX) u0 = min_image(u0, L[0], iL[0]), u1 = min_image(u1, L[1], iL[1]), u2 = min_image(u2, L[2], iL[2]);
      if (CELL == CELL_TRI || CELL == CELL_NEAR) cell_image<CELL>(u0, u1, u2, h);
      a0 += (double)(wv * u0), a1 += (double)(wv * u1), a2 += (double)(wv * u2);
    }
    if (FORM == PLP_WAVE) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        a0 += __shfl_xor(a0, d, 64), a1 += __shfl_xor(a1, d, 64), a2 += __shfl_xor(a2, d, 64);
      }
    }
    if (FORM == PLP_LANE || lane == 0) {
      TO* dst = out + task * 3;
      dst[0] = (TO)a0, dst[1] = (TO)a1, dst[2] = (TO)a2;
    }
  }
}

template <typename TI, typename TO, bool HAS_DV, int FORM>
__global__ __launch_bounds__(256) void pairlist_pull_kernel(const TI* __restrict__ W, const TI* __restrict__ Dv,
                                                            const TI* __restrict__ Own, const TI* __restrict__ Oth,
                                                            const int32_t* __restrict__ pairs, int32_t ocol,
                                                            const int32_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ idx, int64_t nT, int32_t ns,
                                                            int32_t no, int64_t P, TO* __restrict__ out) {
  pairlist_pull_body<TI, TO, HAS_DV, FORM, CELL_OPEN>(W, Dv, Own, Oth, pairs, ocol, ptr, idx, nT, ns, no, P, nullptr, 0, out);
}

template <typename TI, typename TO, bool HAS_DV, int FORM>
__global__ __launch_bounds__(256) void pairlist_pull_pbc_kernel(const TI* __restrict__ W, const TI* __restrict__ Dv,
                                                                const TI* __restrict__ Own, const TI* __restrict__ Oth,
                                                                const int32_t* __restrict__ pairs, int32_t ocol,
                                                                const int32_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ idx, int64_t nT, int32_t ns,
                                                                int32_t no, int64_t P, const TI* __restrict__ box,
                                                                int32_t bstride, TO* __restrict__ out) {
  pairlist_pull_body<TI, TO, HAS_DV, FORM, CELL_BOX>(W, Dv, Own, Oth, pairs, ocol, ptr, idx, nT, ns, no, P, box, bstride, out);
}

// (the triclinic forms: an overload with a fifth template argument, as pairlist_pbc_kernel's)
template <typename TI, typename TO, bool HAS_DV, int FORM, int CELL>
__global__ __launch_bounds__(256) void pairlist_pull_pbc_kernel(const TI* __restrict__ W, const TI* __restrict__ Dv,
                                                                const TI* __restrict__ Own, const TI* __restrict__ Oth,
                                                                const int32_t* __restrict__ pairs, int32_t ocol,
                                                                const int32_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ idx, int64_t nT, int32_t ns,
                                                                int32_t no, int64_t P, const TI* __restrict__ cell,
                                                                TO* __restrict__ out) {
  static_assert(CELL == CELL_TRI || CELL == CELL_NEAR, "a triclinic form");
  pairlist_pull_body<TI, TO, HAS_DV, FORM, CELL>(W, Dv, Own, Oth, pairs, ocol, ptr, idx, nT, ns, no, P, cell, 9, out);
}

static inline dim3 pairlist_grid(int64_t blocks) {
  if (blocks > 65536) blocks = 65536;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

// the sizes of one call: T P and 3 T max(m, n) as element counts that fit a 64-bit byte offset, P within int32
static int pairlist_shape(const char* who, int64_t T, int32_t m, int32_t n, int64_t P, int64_t* count) {
  if (T < 0 || m < 0 || n < 0 || P < 0) return fail(AGGF_ERR_ARG, "%s: negative shape", who);
  if (P > INT32_MAX) return fail(AGGF_ERR_ARG, "%s: more than 2^31 - 1 pairs", who);
  int64_t sites = 0;
  if (__builtin_mul_overflow(T, P, count) || *count > INT64_MAX / 8)
    return fail(AGGF_ERR_ARG, "%s: T P does not fit a 64-bit byte offset", who);
  if (__builtin_mul_overflow(T, 3 * (int64_t)(m > n ? m : n), &sites) || sites > INT64_MAX / 8)
    return fail(AGGF_ERR_ARG, "%s: T n does not fit a 64-bit byte offset", who);
  return AGGF_OK;
}

// (box NULL: the open kernels, with the arguments they have always had; near: the nearest-image form of a (T, 9) cell)
template <typename T>
static void launch_pairlist(int mode, dim3 grid, hipStream_t stream, const void* X, const void* C, const void* V,
                            const void* Y, const int32_t* pairs, int64_t nT, int32_t m, int32_t n, int64_t P,
                            int64_t frames, const void* box, int32_t bstride, bool near, void* out) {
  const dim3 block(256);
#define AGGF_PL_CELL(MODE, CELL)                                                                                \
  AGGF_LAUNCH((pairlist_pbc_kernel<T, MODE, CELL>), grid, block, 0, stream, (const T*)X, (const T*)C, (const T*)V,   \
              (const T*)Y, pairs, nT, m, n, P, frames, (const T*)box, (T*)out)
  if (box && bstride == 9 && near) {
    if (mode == AGGF_PAIR_DIST)
      AGGF_PL_CELL(AGGF_PAIR_DIST, CELL_NEAR);
    else if (mode == AGGF_PAIR_SQDIST)
      AGGF_PL_CELL(AGGF_PAIR_SQDIST, CELL_NEAR);
    else
      AGGF_PL_CELL(AGGF_PAIR_DOT, CELL_NEAR);
  } else if (box && bstride == 9) {
    if (mode == AGGF_PAIR_DIST)
      AGGF_PL_CELL(AGGF_PAIR_DIST, CELL_TRI);
    else if (mode == AGGF_PAIR_SQDIST)
      AGGF_PL_CELL(AGGF_PAIR_SQDIST, CELL_TRI);
    else
      AGGF_PL_CELL(AGGF_PAIR_DOT, CELL_TRI);
  } else if (box) {
#define AGGF_PL_PBC(MODE)                                                                                       \
  AGGF_LAUNCH((pairlist_pbc_kernel<T, MODE>), grid, block, 0, stream, (const T*)X, (const T*)C, (const T*)V,    \
              (const T*)Y, pairs, nT, m, n, P, frames, (const T*)box, bstride, (T*)out)
    if (mode == AGGF_PAIR_DIST)
      AGGF_PL_PBC(AGGF_PAIR_DIST);
    else if (mode == AGGF_PAIR_SQDIST)
      AGGF_PL_PBC(AGGF_PAIR_SQDIST);
    else
      AGGF_PL_PBC(AGGF_PAIR_DOT);
#undef AGGF_PL_PBC
  } else if (mode == AGGF_PAIR_DIST)
    AGGF_LAUNCH((pairlist_kernel<T, AGGF_PAIR_DIST>), grid, block, 0, stream, (const T*)X, (const T*)C, (const T*)V,
                (const T*)Y, pairs, nT, m, n, P, frames, (T*)out);
  else if (mode == AGGF_PAIR_SQDIST)
    AGGF_LAUNCH((pairlist_kernel<T, AGGF_PAIR_SQDIST>), grid, block, 0, stream, (const T*)X, (const T*)C, (const T*)V,
                (const T*)Y, pairs, nT, m, n, P, frames, (T*)out);
  else
    AGGF_LAUNCH((pairlist_kernel<T, AGGF_PAIR_DOT>), grid, block, 0, stream, (const T*)X, (const T*)C, (const T*)V,
                (const T*)Y, pairs, nT, m, n, P, frames, (T*)out);
#undef AGGF_PL_CELL
}

template <typename TI, typename TO, bool HAS_DV>
static void launch_pull_form(int form, hipStream_t stream, const void* W, const void* Dv, const void* Own,
                             const void* Oth, const int32_t* pairs, int32_t ocol, const int32_t* ptr,
                             const int32_t* idx, int64_t nT, int32_t ns, int32_t no, int64_t P, const void* box,
                             int32_t bstride, bool near, void* out) {
  const dim3 block(256);
  const int64_t tasks = nT * ns;
  if (box && bstride == 9 && near && form == PLP_LANE)
    AGGF_LAUNCH((pairlist_pull_pbc_kernel<TI, TO, HAS_DV, PLP_LANE, CELL_NEAR>), pairlist_grid(ceil_div(tasks, 256)), block, 0,
                stream, (const TI*)W, (const TI*)Dv, (const TI*)Own, (const TI*)Oth, pairs, ocol, ptr, idx, nT, ns, no,
                P, (const TI*)box, (TO*)out);
  else if (box && bstride == 9 && near)
    AGGF_LAUNCH((pairlist_pull_pbc_kernel<TI, TO, HAS_DV, PLP_WAVE, CELL_NEAR>), pairlist_grid(ceil_div(tasks, 4)), block, 0,
                stream, (const TI*)W, (const TI*)Dv, (const TI*)Own, (const TI*)Oth, pairs, ocol, ptr, idx, nT, ns, no,
                P, (const TI*)box, (TO*)out);
  else if (box && bstride == 9 && form == PLP_LANE)
    AGGF_LAUNCH((pairlist_pull_pbc_kernel<TI, TO, HAS_DV, PLP_LANE, CELL_TRI>), pairlist_grid(ceil_div(tasks, 256)), block, 0,
                stream, (const TI*)W, (const TI*)Dv, (const TI*)Own, (const TI*)Oth, pairs, ocol, ptr, idx, nT, ns, no,
                P, (const TI*)box, (TO*)out);
  else if (box && bstride == 9)
    AGGF_LAUNCH((pairlist_pull_pbc_kernel<TI, TO, HAS_DV, PLP_WAVE, CELL_TRI>), pairlist_grid(ceil_div(tasks, 4)), block, 0,
                stream, (const TI*)W, (const TI*)Dv, (const TI*)Own, (const TI*)Oth, pairs, ocol, ptr, idx, nT, ns, no,
                P, (const TI*)box, (TO*)out);
  else if (box && form == PLP_LANE)
    AGGF_LAUNCH((pairlist_pull_pbc_kernel<TI, TO, HAS_DV, PLP_LANE>), pairlist_grid(ceil_div(tasks, 256)), block, 0,
                stream, (const TI*)W, (const TI*)Dv, (const TI*)Own, (const TI*)Oth, pairs, ocol, ptr, idx, nT, ns, no,
                P, (const TI*)box, bstride, (TO*)out);
  else if (box)
    AGGF_LAUNCH((pairlist_pull_pbc_kernel<TI, TO, HAS_DV, PLP_WAVE>), pairlist_grid(ceil_div(tasks, 4)), block, 0,
                stream, (const TI*)W, (const TI*)Dv, (const TI*)Own, (const TI*)Oth, pairs, ocol, ptr, idx, nT, ns, no,
                P, (const TI*)box, bstride, (TO*)out);
  else if (form == PLP_LANE)
    AGGF_LAUNCH((pairlist_pull_kernel<TI, TO, HAS_DV, PLP_LANE>), pairlist_grid(ceil_div(tasks, 256)), block, 0, stream,
                (const TI*)W, (const TI*)Dv, (const TI*)Own, (const TI*)Oth, pairs, ocol, ptr, idx, nT, ns, no, P,
                (TO*)out);
  else
    AGGF_LAUNCH((pairlist_pull_kernel<TI, TO, HAS_DV, PLP_WAVE>), pairlist_grid(ceil_div(tasks, 4)), block, 0, stream,
                (const TI*)W, (const TI*)Dv, (const TI*)Own, (const TI*)Oth, pairs, ocol, ptr, idx, nT, ns, no, P,
                (TO*)out);
}

// the sums of one table (nothing to do without sites)
static void launch_pull(int in_dtype, int out_dtype, int32_t max_deg, hipStream_t stream, const void* W, const void* Dv,
                        const void* Own, const void* Oth, const int32_t* pairs, int32_t ocol, const int32_t* ptr,
                        const int32_t* idx, int64_t nT, int32_t ns, int32_t no, int64_t P, const void* box,
                        int32_t bstride, bool near, void* out) {
  if (ns == 0) return;
  const int form = max_deg > PLP_LANE_DEG ? PLP_WAVE : PLP_LANE;
#define AGGF_PULL_FORM(TI, TO)                                                                                       \
  (Dv ? launch_pull_form<TI, TO, true>(form, stream, W, Dv, Own, Oth, pairs, ocol, ptr, idx, nT, ns, no, P, box,     \
                                       bstride, near, out)                                                           \
      : launch_pull_form<TI, TO, false>(form, stream, W, Dv, Own, Oth, pairs, ocol, ptr, idx, nT, ns, no, P, box,    \
                                        bstride, near, out))
  if (in_dtype == AGGF_F32)
    AGGF_PULL_FORM(float, float);
  else if (out_dtype == AGGF_F32)
    AGGF_PULL_FORM(double, float);
  else
    AGGF_PULL_FORM(double, double);
#undef AGGF_PULL_FORM
}

// the box of a box form: (T, 3) or (3,) in the operands' dtype, or (T, 9): a triclinic cell per frame
static int pairlist_box(const char* who, const void* box, int32_t box_stride) {
  if (!box) return fail(AGGF_ERR_ARG, "%s: NULL box", who);
  if (box_stride != 0 && box_stride != 3 && box_stride != 9)
    return fail(AGGF_ERR_ARG, "%s: box_stride %d is none of 0, 3 and 9", who, box_stride);
  return AGGF_OK;
}

// K9c, open (box NULL) or under a box: one launch plan for both
static int pair_list_dist(const char* who, const void* X, const void* C, const void* V, const void* Y,
                          const int32_t* pairs, int64_t T, int32_t m, int32_t n, int64_t P, int dtype, int mode,
                          const void* box, int32_t box_stride, bool near, void* out, hipStream_t stream) {
  int64_t count = 0;
  const int rc = pairlist_shape(who, T, m, n, P, &count);
  if (rc != AGGF_OK) return rc;
  if (dtype != AGGF_F32 && dtype != AGGF_F64) return fail(AGGF_ERR_ARG, "%s: bad dtype", who);
  if (mode != AGGF_PAIR_DIST && mode != AGGF_PAIR_SQDIST && mode != AGGF_PAIR_DOT)
    return fail(AGGF_ERR_ARG, "%s: bad mode", who);
  if (count == 0) return AGGF_OK;
  if (!X || !C || !pairs || !out) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (mode == AGGF_PAIR_DOT && (!V || !Y)) return fail(AGGF_ERR_ARG, "%s: DOT needs V and Y", who);
  // a wave walks all frames of its 64 pairs unless that leaves the chip short of tasks
  const int64_t pblocks = ceil_div(P, 64);
  int64_t frames = T;
  while (frames > PL_MIN_FRAMES && pblocks * ceil_div(T, frames) < PL_TARGET_TASKS) frames = (frames + 1) / 2;
  const int64_t waves = pblocks * ceil_div(T, frames);  // <= count
  const dim3 grid = pairlist_grid(ceil_div(waves, 4));
  if (dtype == AGGF_F64)
    launch_pairlist<double>(mode, grid, stream, X, C, V, Y, pairs, T, m, n, P, frames, box, box_stride, near, out);
  else
    launch_pairlist<float>(mode, grid, stream, X, C, V, Y, pairs, T, m, n, P, frames, box, box_stride, near, out);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

// K9d, open (box NULL) or under a box
static int pair_list_pull(const char* who, const void* W, const void* Dv, const void* X, const void* C,
                          const int32_t* pairs, const int32_t* a_ptr, const int32_t* a_idx, const int32_t* b_ptr,
                          const int32_t* b_idx, int32_t max_deg_a, int32_t max_deg_b, int64_t T, int32_t m, int32_t n,
                          int64_t P, int in_dtype, const void* box, int32_t box_stride, bool near, void* A, void* B,
                          int out_dtype, hipStream_t stream) {
  int64_t count = 0;
  const int rc = pairlist_shape(who, T, m, n, P, &count);
  if (rc != AGGF_OK) return rc;
  if ((in_dtype != AGGF_F32 && in_dtype != AGGF_F64) || (out_dtype != AGGF_F32 && out_dtype != AGGF_F64))
    return fail(AGGF_ERR_ARG, "%s: bad dtype", who);
  if (in_dtype == AGGF_F32 && out_dtype == AGGF_F64)
    return fail(AGGF_ERR_ARG, "%s: float32 inputs with float64 outputs: widen the inputs", who);
  if (max_deg_a < 0 || max_deg_b < 0) return fail(AGGF_ERR_ARG, "%s: negative degree", who);
  if (count == 0 || (!A && !B)) return AGGF_OK;
  if (!W || !X || !C || !pairs) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if ((A && (!a_ptr || !a_idx)) || (B && (!b_ptr || !b_idx)))
    return fail(AGGF_ERR_ARG, "%s: an output without its incidence table", who);
  if (A)
    launch_pull(in_dtype, out_dtype, max_deg_a, stream, W, Dv, X, C, pairs, 0, a_ptr, a_idx, T, n, m, P, box,
                box_stride, near, A);
  if (B)
    launch_pull(in_dtype, out_dtype, max_deg_b, stream, W, Dv, C, X, pairs, 1, b_ptr, b_idx, T, m, n, P, box,
                box_stride, near, B);
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

}  // namespace aggf

using namespace aggf;

extern "C" int aggf_pair_list_dist(const void* X, const void* C, const void* V, const void* Y, const int32_t* pairs,
                                   int64_t T, int32_t m, int32_t n, int64_t P, int dtype, int mode, void* out,
                                   void* stream_v) {
  return pair_list_dist("aggf_pair_list_dist", X, C, V, Y, pairs, T, m, n, P, dtype, mode, nullptr, 0, false, out,
                        (hipStream_t)stream_v);
}

extern "C" int aggf_pair_list_dist_pbc(const void* X, const void* C, const void* V, const void* Y,
                                       const int32_t* pairs, int64_t T, int32_t m, int32_t n, int64_t P, int dtype,
                                       int mode, const void* box, int32_t box_stride, void* out, void* stream_v) {
  const int rc = pairlist_box("aggf_pair_list_dist_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  return pair_list_dist("aggf_pair_list_dist_pbc", X, C, V, Y, pairs, T, m, n, P, dtype, mode, box, box_stride, false,
                        out, (hipStream_t)stream_v);
}

// the cell of a `_cell` entry and its image selector: AGGF_IMAGES_BRICK (the form of box_stride 9) or AGGF_IMAGES_NEAREST
static int pairlist_cell(const char* who, const void* cell, int images) {
  if (!cell) return fail(AGGF_ERR_ARG, "%s: NULL cell", who);
  if (images != AGGF_IMAGES_BRICK && images != AGGF_IMAGES_NEAREST)
    return fail(AGGF_ERR_ARG, "%s: images %d is neither AGGF_IMAGES_BRICK nor AGGF_IMAGES_NEAREST", who, images);
  return AGGF_OK;
}

extern "C" int aggf_pair_list_dist_cell(const void* X, const void* C, const void* V, const void* Y,
                                        const int32_t* pairs, int64_t T, int32_t m, int32_t n, int64_t P, int dtype,
                                        int mode, const void* cell, void* out, void* stream_v, int images) {
  const int rc = pairlist_cell("aggf_pair_list_dist_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return pair_list_dist("aggf_pair_list_dist_cell", X, C, V, Y, pairs, T, m, n, P, dtype, mode, cell, 9,
                        images == AGGF_IMAGES_NEAREST, out, (hipStream_t)stream_v);
}

extern "C" int aggf_pair_list_pull(const void* W, const void* Dv, const void* X, const void* C, const int32_t* pairs,
                                   const int32_t* a_ptr, const int32_t* a_idx, const int32_t* b_ptr,
                                   const int32_t* b_idx, int32_t max_deg_a, int32_t max_deg_b, int64_t T, int32_t m,
                                   int32_t n, int64_t P, int in_dtype, void* A, void* B, int out_dtype,
                                   void* stream_v) {
  return pair_list_pull("aggf_pair_list_pull", W, Dv, X, C, pairs, a_ptr, a_idx, b_ptr, b_idx, max_deg_a, max_deg_b, T,
                        m, n, P, in_dtype, nullptr, 0, false, A, B, out_dtype, (hipStream_t)stream_v);
}

extern "C" int aggf_pair_list_pull_pbc(const void* W, const void* Dv, const void* X, const void* C,
                                       const int32_t* pairs, const int32_t* a_ptr, const int32_t* a_idx,
                                       const int32_t* b_ptr, const int32_t* b_idx, int32_t max_deg_a,
                                       int32_t max_deg_b, int64_t T, int32_t m, int32_t n, int64_t P, int in_dtype,
                                       const void* box, int32_t box_stride, void* A, void* B, int out_dtype,
                                       void* stream_v) {
  const int rc = pairlist_box("aggf_pair_list_pull_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  return pair_list_pull("aggf_pair_list_pull_pbc", W, Dv, X, C, pairs, a_ptr, a_idx, b_ptr, b_idx, max_deg_a,
                        max_deg_b, T, m, n, P, in_dtype, box, box_stride, false, A, B, out_dtype,
                        (hipStream_t)stream_v);
}

extern "C" int aggf_pair_list_pull_cell(const void* W, const void* Dv, const void* X, const void* C,
                                        const int32_t* pairs, const int32_t* a_ptr, const int32_t* a_idx,
                                        const int32_t* b_ptr, const int32_t* b_idx, int32_t max_deg_a,
                                        int32_t max_deg_b, int64_t T, int32_t m, int32_t n, int64_t P, int in_dtype,
                                        const void* cell, void* A, void* B, int out_dtype, void* stream_v,
                                        int images) {
  const int rc = pairlist_cell("aggf_pair_list_pull_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return pair_list_pull("aggf_pair_list_pull_cell", W, Dv, X, C, pairs, a_ptr, a_idx, b_ptr, b_idx, max_deg_a,
                        max_deg_b, T, m, n, P, in_dtype, cell, 9, images == AGGF_IMAGES_NEAREST, A, B, out_dtype,
                        (hipStream_t)stream_v);
}
