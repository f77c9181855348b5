// K11: make molecules whole under an orthorhombic periodic box (aggforce_amd/pbc.py: make_whole; _autograd.py:
// MakeWhole).  X (T, N, 3), a spanning forest over the N atoms (parent[i] in [-1, N), -1 a root; parents may follow
// their children), a box per frame.  Per frame and Cartesian component, with the roundings of min_image
// (aggf_common.h) written out and contraction off:
//
//   n_i = 0 for a root, else (int) rint((x_i - x_parent(i)) invL)      an EDGE count: a function of the input alone
//   k_i = n_i + the n of all ancestors of i                            an exact integer sum along the root path
//   u_i = fma(-(T)k_i, L, x_i)                                         one rounding
//
// Nothing is sequential along the tree: the k are prefix sums along root paths, formed by pointer jumping over the
// host's tables jumps[r][i] = the 2^r-th ancestor of i or -1 -- round r: k_new[i] = k[i] + (jumps[r][i] >= 0 ?
// k[jumps[r][i]] : 0), R rounds with 2^R >= depth, the counts double-buffered with a barrier between rounds.  Integer
// sums make the counts independent of schedule and form: the two forms below, and a NumPy restatement, agree bit for
// bit.  A root never moves; where all counts are 0 the output is the input bit for bit (fma(-0, L, x) == x).
//
//   whole_lds_kernel<T>     LDS form: a workgroup owns a run of whole frames (several small ones, or one) and keeps
//                           their counts in LDS; edge counts, barrier, R rounds, shifted store.  One launch.
//   whole_edge_kernel<T>, whole_jump_kernel, whole_shift_kernel<T>
//                           global form, for N beyond the LDS bound: the same __device__ bodies with the two count
//                           buffers in the caller's workspace; one launch for the edge counts, one per round, one for
//                           the shift.
//
// In place (out == X) is allowed in both forms: no coordinate is written before every count that reads it is final --
// the LDS form reads coordinates only before its first barrier and a workgroup's frames are its own, the global form
// writes coordinates in its last launch only.  No atomics; nothing reads another workgroup's writes within a launch.
//
// Edge behaviour.  A box length that is not positive and finite: that frame's counts are 0 and its coordinates NaN
// (box_lengths' convention).  A non-finite (x_i - x_parent) invL: n_i = 0, so a non-finite coordinate passes through
// to its own output and shifts nothing else.  |n_i| is clamped to 2^15 (WH_MAX_EDGE) and the host refuses a forest of
// depth 2^16 or more, so no int32 sum overflows.  Every index read from parent and jumps is tested against N: one
// out of range marks the atom -- and whatever sums over it -- with WH_BAD, whose coordinates come out NaN (its image
// counts read WH_BAD = INT32_MIN), instead of reading outside X or the counts.
#include "aggf_common.h"

namespace aggf {

constexpr int32_t WH_MAX_EDGE = 1 << 15;
constexpr int32_t WH_BAD = INT32_MIN;  // never a sum: |k| <= (2^16 - 1) 2^15 < 2^31
constexpr int32_t WH_MAX_ROUNDS = 16;  // depth < 2^16

// ---- the bodies both forms run
// one length of a frame's box and its inverse, as box_lengths forms them (NaN unless positive and finite)
template <typename T>
__device__ __forceinline__ void whole_box_length(const T* __restrict__ box, T* L, T* invL) {
  const T l = *box;
  const bool good = l > (T)0 && l < (T)__builtin_inf();
  *L = good ? l : (T)__builtin_nan("");
  *invL = (T)1 / *L;
}
__device__ __forceinline__ float wh_rint(float q) { return __builtin_rintf(q); }
__device__ __forceinline__ double wh_rint(double q) { return __builtin_rint(q); }
__device__ __forceinline__ float wh_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double wh_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// n_i of one component from the atom's and its parent's coordinate
template <typename T>
__device__ __forceinline__ int32_t whole_edge_count(T x, T xp, T invL) {
#pragma clang fp contract(off)
  const T q = (x - xp) * invL;
  if (!(__builtin_fabs(q) < (T)__builtin_inf())) return 0;  // NaN, +-inf (a bad box included: invL is NaN)
  T r = wh_rint(q);
  r = r > (T)WH_MAX_EDGE ? (T)WH_MAX_EDGE : (r < (T)-WH_MAX_EDGE ? (T)-WH_MAX_EDGE : r);
  return (int32_t)r;
}
// n_i of component c of an atom whose parent is p; row: the frame's N x 3 coordinates
template <typename T>
__device__ __forceinline__ int32_t whole_edge(const T* row, T x, int32_t p, int32_t c, int32_t N, T invL) {
  if (p == -1) return 0;
  if (!((uint32_t)p < (uint32_t)N)) return WH_BAD;
  return whole_edge_count(x, row[3 * (int64_t)p + c], invL);
}
// one jump: k + (the count of the 2^r-th ancestor)
__device__ __forceinline__ int32_t whole_add(int32_t k, int32_t ka) {
  return (k == WH_BAD || ka == WH_BAD) ? WH_BAD : k + ka;
}
template <typename T>
__device__ __forceinline__ T whole_shift(int32_t k, T L, T x) {
  if (k == WH_BAD) return (T)__builtin_nan("");
  return wh_fma(-(T)k, L, x);
}


// ---- the triclinic forms (whole_lds_kernel<T, CELL_TRI>, whole_edge_kernel<..>, whole_shift_kernel<..>): `box` is (T, 9), a
// row-major 3 x 3 cell per frame (CellFrame, aggf_common.h).  The edge counts of an atom are the three counts of the
// brick reduction of x_i - x_parent(i), each treated as the box form treats its one: 0 where q is not finite, clamped
// to WH_MAX_EDGE, and the next stage reduced with that count:
//   kc = cnt(dz (1/cz));  dy = fma(-kc, cy, dy);  dx = fma(-kc, cx, dx)
//   kb = cnt(dy (1/by));  dx = fma(-kb, bx, dx)
//   ka = cnt(dx (1/ax))
// Element c of an atom holds the count of lattice vector c (0: a, 1: b, 2: c); the jump rounds sum each as before, and
//   u = x - kc c - kb b - ka a   as nested fmas in that order, component by component (zero entries skipped).
// With zero off-diagonal entries every number is the box form's, bit for bit.  A bad cell (cell_frame) is all NaN:
// counts 0, coordinates NaN.
template <typename T>
__device__ __forceinline__ T whole_count(T q) {
  if (!(__builtin_fabs(q) < (T)__builtin_inf())) return (T)0;
  const T r = wh_rint(q);
  return r > (T)WH_MAX_EDGE ? (T)WH_MAX_EDGE : (r < (T)-WH_MAX_EDGE ? (T)-WH_MAX_EDGE : r);
}
// the count of lattice vector c for atom i whose parent is p; row: the frame's N x 3 coordinates
template <typename T>
__device__ __forceinline__ int32_t whole_edge_cell(const T* row, int32_t i, int32_t p, int32_t c, int32_t N,
                                                   const CellFrame<T>& h) {
#pragma clang fp contract(off)
  if (p == -1) return 0;
  if (!((uint32_t)p < (uint32_t)N)) return WH_BAD;
  const T* x = row + 3 * (int64_t)i;
  const T* xp = row + 3 * (int64_t)p;
  T d0 = x[0] - xp[0], d1 = x[1] - xp[1];
  const T d2 = x[2] - xp[2];
  const T kc = whole_count(d2 * h.icz);
  d1 = wh_fma(-kc, h.cy, d1), d0 = wh_fma(-kc, h.cx, d0);
  const T kb = whole_count(d1 * h.iby);
  d0 = wh_fma(-kb, h.bx, d0);
  const T ka = whole_count(d0 * h.iax);
  return (int32_t)(c == 0 ? ka : (c == 1 ? kb : kc));
}
// component c of the shifted atom from its three counts and component c of the three lattice vectors (ac: c == 0
// only, bc: c <= 1 only)
template <typename T>
__device__ __forceinline__ T whole_shift_cell(int32_t ka, int32_t kb, int32_t kc, int32_t c, T ac, T bc, T cc, T x) {
  if (ka == WH_BAD || kb == WH_BAD || kc == WH_BAD) return (T)__builtin_nan("");
  T u = wh_fma(-(T)kc, cc, x);
  if (c <= 1) u = wh_fma(-(T)kb, bc, u);
  if (c == 0) u = wh_fma(-(T)ka, ac, u);
  return u;
}

// ---------------------------------------------------------------------------
// LDS form.  A workgroup of WH_THREADS lanes takes `frames` consecutive frames at a time: a contiguous span of
// len = frames 3 N elements of X, element g of the span being component c = (g mod 3N) mod 3 of atom i = (g mod 3N) / 3
// of frame g / 3N.  The span is cut into 16-byte cells on X's own 16-byte grid (the first and last cell may be
// partial: a row of 3 N elements starts anywhere); lane l owns cells l, l + WH_THREADS, ... -- at most WH_ELEMS
// elements -- and keeps their coordinates and atom indices in registers from the load to the store, so every
// coordinate is read once and written once: a whole cell by one 16-byte access (the store too when out sits on the
// same grid as X, else by elements), a partial cell by elements.  The parent's coordinate of the edge count is a
// second, cached read of the same frame.  LDS holds the frames' L and 1 / L and the two count buffers of `len` int32.
//
// The largest N.  The counts are 3 int32 per atom, double-buffered: 24 bytes per atom, plus 6 lengths.  The form runs
// ONE workgroup of 16 waves per CU -- at every N: the kernel holds 121 (float32) / 128 (float64, 9 spilled) vector
// registers for a lane's WH_ELEMS coordinates and indices, which leaves 4 waves per SIMD = 16 waves per CU = one
// 1024-lane workgroup, whatever LDS a frame takes.  At that occupancy the CU's 160 KiB of LDS (163,840 B, which one
// workgroup may take whole) can all go to one frame:
//   24 N + 6 * 8 <= 163,840   =>   N <= 6824   (WH_LDS_MAX_N; the lengths counted as float64 for both dtypes)
// and a lane then owns ceil((3 * 6824 + 3) / 1024) = 20 elements = 5 cells of float32 or 10 of float64 (WH_ELEMS).
// The LDS of a launch is sized by its frames (dynamic size).  Frames of at most WH_SPAN / 3 atoms are grouped up to a
// span of WH_SPAN = 4096 elements (one float32 cell per lane), at most WH_MAX_FRAMES of them, fewer while that leaves
// under WH_MIN_GROUPS workgroups.  The register arrays are sized for the largest frame and used at every N: a variant
// with fewer cells per lane for small frames (two or more workgroups per CU) is not built.
// (Measured rates, and why they are below the streaming kernels': DESIGN.md section 3, K11.)
constexpr int WH_THREADS = 1024;
constexpr int WH_ELEMS = 20;
constexpr int32_t WH_LDS_BYTES = 160 * 1024;
constexpr int32_t WH_LDS_MAX_N = (WH_LDS_BYTES - 6 * 8) / 24;
constexpr int32_t WH_SPAN = 4096;
constexpr int32_t WH_MAX_FRAMES = 64;
constexpr int64_t WH_MIN_GROUPS = 512;  // two rounds of one workgroup on each of 256 CUs
static_assert(WH_LDS_MAX_N == 6824, "the bound derived above");
static_assert((3 * (int64_t)WH_LDS_MAX_N + 3 + 3) / 4 <= (int64_t)WH_THREADS * (WH_ELEMS / 4) &&
                  (3 * (int64_t)WH_LDS_MAX_N + 1 + 1) / 2 <= (int64_t)WH_THREADS * (WH_ELEMS / 2),
              "a lane's registers hold the largest frame");

// A triclinic frame stages nine numbers (CellFrame) where a box stages six: the largest frame of the cell form is one
// atom smaller, 24 N + 80 <= 163,840 => N <= 6823 (WH_LDS_MAX_N_CELL); nothing else of the plan differs.
constexpr int32_t WH_LDS_MAX_N_CELL = (WH_LDS_BYTES - 80) / 24;
static_assert(WH_LDS_MAX_N_CELL == WH_LDS_MAX_N - 1, "the bound derived above");
static inline int64_t whole_lds_lengths_bytes(int32_t frames, bool cell = false) {
  return round_up((cell ? 9 : 6) * (int64_t)frames * 8, 16);
}
// (a forest without rounds never touches the second count buffer: it is not allocated)
static inline int64_t whole_lds_bytes(int32_t frames, int32_t N, int32_t rounds, bool cell = false) {
  return whole_lds_lengths_bytes(frames, cell) + (rounds > 0 ? 2 : 1) * 4 * 3 * (int64_t)frames * N;
}
static int32_t whole_lds_frames(int64_t T, int32_t N) {
  int64_t f = WH_SPAN / (3 * (int64_t)N);
  if (f > WH_MAX_FRAMES) f = WH_MAX_FRAMES;
  if (f > T) f = T;
  while (f > 1 && ceil_div(T, f) < WH_MIN_GROUPS) f = (f + 1) / 2;
  return f < 1 ? 1 : (int32_t)f;
}

template <typename T, int CELL>
__device__ __forceinline__ void whole_lds_body(const T* X, int64_t nT, int32_t N, const int32_t* __restrict__ parent,
                                               const int32_t* __restrict__ jumps, int32_t rounds,
                                               const T* __restrict__ box, int32_t bstride, int32_t frames, T* out,
                                               int32_t* __restrict__ images) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  using V = typename Vec16<T>::type;
  constexpr int VN = Vec16<T>::N, SLOTS = WH_ELEMS / VN;
  const int32_t n3 = 3 * N, tid = threadIdx.x;
  T* sL = reinterpret_cast<T*>(smem_raw);
  T* sI = sL + 3 * frames;
  CellFrame<T>* sH = reinterpret_cast<CellFrame<T>*>(smem_raw);  // (CELL_TRI: instead of sL and sI)
  int32_t* kbuf = reinterpret_cast<int32_t*>(smem_raw + ((CELL == CELL_TRI ? 9 : 6) * (int64_t)frames * 8 + 15) / 16 * 16);
  const int64_t groups = (nT + frames - 1) / frames;
  for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int64_t t0 = grp * frames;
    const int32_t nf = t0 + frames <= nT ? frames : (int32_t)(nT - t0);
    const int32_t len = nf * n3;
    const int64_t base = t0 * n3;
    const T* xs = X + base;
    T* os = out + base;
    const int32_t off = (int32_t)(((uintptr_t)xs / sizeof(T)) % VN);  // elements of the first cell before the span
    const int32_t ncell = (off + len + VN - 1) / VN;
    const bool vec_out = ((uintptr_t)os & 15) == ((uintptr_t)xs & 15);
    int32_t* cur = kbuf;
    int32_t* nxt = kbuf + (int64_t)frames * n3;
    if (CELL == CELL_BOX && tid < 3 * nf) whole_box_length(box + (t0 + tid / 3) * bstride + tid % 3, sL + tid, sI + tid);
    if (CELL == CELL_TRI && tid < nf) cell_frame(box + (t0 + tid) * 9, sH[tid]);
    __syncthreads();

    // per owned element: coordinate and meta = atom index | (3 frame + component) << 16; -1: not in the span
    T xr[SLOTS][VN];
    int32_t meta[SLOTS][VN];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int32_t cell = s * WH_THREADS + tid;
      const int32_t g0 = cell * VN - off;
#pragma unroll
      for (int q = 0; q < VN; ++q) xr[s][q] = (T)0, meta[s][q] = -1;
      if (cell >= ncell) continue;
      if (g0 >= 0 && g0 + VN <= len) {
        const V v = *reinterpret_cast<const V*>(xs + g0);
#pragma unroll
        for (int q = 0; q < VN; ++q) xr[s][q] = v[q];
      } else {
#pragma unroll
        for (int q = 0; q < VN; ++q)
          if (g0 + q >= 0 && g0 + q < len) xr[s][q] = xs[g0 + q];
      }
      // (frame, atom, component) of the cell's first element in the span by one division, of the others by stepping
      const int32_t gs = g0 < 0 ? 0 : g0;
      int32_t f = gs / n3, i = (gs - f * n3) / 3, c = gs - f * n3 - 3 * i;
#pragma unroll
      for (int q = 0; q < VN; ++q) {
        const int32_t g = g0 + q;
        if (g < gs || g >= len) continue;
        meta[s][q] = i | ((3 * f + c) << 16);
        if (CELL == CELL_TRI)
          cur[g] = whole_edge_cell<T>(xs + (int64_t)f * n3, i, parent[i], c, N, sH[f]);
        else
          cur[g] = whole_edge<T>(xs + (int64_t)f * n3, xr[s][q], parent[i], c, N, sI[3 * f + c]);
        if (++c == 3) {
          c = 0;
          if (++i == N) i = 0, ++f;
        }
      }
    }
    __syncthreads();  // every coordinate of the span has been read: from here on `out` may be X

    for (int32_t r = 0; r < rounds; ++r) {
      const int32_t* jr = jumps + (int64_t)r * N;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int32_t g0 = (s * WH_THREADS + tid) * VN - off;
#pragma unroll
        for (int q = 0; q < VN; ++q) {
          if (meta[s][q] < 0) continue;
          const int32_t i = meta[s][q] & 0xffff, a = jr[i];
          int32_t k = cur[g0 + q];
          if (a != -1) k = (uint32_t)a < (uint32_t)N ? whole_add(k, cur[g0 + q + 3 * (a - i)]) : WH_BAD;
          nxt[g0 + q] = k;
        }
      }
      __syncthreads();
      int32_t* sw = cur;
      cur = nxt, nxt = sw;
    }

#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int32_t cell = s * WH_THREADS + tid;
      const int32_t g0 = cell * VN - off;
      if (cell >= ncell) continue;
      T u[VN];
#pragma unroll
      for (int q = 0; q < VN; ++q) {
        if (meta[s][q] < 0) {
          u[q] = (T)0;
        } else if (CELL == CELL_TRI) {
          const int32_t fc = meta[s][q] >> 16, f = fc / 3, c = fc - 3 * f;
          const int32_t* k = cur + (g0 + q - c);
          const T* e = &sH[f].ax;  // ax | bx by | cx cy cz
          u[q] = whole_shift_cell<T>(k[0], k[1], k[2], c, e[0], e[c <= 1 ? 1 + c : 1], e[3 + c], xr[s][q]);
        } else {
          u[q] = whole_shift<T>(cur[g0 + q], sL[meta[s][q] >> 16], xr[s][q]);
        }
      }
      if (vec_out && g0 >= 0 && g0 + VN <= len) {
        V v;
#pragma unroll
        for (int q = 0; q < VN; ++q) v[q] = u[q];
        *reinterpret_cast<V*>(os + g0) = v;
      } else {
#pragma unroll
        for (int q = 0; q < VN; ++q)
          if (meta[s][q] >= 0) os[g0 + q] = u[q];
      }
    }
    if (images)
      for (int32_t g = tid; g < len; g += WH_THREADS) images[base + g] = cur[g];
    __syncthreads();  // (the next group's lengths and counts reuse the LDS)
  }
}

template <typename T>
__global__ __launch_bounds__(WH_THREADS) void whole_lds_kernel(const T* X, int64_t nT, int32_t N,
                                                               const int32_t* __restrict__ parent,
                                                               const int32_t* __restrict__ jumps, int32_t rounds,
                                                               const T* __restrict__ box, int32_t bstride,
                                                               int32_t frames, T* out, int32_t* __restrict__ images) {
  whole_lds_body<T, CELL_BOX>(X, nT, N, parent, jumps, rounds, box, bstride, frames, out, images);
}

// (the triclinic forms of the three kernels are overloads with a second template argument, CELL_TRI the only value
// instantiated, and no stride among their arguments)
template <typename T, int CELL>
__global__ __launch_bounds__(WH_THREADS) void whole_lds_kernel(const T* X, int64_t nT, int32_t N,
                                                               const int32_t* __restrict__ parent,
                                                               const int32_t* __restrict__ jumps, int32_t rounds,
                                                               const T* __restrict__ cell, int32_t frames, T* out,
                                                               int32_t* __restrict__ images) {
  static_assert(CELL == CELL_TRI, "the triclinic form");
  whole_lds_body<T, CELL>(X, nT, N, parent, jumps, rounds, cell, 9, frames, out, images);
}

// ---------------------------------------------------------------------------
// Global form: element e of the (T, 3 N) arrays per lane, grid-stride; counts (T, 3 N) int32 in the workspace.
template <typename T>
__global__ __launch_bounds__(256) void whole_edge_kernel(const T* __restrict__ X, int64_t nT, int32_t N,
                                                         const int32_t* __restrict__ parent, const T* __restrict__ box,
                                                         int32_t bstride, int32_t* __restrict__ cnt) {
  const int64_t n3 = 3 * (int64_t)N, total = nT * n3;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int64_t t = g / n3;
    const int32_t e = (int32_t)(g - t * n3), i = e / 3, c = e - 3 * i;
    T L, iL;
    whole_box_length(box + t * bstride + c, &L, &iL);
    cnt[g] = whole_edge<T>(X + t * n3, X[g], parent[i], c, N, iL);
  }
}

template <typename T, int CELL>
__global__ __launch_bounds__(256) void whole_edge_kernel(const T* __restrict__ X, int64_t nT, int32_t N,
                                                         const int32_t* __restrict__ parent,
                                                         const T* __restrict__ cell, int32_t* __restrict__ cnt) {
  static_assert(CELL == CELL_TRI, "the triclinic form");
  const int64_t n3 = 3 * (int64_t)N, total = nT * n3;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int64_t t = g / n3;
    const int32_t e = (int32_t)(g - t * n3), i = e / 3, c = e - 3 * i;
    CellFrame<T> h;
    cell_frame(cell + t * 9, h);
    cnt[g] = whole_edge_cell<T>(X + t * n3, i, parent[i], c, N, h);
  }
}

__global__ __launch_bounds__(256) void whole_jump_kernel(const int32_t* __restrict__ cur, const int32_t* __restrict__ jr,
                                                         int64_t nT, int32_t N, int32_t* __restrict__ nxt) {
  const int64_t n3 = 3 * (int64_t)N, total = nT * n3;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int32_t e = (int32_t)(g % n3), i = e / 3, a = jr[i];
    int32_t k = cur[g];
    if (a != -1) k = (uint32_t)a < (uint32_t)N ? whole_add(k, cur[g + 3 * ((int64_t)a - i)]) : WH_BAD;
    nxt[g] = k;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void whole_shift_kernel(const T* X, const int32_t* __restrict__ cnt, int64_t nT,
                                                          int32_t N, const T* __restrict__ box, int32_t bstride, T* out,
                                                          int32_t* __restrict__ images) {
  const int64_t n3 = 3 * (int64_t)N, total = nT * n3;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int64_t t = g / n3;
    const int32_t c = (int32_t)((g - t * n3) % 3);
    T L, iL;
    whole_box_length(box + t * bstride + c, &L, &iL);
    const int32_t k = cnt[g];
    out[g] = whole_shift<T>(k, L, X[g]);
    if (images) images[g] = k;
  }
}

template <typename T, int CELL>
__global__ __launch_bounds__(256) void whole_shift_kernel(const T* X, const int32_t* __restrict__ cnt, int64_t nT,
                                                          int32_t N, const T* __restrict__ cell, T* out,
                                                          int32_t* __restrict__ images) {
  static_assert(CELL == CELL_TRI, "the triclinic form");
  const int64_t n3 = 3 * (int64_t)N, total = nT * n3;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int64_t t = g / n3;
    const int32_t c = (int32_t)((g - t * n3) % 3);
    const T* m = cell + t * 9;  // (component c of the rows a, b, c: m[c], m[3 + c], m[6 + c]; no inverse is needed)
    const T nan = (T)__builtin_nan("");
    const bool ok = cell_good(m);
    const int32_t* k = cnt + (g - c);
    out[g] = whole_shift_cell<T>(k[0], k[1], k[2], c, ok ? m[0] : nan, ok ? m[c <= 1 ? 3 + c : 3] : nan,
                                 ok ? m[6 + c] : nan, X[g]);
    if (images) images[g] = k[c];
  }
}

// ---------------------------------------------------------------------------
constexpr int WH_AUTO = 0, WH_LDS = 1, WH_GLOBAL = 2;

// the global form's two count buffers (one without rounds); 0: the sizes do not fit
static int64_t whole_ws_bytes(int64_t T, int32_t N, int32_t rounds) {
  int64_t elems = 0;
  if (__builtin_mul_overflow(T, 3 * (int64_t)N, &elems) || elems > INT64_MAX / 16) return 0;
  return elems * 4 * (rounds > 0 ? 2 : 1);
}

static inline dim3 whole_grid(int64_t blocks, int64_t cap) {
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return dim3((unsigned)blocks);
}

template <typename T>
static int launch_whole_lds(hipStream_t stream, const void* X, int64_t nT, int32_t N, const int32_t* parent,
                            const int32_t* jumps, int32_t rounds, const void* box, int32_t bstride, void* out,
                            int32_t* images) {
  const bool cell = bstride == 9;
  static PerDeviceOnce once[2];
  if (!*once[cell].flag()) {
    AGGF_HIP_OK(hipFuncSetAttribute(cell ? (const void*)whole_lds_kernel<T, CELL_TRI> : (const void*)whole_lds_kernel<T>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, WH_LDS_BYTES));
    *once[cell].flag() = true;
  }
  const int32_t frames = whole_lds_frames(nT, N);
  const int64_t lds = whole_lds_bytes(frames, N, rounds, cell);
  if (lds > WH_LDS_BYTES) return fail(AGGF_ERR_ARG, "aggf_make_whole: %d atoms do not fit the LDS form", N);
  if (cell)
    AGGF_LAUNCH((whole_lds_kernel<T, CELL_TRI>), whole_grid(ceil_div(nT, frames), 1 << 20), dim3(WH_THREADS), (size_t)lds,
                stream, (const T*)X, nT, N, parent, jumps, rounds, (const T*)box, frames, (T*)out, images);
  else
    AGGF_LAUNCH((whole_lds_kernel<T>), whole_grid(ceil_div(nT, frames), 1 << 20), dim3(WH_THREADS), (size_t)lds, stream,
                (const T*)X, nT, N, parent, jumps, rounds, (const T*)box, bstride, frames, (T*)out, images);
  return AGGF_OK;
}

template <typename T>
static void launch_whole_global(hipStream_t stream, const void* X, int64_t nT, int32_t N, const int32_t* parent,
                                const int32_t* jumps, int32_t rounds, const void* box, int32_t bstride, void* out,
                                int32_t* images, void* ws) {
  const int64_t total = nT * 3 * (int64_t)N;
  const dim3 grid = whole_grid(ceil_div(total, 256), 65536), block(256);
  int32_t* cur = (int32_t*)ws;
  int32_t* nxt = cur + total;
  const bool cell = bstride == 9;
  if (cell)
    AGGF_LAUNCH((whole_edge_kernel<T, CELL_TRI>), grid, block, 0, stream, (const T*)X, nT, N, parent, (const T*)box, cur);
  else
    AGGF_LAUNCH((whole_edge_kernel<T>), grid, block, 0, stream, (const T*)X, nT, N, parent, (const T*)box, bstride, cur);
  for (int32_t r = 0; r < rounds; ++r) {
    AGGF_LAUNCH(whole_jump_kernel, grid, block, 0, stream, (const int32_t*)cur, jumps + (int64_t)r * N, nT, N, nxt);
    int32_t* sw = cur;
    cur = nxt, nxt = sw;
  }
  if (cell)
    AGGF_LAUNCH((whole_shift_kernel<T, CELL_TRI>), grid, block, 0, stream, (const T*)X, (const int32_t*)cur, nT, N,
                (const T*)box, (T*)out, images);
  else
    AGGF_LAUNCH((whole_shift_kernel<T>), grid, block, 0, stream, (const T*)X, (const int32_t*)cur, nT, N, (const T*)box,
                bstride, (T*)out, images);
}

}  // namespace aggf

using namespace aggf;

extern "C" int32_t aggf_make_whole_lds_max_sites(void) { return WH_LDS_MAX_N; }

extern "C" size_t aggf_make_whole_workspace_bytes(int64_t T, int32_t N, int32_t rounds, int dtype) {
  (void)dtype;  // (the counts are int32 whatever the coordinates are)
  if (T <= 0 || N <= 0 || rounds < 0) return 0;
  return (size_t)whole_ws_bytes(T, N, rounds);
}

extern "C" int aggf_make_whole(const void* X, int64_t T, int32_t N, int dtype, const int32_t* parent,
                               const int32_t* jumps, int32_t rounds, const void* box, int32_t box_stride, void* out,
                               int32_t* images, void* ws, size_t ws_bytes, int form, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (T < 0 || N < 0) return fail(AGGF_ERR_ARG, "aggf_make_whole: negative shape");
  if (dtype != AGGF_F32 && dtype != AGGF_F64) return fail(AGGF_ERR_ARG, "aggf_make_whole: bad dtype");
  if (rounds < 0 || rounds > WH_MAX_ROUNDS)
    return fail(AGGF_ERR_ARG, "aggf_make_whole: %d rounds (a forest of depth 2^16 or more is refused)", rounds);
  if (!box) return fail(AGGF_ERR_ARG, "aggf_make_whole: NULL box");
  if (box_stride != 0 && box_stride != 3 && box_stride != 9)
    return fail(AGGF_ERR_ARG, "aggf_make_whole: box_stride %d is none of 0, 3 and 9", box_stride);
  const int32_t lds_max = box_stride == 9 ? WH_LDS_MAX_N_CELL : WH_LDS_MAX_N;
  if (form != WH_AUTO && form != WH_LDS && form != WH_GLOBAL) return fail(AGGF_ERR_ARG, "aggf_make_whole: bad form");
  if (T == 0 || N == 0) return AGGF_OK;
  const int64_t ws_need = whole_ws_bytes(T, N, rounds);
  if (ws_need == 0) return fail(AGGF_ERR_ARG, "aggf_make_whole: T N does not fit a 64-bit byte offset");
  if (!X || !parent || !out) return fail(AGGF_ERR_ARG, "aggf_make_whole: NULL pointer");
  if (rounds > 0 && !jumps) return fail(AGGF_ERR_ARG, "aggf_make_whole: rounds without jump tables");
  if (form == WH_LDS && N > lds_max)
    return fail(AGGF_ERR_ARG, "aggf_make_whole: the LDS form holds at most %d atoms, not %d", lds_max, N);
  if (form == WH_AUTO) form = N <= lds_max ? WH_LDS : WH_GLOBAL;
  if (form == WH_LDS) {
    const int rc = dtype == AGGF_F64 ? launch_whole_lds<double>(stream, X, T, N, parent, jumps, rounds, box, box_stride,
                                                                out, images)
                                     : launch_whole_lds<float>(stream, X, T, N, parent, jumps, rounds, box, box_stride,
                                                               out, images);
    if (rc != AGGF_OK) return rc;
  } else {
    if (!ws || ws_bytes < (size_t)ws_need) return fail(AGGF_ERR_WORKSPACE, "aggf_make_whole: workspace too small");
    if ((uintptr_t)ws % 4) return fail(AGGF_ERR_WORKSPACE, "aggf_make_whole: workspace is not element-aligned");
    if (dtype == AGGF_F64)
      launch_whole_global<double>(stream, X, T, N, parent, jumps, rounds, box, box_stride, out, images, ws);
    else
      launch_whole_global<float>(stream, X, T, N, parent, jumps, rounds, box, box_stride, out, images, ws);
  }
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}
