// K4: Gaussian-basis distance featuriser (gb_feat) and the featurised regression matrix,
// without ever materialising the one-hot (T, N, n_feat) feature tensor.
//
// Reference: qp/jaxfeat.py (gb_feat 20-184, gaussian_dist_basis 187-240, clipped_gauss
// 243-276, channel_allocate 279-368, gb_subfeat 371-464, gb_subfeat_jac 467-567),
// map/tools.py:63-104 (smear_map), qp/featlinearmap.py:361-369 (regression matrix) and
// 512-520 (map application).  Facts used: every atom of a constraint group is
// replaced by the group mean before the distance is taken, so all atoms of a channel share
// one distance r[t,ch] = |p[t,ch] - cg[t,c]| and one Gaussian row, and
//   feat[t,a,(ch,k)]  = [ch == channel(a)] * g_k(r[t,ch])
//   div [t,(ch,k),:]  = |ch| * g_k'(r[t,ch]) * (p[t,ch] - cg[t,c]) / r[t,ch]        (closed form of
//                       the reference's jacrev; cg is a constant of the differentiation)
//   R3[t,(ch,k),d]    = g_k(r) * Fg[t,ch,d] + kbt * div[t,(ch,k),d],  Fg = group force sums
// with g_k(r) = max(exp(-((r-c_k)/w)^2), clip) - clip.  The float32 arithmetic of the
// reference (JAX default) is kept for positions, distances and Gaussians.
//
// Box forms (gb_*_pbc_kernel; not in the reference): the displacement p[t,ch] - cg[t,c] is replaced by its minimum image
// under an orthorhombic box per frame (min_image, aggf_common.h; `box` (T, 3) with bstride 3, or (3,) with bstride 0, in
// the feature dtype), so r is the minimum-image distance and u its direction.  Group means and mapped sites are taken
// as given: they need whole groups and whole beads (K11).  A frame whose box is bad has NaN features (its Gaussian
// columns of the regression matrix, its row of the applied map) and the whole distance range.  Each pair of kernels
// shares one __device__ body; the open ones keep their names, arguments and bits.  gb_regmat_kernel has no box form.
//
// Cell forms (the same gb_*_pbc_kernel families, template argument CELL = CELL_TRI or CELL_NEAR beside CELL_BOX): the
// displacement is replaced by its brick image or its nearest image under a triclinic cell per frame (cell_image,
// aggf_common.h; `box` then holds the (T, 9) row-major cells in the feature dtype), with every convention of the box
// forms; a frame whose cell is bad by cell_good's rule is a frame whose box is bad.  The open and the box
// instantiations are the kernels they were, instruction for instruction.
#include "aggf_common.h"

namespace aggf {

// out[t,g,d] = sum (or mean: each term multiplied by 1/|g| first, like the smear matrix
// product) of X[t,a,d] over the atoms of group g
template <typename TIn, typename TO>
__global__ __launch_bounds__(256) void group_reduce_kernel(const TIn* __restrict__ X, int64_t T, int32_t N,
                                                           const int32_t* __restrict__ grp_ptr,
                                                           const int32_t* __restrict__ grp_atoms,
                                                           int32_t G, int mean, TO* __restrict__ out) {
  const int64_t row_in = (int64_t)N * 3, row_out = (int64_t)G * 3;
  for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
    const TIn* src = X + t * row_in;
    TO* dst = out + t * row_out;
    for (int e = threadIdx.x; e < (int)row_out; e += blockDim.x) {
      const int g = e / 3, d = e - 3 * g;
      const int b = grp_ptr[g], en = grp_ptr[g + 1];
      // mean weights are the float32 entries of the reference's smear matrix (map/tools.py:94-101), whatever TO
      const TO w = mean ? (TO)(1.0f / (float)(en - b)) : (TO)1;
      TO acc = 0;
      for (int j = b; j < en; ++j) acc += w * (TO)src[(int64_t)grp_atoms[j] * 3 + d];
      dst[e] = acc;
    }
  }
}

// TG = arithmetic type of positions, distances and Gaussians: float (the reference's JAX default; the default
// here) or double (opt-in `feature_dtype=np.float64` of gb_feat: product and float64 oracle then share arithmetic)
template <typename TG>
struct GbParams {
  const TG* centers;  // n_basis grid centres
  int32_t n_basis;
  TG width, clip;
};

__device__ __forceinline__ float gb_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double gb_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ float gb_exp(float x) { return expf(x); }
__device__ __forceinline__ double gb_exp(double x) { return exp(x); }
__device__ __forceinline__ float gb_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double gb_max(double a, double b) { return fmax(a, b); }

// arithmetic type of the products with the forces: NumPy promotion of (force dtype, feature dtype)
template <typename TF, typename TG>
struct GbProd { typedef double type; };
template <>
struct GbProd<float, float> { typedef float type; };

// A body shared by an open and a box kernel takes its grid-stride loop bounds from the kernel: read in the __global__
// function the launch dimensions compile to what they always did (inside a __device__ body the compiler no longer
// assumes whole workgroups and adds the partial-workgroup look-up to the open kernels' prologues)
#define GB_FIRST ((int64_t)blockIdx.x * blockDim.x + threadIdx.x)
#define GB_STEP ((int64_t)gridDim.x * blockDim.x)

// the box of one frame in a box form: lengths, their inverses (formed once per frame) and whether all three are good
template <typename TG>
struct GbCell {
  TG L[3], iL[3];
  bool ok;
};
template <typename TG>
__device__ __forceinline__ void gb_cell(const TG* __restrict__ box, int32_t bstride, int64_t t, GbCell<TG>& cell) {
  cell.ok = box_lengths(box + t * bstride, cell.L, cell.iL);
}
// the cell of one frame in a cell form (CELL_TRI, CELL_NEAR): the frame of its nine numbers (row t of a (T, 9) array;
// NaN throughout when it is bad by cell_good's rule) and whether it is good
template <typename TG>
struct GbTri {
  CellFrame<TG> h;
  bool ok;
};
template <typename TG>
__device__ __forceinline__ void gb_cell(const TG* __restrict__ cell9, int32_t, int64_t t, GbTri<TG>& cell) {
  cell.ok = cell_frame(cell9 + t * 9, cell.h);
}
// what a body of form CELL holds of a frame (the open form holds nothing: the type only has to exist)
template <typename TG, int CELL>
struct GbFrameOf { typedef GbCell<TG> type; };
template <typename TG>
struct GbFrameOf<TG, CELL_TRI> { typedef GbTri<TG> type; };
template <typename TG>
struct GbFrameOf<TG, CELL_NEAR> { typedef GbTri<TG> type; };

// distance, unit vector and Gaussian row of channel ch at frame t; CELL_BOX: of the minimum image under `cell`,
// CELL_TRI / CELL_NEAR: of the brick / nearest image under it (cell_image, aggf_common.h)
template <typename TG, int CELL = CELL_OPEN>
__device__ __forceinline__ void gb_geometry(const TG* __restrict__ Pg, const TG* __restrict__ cg,
                                            int64_t t, int32_t G, int32_t ch, int32_t n_cg, int32_t site,
                                            TG& r, TG u[3], const typename GbFrameOf<TG, CELL>::type* cell = nullptr) {
  // no fused multiply-add here: whether dx*dx + dy*dy + dz*dz contracts is otherwise decided per kernel the function is
  // inlined into, and the kernels that evaluate a feature (regression matrix, constraint rows, the two application
  // kernels) must agree on it to the last bit -- as the reference's NumPy/JAX float32 arithmetic does
#pragma clang fp contract(off)
  const TG* p = Pg + (t * G + ch) * 3;
  const TG* c = cg + (t * n_cg + site) * 3;
  TG dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
  if constexpr (CELL == CELL_BOX) {
    dx = min_image(dx, cell->L[0], cell->iL[0]);
    dy = min_image(dy, cell->L[1], cell->iL[1]);
    dz = min_image(dz, cell->L[2], cell->iL[2]);
  } else if constexpr (CELL != CELL_OPEN) {
    cell_image<CELL>(dx, dy, dz, cell->h);
  }
  r = gb_sqrt(dx * dx + dy * dy + dz * dz);
  u[0] = dx / r;  // NaN at r == 0, like the gradient of jnp.linalg.norm
  u[1] = dy / r;
  u[2] = dz / r;
}

template <typename TG>
__device__ __forceinline__ void gb_gauss(const GbParams<TG>& gp, TG r, int k, TG& g, TG& dg) {
#pragma clang fp contract(off)
  const TG arg = (r - gp.centers[k]) / gp.width;
  const TG raw = gb_exp(-(arg * arg));
  g = gb_max(raw, gp.clip) - gp.clip;
  dg = raw > gp.clip ? (TG)-2 * arg / gp.width * raw : (TG)0;
}
// (the clip turns a NaN distance into a zero feature: a frame whose box is bad says so instead)
template <typename TG, typename TC>
__device__ __forceinline__ void gb_bad_cell(const TC& cell, TG& g, TG& dg) {
  if (!cell.ok) g = dg = (TG)__builtin_nan("");
}

// compact per-channel features: gauss[t,ch,k], grad[t,ch,k,:] = |ch| g_k'(r) u
template <typename TG, int CELL>
__device__ __forceinline__ void gb_channels_body(const TG* __restrict__ Pg, const TG* __restrict__ cg, int64_t T,
                                                 int32_t G, int32_t n_cg, int32_t site,
                                                 const float* __restrict__ sizes, int32_t n_ch, GbParams<TG> gp,
                                                 const TG* __restrict__ box, int32_t bstride, TG* __restrict__ gauss,
                                                 TG* __restrict__ grad, int64_t first, int64_t step) {
  const int64_t total = T * n_ch;
  for (int64_t i = first; i < total; i += step) {
    const int64_t t = i / n_ch;
    const int ch = (int)(i - t * n_ch);
    TG r, u[3];
    typename GbFrameOf<TG, CELL>::type cell;
    if (CELL != CELL_OPEN) gb_cell(box, bstride, t, cell);
    gb_geometry<TG, CELL>(Pg, cg, t, G, ch, n_cg, site, r, u, &cell);
    const TG m = (TG)sizes[ch];
    for (int k = 0; k < gp.n_basis; ++k) {
      TG g, dg;
      gb_gauss(gp, r, k, g, dg);
      if (CELL != CELL_OPEN) gb_bad_cell(cell, g, dg);
      const int64_t o = i * gp.n_basis + k;
      gauss[o] = g;
      grad[o * 3 + 0] = m * dg * u[0];
      grad[o * 3 + 1] = m * dg * u[1];
      grad[o * 3 + 2] = m * dg * u[2];
    }
  }
}

template <typename TG>
__global__ __launch_bounds__(256) void gb_channels_kernel(const TG* __restrict__ Pg,
                                                          const TG* __restrict__ cg, int64_t T, int32_t G,
                                                          int32_t n_cg, int32_t site,
                                                          const float* __restrict__ sizes, int32_t n_ch,
                                                          GbParams<TG> gp, TG* __restrict__ gauss,
                                                          TG* __restrict__ grad) {
  gb_channels_body<TG, CELL_OPEN>(Pg, cg, T, G, n_cg, site, sizes, n_ch, gp, nullptr, 0, gauss, grad, GB_FIRST, GB_STEP);
}

template <typename TG, int CELL>
__global__ __launch_bounds__(256) void gb_channels_pbc_kernel(const TG* __restrict__ Pg,
                                                              const TG* __restrict__ cg, int64_t T, int32_t G,
                                                              int32_t n_cg, int32_t site,
                                                              const float* __restrict__ sizes, int32_t n_ch,
                                                              GbParams<TG> gp, const TG* __restrict__ box,
                                                              int32_t bstride, TG* __restrict__ gauss,
                                                              TG* __restrict__ grad) {
  gb_channels_body<TG, CELL>(Pg, cg, T, G, n_cg, site, sizes, n_ch, gp, box, bstride, gauss, grad, GB_FIRST, GB_STEP);
}

// R3 (T, ld_feat, 3): columns [0, n_id) = group force sums (id_feat block, optional), then
// n_ch * n_basis Gaussian columns; columns up to ld_feat are left untouched (ignored by K1).
// TO = storage type of R3: the products are formed in TF (the reference's arithmetic) and only then widened,
// so a float64 R3 -- K1's in-place operand for float64 products -- holds exactly the float32 matrix.
template <typename TF, typename TG, typename TO>
__global__ __launch_bounds__(256) void gb_regmat_kernel(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                        const TG* __restrict__ cg, int64_t T, int32_t G,
                                                        int32_t n_cg, int32_t site,
                                                        const float* __restrict__ sizes, int32_t n_id,
                                                        int32_t n_ch, GbParams<TG> gp, double kbt_d, int32_t ld_feat,
                                                        TO* __restrict__ R3) {
  typedef typename GbProd<TF, TG>::type TP;
  const TP kbt = (TP)kbt_d;
  const int per_frame = n_id + n_ch;  // work items per frame: id columns, then channels
  const int64_t total = T * per_frame;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / per_frame;
    const int j = (int)(i - t * per_frame);
    TO* row = R3 + t * (int64_t)ld_feat * 3;
    if (j < n_id) {
      const TF* f = Fg + (t * G + j) * 3;
      row[j * 3 + 0] = (TO)f[0];
      row[j * 3 + 1] = (TO)f[1];
      row[j * 3 + 2] = (TO)f[2];
      continue;
    }
    const int ch = j - n_id;
    TG r, u[3];
    gb_geometry(Pg, cg, t, G, ch, n_cg, site, r, u);
    const TF* f = Fg + (t * G + ch) * 3;
    const TP f0 = (TP)f[0], f1 = (TP)f[1], f2 = (TP)f[2];
    const TG m = (TG)sizes[ch];
    TO* o = row + ((int64_t)n_id + (int64_t)ch * gp.n_basis) * 3;
    for (int k = 0; k < gp.n_basis; ++k) {
      TG g, dg;
      gb_gauss(gp, r, k, g, dg);
      const TG s = m * dg;
      o[k * 3 + 0] = (TO)((TP)g * f0 + kbt * (TP)(s * u[0]));
      o[k * 3 + 1] = (TO)((TP)g * f1 + kbt * (TP)(s * u[1]));
      o[k * 3 + 2] = (TO)((TP)g * f2 + kbt * (TP)(s * u[2]));
    }
  }
}

// ---------------------------------------------------------------------------
// Column compaction of the fused fit.  A clipped Gaussian column (ch, k) is identically zero over the
// whole trajectory when the channel never comes within w sqrt(ln(1/clip)) of centre c_k (the point of a
// cut-off basis); such a column contributes a zero row/column to P and zeros to every constraint row, so
// its coefficient in the minimiser is exactly 0 (l2 > 0) and it can be left out of the Gram matrix and of
// the solve.  gb_range_kernel finds, per (site, channel), the range of distances over the frames.

__device__ __forceinline__ void atomic_min_pos_float(float* addr, float v) {
  atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));  // order-preserving for v >= 0
}
__device__ __forceinline__ void atomic_max_pos_float(float* addr, float v) {
  atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
}

// rmin/rmax (n_cg, G) must be initialised to +inf / 0.  grid = (channel blocks, sites, frame slices).
// A NaN distance (non-finite coordinates, under a box a bad length too) marks the channel as spanning everything.
// CELL_BOX / CELL_TRI / CELL_NEAR: the range of the image distances, which is what those forms of the feature kernels
// evaluate (`box`: (T, 3) or (3,) lengths by bstride, or the (T, 9) rows of a cell).
__device__ __forceinline__ float gb_range_sq(float dx, float dy, float dz) {
#pragma clang fp contract(off)
  return __builtin_fmaf(dy, dy, dx * dx) + dz * dz;
}
template <int CELL>
__device__ __forceinline__ void gb_range_body(const float* __restrict__ Pg, const float* __restrict__ cg, int64_t T,
                                              int32_t G, int32_t n_cg, int32_t n_ch, const float* __restrict__ box,
                                              int32_t bstride, float* __restrict__ rmin, float* __restrict__ rmax) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  const int site = blockIdx.y;
  if (ch >= n_ch) return;
  float lo = INFINITY, hi = 0.0f;
  for (int64_t t = blockIdx.z; t < T; t += gridDim.z) {
    const float* p = Pg + (t * G + ch) * 3;
    const float* c = cg + (t * n_cg + site) * 3;
    float dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
    if constexpr (CELL == CELL_BOX) {
      float L[3], iL[3];
      box_lengths(box + t * bstride, L, iL);
      dx = min_image(dx, L[0], iL[0]), dy = min_image(dy, L[1], iL[1]), dz = min_image(dz, L[2], iL[2]);
    } else if constexpr (CELL != CELL_OPEN) {
      CellFrame<float> h;
      cell_frame(box + t * 9, h);  // a bad frame: NaN throughout, so r is NaN and the channel spans everything
      cell_image<CELL>(dx, dy, dz, h);
    }
    // (the open and the box form leave the contraction of this sum to the compiler, which has always formed
    // fma(dy, dy, dx dx) + dz dz for both; the cell forms say so, or a diagonal cell would not give the box form's bits)
    const float r = sqrtf(CELL >= CELL_TRI ? gb_range_sq(dx, dy, dz) : dx * dx + dy * dy + dz * dz);
    if (!(r == r)) { lo = 0.0f; hi = INFINITY; }
    lo = fminf(lo, r);
    hi = fmaxf(hi, r);
  }
  atomic_min_pos_float(rmin + (int64_t)site * G + ch, lo);
  atomic_max_pos_float(rmax + (int64_t)site * G + ch, hi);
}

__global__ __launch_bounds__(256) void gb_range_kernel(const float* __restrict__ Pg, const float* __restrict__ cg,
                                                       int64_t T, int32_t G, int32_t n_cg, int32_t n_ch,
                                                       float* __restrict__ rmin, float* __restrict__ rmax) {
  gb_range_body<CELL_OPEN>(Pg, cg, T, G, n_cg, n_ch, nullptr, 0, rmin, rmax);
}

template <int CELL>
__global__ __launch_bounds__(256) void gb_range_pbc_kernel(const float* __restrict__ Pg, const float* __restrict__ cg,
                                                           int64_t T, int32_t G, int32_t n_cg, int32_t n_ch,
                                                           const float* __restrict__ box, int32_t bstride,
                                                           float* __restrict__ rmin, float* __restrict__ rmax) {
  gb_range_body<CELL>(Pg, cg, T, G, n_cg, n_ch, box, bstride, rmin, rmax);
}

// An entry g f + kbt (s u) of the regression matrix is one multiply-add and one product rounded on its own, and which of
// the two products the multiply-add absorbs is left to the compiler in the open and the box form (see the note on the
// NaN store below).  It has decided per instantiation and per COMPONENT, the same way in both: fma(g, f, kbt su) where
// the table says g_first, fma(kbt, su, g f) elsewhere.  The cell forms write that decision out, so that a diagonal cell
// gives the box form's bits and a lattice shift is undone to the open form's bits, whichever way the search of the
// nearest form moves the compiler.  (tests/test_gpu_feat_cell.py holds the cell forms to the other two bit for bit:
// if a compiler decides otherwise for those, this table follows.)
template <typename TF, typename TG, typename TO>
struct GbFuse { static constexpr bool g_first[3] = {true, false, false}; };  // float products widened; double features
template <>
struct GbFuse<float, float, float> { static constexpr bool g_first[3] = {false, false, false}; };
template <>
struct GbFuse<double, float, double> { static constexpr bool g_first[3] = {true, true, false}; };
template <>
struct GbFuse<double, double, double> { static constexpr bool g_first[3] = {true, true, false}; };
template <typename TP>
__device__ __forceinline__ TP gb_entry(bool g_first, TP g, TP f, TP kbt, TP su) {
#pragma clang fp contract(off)
  return g_first ? cell_fma(g, f, kbt * su) : cell_fma(kbt, su, g * f);
}

// Compact regression matrix: column j < n_id = group force sums; column n_id + j = the Gaussian column
// cols[j] = ch * n_basis + k (only the listed ones).  One thread per (frame, compact column): consecutive
// threads write consecutive 3-vectors (coalesced), the distance of a channel is recomputed per listed k.
template <typename TF, typename TG, typename TO, int CELL>
__device__ __forceinline__ void gb_regmat_cols_body(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                    const TG* __restrict__ cg, int64_t T, int32_t G, int32_t n_cg,
                                                    int32_t site, const float* __restrict__ sizes, int32_t n_id,
                                                    const int32_t* __restrict__ cols, int32_t n_cols, GbParams<TG> gp,
                                                    double kbt_d, int32_t ld_feat, const TG* __restrict__ box,
                                                    int32_t bstride, TO* __restrict__ R3, int64_t first,
                                                    int64_t step) {
  typedef typename GbProd<TF, TG>::type TP;
  const TP kbt = (TP)kbt_d;
  const int per_frame = n_id + n_cols;
  const int64_t total = T * per_frame;
  for (int64_t i = first; i < total; i += step) {
    const int64_t t = i / per_frame;
    const int j = (int)(i - t * per_frame);
    TO* o = R3 + (t * (int64_t)ld_feat + j) * 3;
    if (j < n_id) {
      const TF* f = Fg + (t * G + j) * 3;
      o[0] = (TO)f[0];
      o[1] = (TO)f[1];
      o[2] = (TO)f[2];
      continue;
    }
    const int full = cols[j - n_id];
    const int ch = full / gp.n_basis, k = full - ch * gp.n_basis;
    TG r, u[3], g, dg;
    typename GbFrameOf<TG, CELL>::type cell;
    if (CELL != CELL_OPEN) gb_cell(box, bstride, t, cell);
    gb_geometry<TG, CELL>(Pg, cg, t, G, ch, n_cg, site, r, u, &cell);
    gb_gauss(gp, r, k, g, dg);
    const TF* f = Fg + (t * G + ch) * 3;
    const TG s = (TG)sizes[ch] * dg;
    if constexpr (CELL >= CELL_TRI) {
      typedef GbFuse<TF, TG, TO> FU;
      o[0] = (TO)gb_entry<TP>(FU::g_first[0], (TP)g, (TP)f[0], kbt, (TP)(s * u[0]));
      o[1] = (TO)gb_entry<TP>(FU::g_first[1], (TP)g, (TP)f[1], kbt, (TP)(s * u[1]));
      o[2] = (TO)gb_entry<TP>(FU::g_first[2], (TP)g, (TP)f[2], kbt, (TP)(s * u[2]));
    } else {
      o[0] = (TO)((TP)g * (TP)f[0] + kbt * (TP)(s * u[0]));
      o[1] = (TO)((TP)g * (TP)f[1] + kbt * (TP)(s * u[1]));
      o[2] = (TO)((TP)g * (TP)f[2] + kbt * (TP)(s * u[2]));
    }
    // (a bad box says so AFTER the products: a select in front of them changes which of the multiply-adds the compiler
    // fuses, and the box form must round as the open one does)
    if (CELL != CELL_OPEN && !cell.ok) o[0] = o[1] = o[2] = (TO)__builtin_nan("");
  }
}

template <typename TF, typename TG, typename TO>
__global__ __launch_bounds__(256) void gb_regmat_cols_kernel(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                             const TG* __restrict__ cg, int64_t T, int32_t G,
                                                             int32_t n_cg, int32_t site,
                                                             const float* __restrict__ sizes, int32_t n_id,
                                                             const int32_t* __restrict__ cols, int32_t n_cols,
                                                             GbParams<TG> gp, double kbt_d, int32_t ld_feat,
                                                             TO* __restrict__ R3) {
  gb_regmat_cols_body<TF, TG, TO, CELL_OPEN>(Fg, Pg, cg, T, G, n_cg, site, sizes, n_id, cols, n_cols, gp, kbt_d, ld_feat,
                                         nullptr, 0, R3, GB_FIRST, GB_STEP);
}

template <typename TF, typename TG, typename TO, int CELL>
__global__ __launch_bounds__(256) void gb_regmat_cols_pbc_kernel(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                                 const TG* __restrict__ cg, int64_t T, int32_t G,
                                                                 int32_t n_cg, int32_t site,
                                                                 const float* __restrict__ sizes, int32_t n_id,
                                                                 const int32_t* __restrict__ cols, int32_t n_cols,
                                                                 GbParams<TG> gp, double kbt_d, int32_t ld_feat,
                                                                 const TG* __restrict__ box, int32_t bstride,
                                                                 TO* __restrict__ R3) {
  gb_regmat_cols_body<TF, TG, TO, CELL>(Fg, Pg, cg, T, G, n_cg, site, sizes, n_id, cols, n_cols, gp, kbt_d, ld_feat,
                                        box, bstride, R3, GB_FIRST, GB_STEP);
}

// CLAMap application of the [id | gb] feature-linear map (featlinearmap.py:512-520,
// map/core.py:428-430): out[t,c,:] = sum_f coef[c,f] * (feat_c[t]' F[t] + div_c[t])[f,:]
// -- the divergence enters WITHOUT kbt, exactly as in the reference's trans_f.
// One wave per (block of GB_FR frames, site); lanes stride over id columns and channels.  A lane's coefficients of a
// channel are read ONCE for the GB_FR frames (per frame they were 43 KB of L1/L2 reads per (frame, site) at BASELINE
// config 4 -- 55 GB per application, the kernel's bound: 16 ms), and a channel none of whose columns the fit kept
// costs neither the distance nor the expf.  Per frame the terms are added in the same order as one frame at a time.
constexpr int GB_FR = 4;
constexpr int GB_CB = 8;  // coefficients of a channel held in registers (basis functions beyond: read in the loop)

// The wave's index is the same in every lane, which the compiler cannot prove of threadIdx.x >> 6.  The cell forms say
// so: the frames' cells are then read with scalar loads, once per wave and not once per lane.  (Reads only; every
// store of these kernels is a vector store.)
__device__ __forceinline__ int64_t gb_wave_uniform(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Under a box or a cell: those of the GB_FR frames are read once per (frame block, site), before the channels; a frame whose box is
// bad gets a NaN row whatever its coefficients.
template <typename TF, typename TG, int CELL>
__device__ __forceinline__ void gb_apply_body(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                              const TG* __restrict__ cg, int64_t T, int32_t G, int32_t n_cg,
                                              const float* __restrict__ sizes, int32_t n_id, int32_t n_ch,
                                              GbParams<TG> gp, const double* __restrict__ coef, int32_t n_feat,
                                              const TG* __restrict__ box, int32_t bstride, double* __restrict__ out,
                                              int64_t first, int64_t step) {
  typedef typename GbProd<TF, TG>::type TP;
  const int lane = threadIdx.x & 63;
  const int64_t wid = CELL >= CELL_TRI ? gb_wave_uniform(first >> 6) : first >> 6;
  const int64_t nw = step >> 6;
  const int64_t n_blk = (T + GB_FR - 1) / GB_FR;
  for (int64_t i = wid; i < n_blk * n_cg; i += nw) {
    const int64_t blk = i / n_cg;  // consecutive waves: the same frames, the sites one after the other
    const int site = (int)(i - blk * n_cg);
    const int64_t t0 = blk * GB_FR;
    const int nf = T - t0 < GB_FR ? (int)(T - t0) : GB_FR;
    const double* cf = coef + (int64_t)site * n_feat;
    double acc[GB_FR][3];
#pragma unroll
    for (int f = 0; f < GB_FR; ++f) acc[f][0] = acc[f][1] = acc[f][2] = 0.0;
    typename GbFrameOf<TG, CELL>::type cell[GB_FR];
    if (CELL != CELL_OPEN) {
#pragma unroll
      for (int f = 0; f < GB_FR; ++f)
        if (f < nf) gb_cell(box, bstride, t0 + f, cell[f]);
    }
    for (int g = lane; g < n_id; g += 64) {
      const double c = cf[g];
#pragma unroll
      for (int f = 0; f < GB_FR; ++f) {
        if (f < nf) {
          const TF* fv = Fg + ((t0 + f) * G + g) * 3;
          acc[f][0] += c * (double)fv[0];
          acc[f][1] += c * (double)fv[1];
          acc[f][2] += c * (double)fv[2];
        }
      }
    }
    for (int ch = lane; ch < n_ch; ch += 64) {
      const double* cc = cf + n_id + (int64_t)ch * gp.n_basis;
      double cb[GB_CB];  // the loads are issued together: one memory latency per channel, not one per basis function
#pragma unroll
      for (int k = 0; k < GB_CB; ++k) cb[k] = k < gp.n_basis ? cc[k] : 0.0;
      bool any = false;
#pragma unroll
      for (int k = 0; k < GB_CB; ++k) any |= cb[k] != 0.0;
      for (int k = GB_CB; k < gp.n_basis; ++k) any |= cc[k] != 0.0;
      if (!any) continue;  // no column of this channel was kept by the fit (identically zero over the training frames)
      TG r[GB_FR], u[GB_FR][3];
      TP fr[GB_FR][3];
#pragma unroll
      for (int f = 0; f < GB_FR; ++f) {
        if (f < nf) {
          gb_geometry<TG, CELL>(Pg, cg, t0 + f, G, ch, n_cg, site, r[f], u[f], &cell[f]);
          const TF* fv = Fg + ((t0 + f) * G + ch) * 3;
          fr[f][0] = (TP)fv[0];
          fr[f][1] = (TP)fv[1];
          fr[f][2] = (TP)fv[2];
        }
      }
      const TG m = (TG)sizes[ch];
      auto add_basis = [&](int k, double c) {
        if (c == 0.0) return;  // a column the fit left out: no expf
#pragma unroll
        for (int f = 0; f < GB_FR; ++f) {
          if (f < nf) {
            TG g, dg;
            gb_gauss(gp, r[f], k, g, dg);
            const TG s = m * dg;
            acc[f][0] += c * ((double)((TP)g * fr[f][0]) + (double)(s * u[f][0]));
            acc[f][1] += c * ((double)((TP)g * fr[f][1]) + (double)(s * u[f][1]));
            acc[f][2] += c * ((double)((TP)g * fr[f][2]) + (double)(s * u[f][2]));
          }
        }
      };
#pragma unroll
      for (int k = 0; k < GB_CB; ++k)
        if (k < gp.n_basis) add_basis(k, cb[k]);
      for (int k = GB_CB; k < gp.n_basis; ++k) add_basis(k, cc[k]);
    }
#pragma unroll
    for (int f = 0; f < GB_FR; ++f) {
      double a0 = acc[f][0], a1 = acc[f][1], a2 = acc[f][2];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_down(a0, off, 64);
        a1 += __shfl_down(a1, off, 64);
        a2 += __shfl_down(a2, off, 64);
      }
      if (lane == 0 && f < nf) {
        if (CELL != CELL_OPEN && !cell[f].ok) a0 = a1 = a2 = __builtin_nan("");
        double* o = out + ((t0 + f) * n_cg + site) * 3;
        o[0] = a0;
        o[1] = a1;
        o[2] = a2;
      }
    }
  }
}

template <typename TF, typename TG>
__global__ __launch_bounds__(256) void gb_apply_kernel(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                       const TG* __restrict__ cg, int64_t T, int32_t G,
                                                       int32_t n_cg, const float* __restrict__ sizes,
                                                       int32_t n_id, int32_t n_ch, GbParams<TG> gp,
                                                       const double* __restrict__ coef, int32_t n_feat,
                                                       double* __restrict__ out) {
  gb_apply_body<TF, TG, CELL_OPEN>(Fg, Pg, cg, T, G, n_cg, sizes, n_id, n_ch, gp, coef, n_feat, nullptr, 0, out, GB_FIRST,
                               GB_STEP);
}

template <typename TF, typename TG, int CELL>
__global__ __launch_bounds__(256) void gb_apply_pbc_kernel(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                           const TG* __restrict__ cg, int64_t T, int32_t G,
                                                           int32_t n_cg, const float* __restrict__ sizes,
                                                           int32_t n_id, int32_t n_ch, GbParams<TG> gp,
                                                           const double* __restrict__ coef, int32_t n_feat,
                                                           const TG* __restrict__ box, int32_t bstride,
                                                           double* __restrict__ out) {
  gb_apply_body<TF, TG, CELL>(Fg, Pg, cg, T, G, n_cg, sizes, n_id, n_ch, gp, coef, n_feat, box, bstride, out, GB_FIRST,
                              GB_STEP);
}

// The same map from a COMPACT coefficient list: the fit keeps ~a third of the Gaussian columns (2.1 of 8 basis
// functions per channel at BASELINE config 4) and different ones for every channel, so in gb_apply_kernel -- lane =
// channel -- nearly every basis function is executed by the wave for the few lanes that need it.  Here lane = one kept
// column (ch, k) of the site: no idle lanes; the distance of a channel is recomputed for each of its kept columns
// (cheaper than the expf it replaces).  col_ptr[n_cg + 1] / col_idx (ch * n_basis + k) / col_val: the non-zero
// Gaussian coefficients per site; coef_id (n_cg, n_id): the id block, dense.
template <typename TF, typename TG, int CELL>
__device__ __forceinline__ void gb_apply_cols_body(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                   const TG* __restrict__ cg, int64_t T, int32_t G, int32_t n_cg,
                                                   const float* __restrict__ sizes, int32_t n_id,
                                                   const double* __restrict__ coef_id,
                                                   const int32_t* __restrict__ col_ptr,
                                                   const int32_t* __restrict__ col_idx,
                                                   const double* __restrict__ col_val, GbParams<TG> gp,
                                                   const TG* __restrict__ box, int32_t bstride,
                                                   double* __restrict__ out, int64_t first, int64_t step) {
  typedef typename GbProd<TF, TG>::type TP;
  const int lane = threadIdx.x & 63;
  const int64_t wid = CELL >= CELL_TRI ? gb_wave_uniform(first >> 6) : first >> 6;
  const int64_t nw = step >> 6;
  const int64_t n_blk = (T + GB_FR - 1) / GB_FR;
  for (int64_t i = wid; i < n_blk * n_cg; i += nw) {
    const int64_t blk = i / n_cg;
    const int site = (int)(i - blk * n_cg);
    const int64_t t0 = blk * GB_FR;
    const int nf = T - t0 < GB_FR ? (int)(T - t0) : GB_FR;
    double acc[GB_FR][3];
#pragma unroll
    for (int f = 0; f < GB_FR; ++f) acc[f][0] = acc[f][1] = acc[f][2] = 0.0;
    typename GbFrameOf<TG, CELL>::type cell[GB_FR];
    if (CELL != CELL_OPEN) {
#pragma unroll
      for (int f = 0; f < GB_FR; ++f)
        if (f < nf) gb_cell(box, bstride, t0 + f, cell[f]);
    }
    for (int g = lane; g < n_id; g += 64) {
      const double c = coef_id[(int64_t)site * n_id + g];
#pragma unroll
      for (int f = 0; f < GB_FR; ++f) {
        if (f < nf) {
          const TF* fv = Fg + ((t0 + f) * G + g) * 3;
          acc[f][0] += c * (double)fv[0];
          acc[f][1] += c * (double)fv[1];
          acc[f][2] += c * (double)fv[2];
        }
      }
    }
    for (int e = col_ptr[site] + lane; e < col_ptr[site + 1]; e += 64) {
      const int full = col_idx[e];
      const int ch = full / gp.n_basis, k = full - ch * gp.n_basis;
      const double c = col_val[e];
      const TG m = (TG)sizes[ch];
#pragma unroll
      for (int f = 0; f < GB_FR; ++f) {
        if (f < nf) {
          TG r, u[3], g, dg;
          gb_geometry<TG, CELL>(Pg, cg, t0 + f, G, ch, n_cg, site, r, u, &cell[f]);
          gb_gauss(gp, r, k, g, dg);
          const TF* fv = Fg + ((t0 + f) * G + ch) * 3;
          const TG sd = m * dg;
          acc[f][0] += c * ((double)((TP)g * (TP)fv[0]) + (double)(sd * u[0]));
          acc[f][1] += c * ((double)((TP)g * (TP)fv[1]) + (double)(sd * u[1]));
          acc[f][2] += c * ((double)((TP)g * (TP)fv[2]) + (double)(sd * u[2]));
        }
      }
    }
#pragma unroll
    for (int f = 0; f < GB_FR; ++f) {
      double a0 = acc[f][0], a1 = acc[f][1], a2 = acc[f][2];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_down(a0, off, 64);
        a1 += __shfl_down(a1, off, 64);
        a2 += __shfl_down(a2, off, 64);
      }
      if (lane == 0 && f < nf) {
        if (CELL != CELL_OPEN && !cell[f].ok) a0 = a1 = a2 = __builtin_nan("");
        double* o = out + ((t0 + f) * n_cg + site) * 3;
        o[0] = a0;
        o[1] = a1;
        o[2] = a2;
      }
    }
  }
}

template <typename TF, typename TG>
__global__ __launch_bounds__(256) void gb_apply_cols_kernel(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                            const TG* __restrict__ cg, int64_t T, int32_t G,
                                                            int32_t n_cg, const float* __restrict__ sizes,
                                                            int32_t n_id, const double* __restrict__ coef_id,
                                                            const int32_t* __restrict__ col_ptr,
                                                            const int32_t* __restrict__ col_idx,
                                                            const double* __restrict__ col_val, GbParams<TG> gp,
                                                            double* __restrict__ out) {
  gb_apply_cols_body<TF, TG, CELL_OPEN>(Fg, Pg, cg, T, G, n_cg, sizes, n_id, coef_id, col_ptr, col_idx, col_val, gp, nullptr,
                                    0, out, GB_FIRST, GB_STEP);
}

template <typename TF, typename TG, int CELL>
__global__ __launch_bounds__(256) void gb_apply_cols_pbc_kernel(const TF* __restrict__ Fg, const TG* __restrict__ Pg,
                                                                const TG* __restrict__ cg, int64_t T, int32_t G,
                                                                int32_t n_cg, const float* __restrict__ sizes,
                                                                int32_t n_id, const double* __restrict__ coef_id,
                                                                const int32_t* __restrict__ col_ptr,
                                                                const int32_t* __restrict__ col_idx,
                                                                const double* __restrict__ col_val, GbParams<TG> gp,
                                                                const TG* __restrict__ box, int32_t bstride,
                                                                double* __restrict__ out) {
  gb_apply_cols_body<TF, TG, CELL>(Fg, Pg, cg, T, G, n_cg, sizes, n_id, coef_id, col_ptr, col_idx, col_val, gp, box,
                                   bstride, out, GB_FIRST, GB_STEP);
}

static inline dim3 feat_grid(int64_t n) {
  int64_t g = ceil_div(n, 256);
  if (g > 16384) g = 16384;
  if (g < 1) g = 1;
  return dim3((unsigned)g);
}

static int check_gb(const void* centers, int32_t n_basis, double width) {
  if (!centers || n_basis <= 0 || n_basis > 64) return fail(AGGF_ERR_ARG, "gb_feat: bad n_basis / centres");
  if (!(width > 0.0)) return fail(AGGF_ERR_ARG, "gb_feat: width must be positive");
  return AGGF_OK;
}

// the form a launcher runs: open without a box, else by `images` (GB_BOX: lengths; the selector of a _cell entry)
constexpr int GB_BOX = -1;
static int check_gb_cell(const char* who, const void* cell, int images) {
  if (!cell) return fail(AGGF_ERR_ARG, "%s: NULL cell", who);
  if (images != AGGF_IMAGES_BRICK && images != AGGF_IMAGES_NEAREST)
    return fail(AGGF_ERR_ARG, "%s: images %d is neither AGGF_IMAGES_BRICK nor AGGF_IMAGES_NEAREST", who, images);
  return AGGF_OK;
}
// one launch line for the three forms under a box: KERNEL(...) takes the form as its last template argument
#define AGGF_GB_FORMS(images, LAUNCH_OF)                              \
  do {                                                                \
    if ((images) == GB_BOX) { LAUNCH_OF(CELL_BOX); }                  \
    else if ((images) == AGGF_IMAGES_NEAREST) { LAUNCH_OF(CELL_NEAR); } \
    else { LAUNCH_OF(CELL_TRI); }                                     \
  } while (0)

// the box of a box form: (T, 3) or (3,) in the feature dtype
static int check_gb_box(const char* who, const void* box, int32_t box_stride) {
  if (!box) return fail(AGGF_ERR_ARG, "%s: NULL box", who);
  if (box_stride != 0 && box_stride != 3) return fail(AGGF_ERR_ARG, "%s: box_stride %d is neither 0 nor 3", who, box_stride);
  return AGGF_OK;
}

}  // namespace aggf

using namespace aggf;

extern "C" int aggf_group_reduce(const void* X, int64_t T, int32_t N, int in_dtype,
                                 const int32_t* grp_ptr, const int32_t* grp_atoms, int32_t n_groups,
                                 int mean, int out_dtype, void* out, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!X || !grp_ptr || !grp_atoms || !out) return fail(AGGF_ERR_ARG, "aggf_group_reduce: NULL pointer");
  if (T <= 0 || N <= 0 || n_groups <= 0) return fail(AGGF_ERR_ARG, "aggf_group_reduce: empty problem");
  const dim3 grid((unsigned)(T < 8192 ? T : 8192)), block(256);
  if (in_dtype == AGGF_F32 && out_dtype == AGGF_F32)
    AGGF_LAUNCH((group_reduce_kernel<float, float>), grid, block, 0, stream, (const float*)X, T, N, grp_ptr, grp_atoms, n_groups, mean, (float*)out);
  else if (in_dtype == AGGF_F64 && out_dtype == AGGF_F64)
    AGGF_LAUNCH((group_reduce_kernel<double, double>), grid, block, 0, stream, (const double*)X, T, N, grp_ptr, grp_atoms, n_groups, mean, (double*)out);
  else if (in_dtype == AGGF_F64 && out_dtype == AGGF_F32)
    AGGF_LAUNCH((group_reduce_kernel<double, float>), grid, block, 0, stream, (const double*)X, T, N, grp_ptr, grp_atoms, n_groups, mean, (float*)out);
  else if (in_dtype == AGGF_F32 && out_dtype == AGGF_F64)
    AGGF_LAUNCH((group_reduce_kernel<float, double>), grid, block, 0, stream, (const float*)X, T, N, grp_ptr, grp_atoms, n_groups, mean, (double*)out);
  else
    return fail(AGGF_ERR_ARG, "aggf_group_reduce: bad dtype");
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

// every K4 entry point below, open (box NULL) or under a box: one validation and one launch plan for both
static int gb_channels(const char* who, const void* Pg, const void* cg, int g_dtype, int64_t T, int32_t G, int32_t n_cg,
                       int32_t site, const float* sizes, int32_t n_ch, const void* centers, int32_t n_basis,
                       double width, double clip, const void* box, int32_t bstride, int images, void* gauss,
                       void* grad, hipStream_t stream) {
  if (!Pg || !cg || !sizes || !gauss || !grad) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (T <= 0 || G <= 0 || n_ch <= 0 || n_ch > G || site < 0 || site >= n_cg)
    return fail(AGGF_ERR_ARG, "%s: bad shape", who);
  int rc = check_gb(centers, n_basis, width);
  if (rc) return rc;
  if (g_dtype == AGGF_F32) {
    GbParams<float> gp{(const float*)centers, n_basis, (float)width, (float)clip};
#define GB_CHANNELS_OF(FORM) AGGF_LAUNCH((gb_channels_pbc_kernel<TG, FORM>), feat_grid(T * n_ch), dim3(256), 0, stream, (const TG*)Pg, (const TG*)cg, T, G, n_cg, site, sizes, n_ch, gp, (const TG*)box, bstride, (TG*)gauss, (TG*)grad)
    typedef float TG;
    if (box)
      AGGF_GB_FORMS(images, GB_CHANNELS_OF);
    else
      AGGF_LAUNCH(gb_channels_kernel<float>, feat_grid(T * n_ch), dim3(256), 0, stream, (const float*)Pg, (const float*)cg, T, G, n_cg, site, sizes, n_ch, gp, (float*)gauss, (float*)grad);
  } else if (g_dtype == AGGF_F64) {
    GbParams<double> gp{(const double*)centers, n_basis, width, clip};
    typedef double TG;
    if (box)
      AGGF_GB_FORMS(images, GB_CHANNELS_OF);
    else
      AGGF_LAUNCH(gb_channels_kernel<double>, feat_grid(T * n_ch), dim3(256), 0, stream, (const double*)Pg, (const double*)cg, T, G, n_cg, site, sizes, n_ch, gp, (double*)gauss, (double*)grad);
#undef GB_CHANNELS_OF
  } else {
    return fail(AGGF_ERR_ARG, "%s: bad feature dtype", who);
  }
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

// dispatch over (force dtype, feature dtype, output dtype): out must be the promoted product dtype or float64
#define AGGF_GB_DISPATCH(WHO, LAUNCH)                                                                          \
  do {                                                                                                         \
    if (g_dtype == AGGF_F32) {                                                                                 \
      GbParams<float> gp{(const float*)centers, n_basis, (float)width, (float)clip};                           \
      typedef float TG;                                                                                        \
      if (f_dtype == AGGF_F32 && out_dtype == AGGF_F32) { typedef float TF; typedef float TO __attribute__((unused)); LAUNCH; }        \
      else if (f_dtype == AGGF_F32 && out_dtype == AGGF_F64) { typedef float TF; typedef double TO __attribute__((unused)); LAUNCH; }  \
      else if (f_dtype == AGGF_F64 && out_dtype == AGGF_F64) { typedef double TF; typedef double TO __attribute__((unused)); LAUNCH; } \
      else return fail(AGGF_ERR_ARG, "%s: bad dtype (out must be the product dtype or float64)", WHO);         \
    } else if (g_dtype == AGGF_F64) {                                                                          \
      GbParams<double> gp{(const double*)centers, n_basis, width, clip};                                       \
      typedef double TG;                                                                                       \
      if (f_dtype == AGGF_F32 && out_dtype == AGGF_F64) { typedef float TF; typedef double TO __attribute__((unused)); LAUNCH; }       \
      else if (f_dtype == AGGF_F64 && out_dtype == AGGF_F64) { typedef double TF; typedef double TO __attribute__((unused)); LAUNCH; } \
      else return fail(AGGF_ERR_ARG, "%s: bad dtype (float64 features give float64 products)", WHO);           \
    } else {                                                                                                   \
      return fail(AGGF_ERR_ARG, "%s: bad feature dtype", WHO);                                                 \
    }                                                                                                          \
  } while (0)

extern "C" int aggf_gb_regmat(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype, int64_t T,
                              int32_t G, int32_t n_cg, int32_t site, const float* sizes, int32_t n_id,
                              int32_t n_ch, const void* centers, int32_t n_basis, double width,
                              double clip, double kbt, int32_t ld_feat, void* R3, int out_dtype, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!Fg || !Pg || !cg || !sizes || !R3) return fail(AGGF_ERR_ARG, "aggf_gb_regmat: NULL pointer");
  if (T <= 0 || G <= 0 || n_ch < 0 || n_ch > G || n_id < 0 || n_id > G || site < 0 || site >= n_cg ||
      ld_feat < n_id + n_ch * n_basis)
    return fail(AGGF_ERR_ARG, "aggf_gb_regmat: bad shape");
  int rc = check_gb(centers, n_basis, width);
  if (rc) return rc;
  const dim3 grid = feat_grid(T * (n_id + n_ch));
  const char* who = "aggf_gb_regmat";
  AGGF_GB_DISPATCH(who,
                   AGGF_LAUNCH((gb_regmat_kernel<TF, TG, TO>), grid, dim3(256), 0, stream, (const TF*)Fg,
                                      (const TG*)Pg, (const TG*)cg, T, G, n_cg, site, sizes, n_id, n_ch, gp, kbt,
                                      ld_feat, (TO*)R3));
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

static int gb_apply(const char* who, const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype, int64_t T,
                    int32_t G, int32_t n_cg, const float* sizes, int32_t n_id, int32_t n_ch, const void* centers,
                    int32_t n_basis, double width, double clip, const double* coef, int32_t n_feat, const void* box,
                    int32_t bstride, int images, double* out, hipStream_t stream) {
  if (!Fg || !Pg || !cg || !sizes || !coef || !out) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (T <= 0 || G <= 0 || n_cg <= 0 || n_ch < 0 || n_ch > G || n_id < 0 || n_id > G ||
      n_feat != n_id + n_ch * n_basis)
    return fail(AGGF_ERR_ARG, "%s: bad shape", who);
  int rc = check_gb(centers, n_basis, width);
  if (rc) return rc;
  const dim3 grid = feat_grid(((T + GB_FR - 1) / GB_FR) * n_cg * 64);
  const int out_dtype = AGGF_F64;
#define GB_APPLY_OF(FORM)                                                                                           \
  AGGF_LAUNCH((gb_apply_pbc_kernel<TF, TG, FORM>), grid, dim3(256), 0, stream, (const TF*)Fg, (const TG*)Pg,        \
              (const TG*)cg, T, G, n_cg, sizes, n_id, n_ch, gp, coef, n_feat, (const TG*)box, bstride, out)
  if (box)
    AGGF_GB_DISPATCH(who, AGGF_GB_FORMS(images, GB_APPLY_OF));
  else
    AGGF_GB_DISPATCH(who, AGGF_LAUNCH((gb_apply_kernel<TF, TG>), grid, dim3(256), 0, stream, (const TF*)Fg,
                                      (const TG*)Pg, (const TG*)cg, T, G, n_cg, sizes, n_id, n_ch, gp, coef, n_feat,
                                      out));
#undef GB_APPLY_OF
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

static int gb_apply_cols(const char* who, const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype,
                         int64_t T, int32_t G, int32_t n_cg, const float* sizes, int32_t n_id, const double* coef_id,
                         const int32_t* col_ptr, const int32_t* col_idx, const double* col_val, const void* centers,
                         int32_t n_basis, double width, double clip, const void* box, int32_t bstride, int images,
                         double* out, hipStream_t stream) {
  if (!Fg || !Pg || !cg || !sizes || !col_ptr || !out || (n_id > 0 && !coef_id))
    return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (T <= 0 || G <= 0 || n_cg <= 0 || n_id < 0 || n_id > G) return fail(AGGF_ERR_ARG, "%s: bad shape", who);
  int rc = check_gb(centers, n_basis, width);
  if (rc) return rc;
  const dim3 grid = feat_grid(((T + GB_FR - 1) / GB_FR) * n_cg * 64);
  const int out_dtype = AGGF_F64;
#define GB_APPLY_COLS_OF(FORM)                                                                                      \
  AGGF_LAUNCH((gb_apply_cols_pbc_kernel<TF, TG, FORM>), grid, dim3(256), 0, stream, (const TF*)Fg, (const TG*)Pg,   \
              (const TG*)cg, T, G, n_cg, sizes, n_id, coef_id, col_ptr, col_idx, col_val, gp, (const TG*)box, bstride, \
              out)
  if (box)
    AGGF_GB_DISPATCH(who, AGGF_GB_FORMS(images, GB_APPLY_COLS_OF));
  else
    AGGF_GB_DISPATCH(who, AGGF_LAUNCH((gb_apply_cols_kernel<TF, TG>), grid, dim3(256), 0, stream, (const TF*)Fg,
                                      (const TG*)Pg, (const TG*)cg, T, G, n_cg, sizes, n_id, coef_id, col_ptr, col_idx,
                                      col_val, gp, out));
#undef GB_APPLY_COLS_OF
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

static int gb_distance_range(const char* who, const float* Pg, const float* cg, int64_t T, int32_t G, int32_t n_cg,
                             int32_t n_ch, const float* box, int32_t bstride, int images, float* rmin,
                             float* rmax, hipStream_t stream) {
  if (!Pg || !cg || !rmin || !rmax) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (T <= 0 || G <= 0 || n_cg <= 0 || n_cg > 65535 || n_ch <= 0 || n_ch > G)
    return fail(AGGF_ERR_ARG, "%s: bad shape", who);
  int64_t slices = ceil_div(T, 256);
  if (slices > 256) slices = 256;
  const dim3 grid((unsigned)ceil_div(n_ch, 256), (unsigned)n_cg, (unsigned)slices);
#define GB_RANGE_OF(FORM) \
  AGGF_LAUNCH(gb_range_pbc_kernel<FORM>, grid, dim3(256), 0, stream, Pg, cg, T, G, n_cg, n_ch, box, bstride, rmin, rmax)
  if (box)
    AGGF_GB_FORMS(images, GB_RANGE_OF);
  else
    AGGF_LAUNCH(gb_range_kernel, grid, dim3(256), 0, stream, Pg, cg, T, G, n_cg, n_ch, rmin, rmax);
#undef GB_RANGE_OF
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

static int gb_regmat_cols(const char* who, const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype,
                          int64_t T, int32_t G, int32_t n_cg, int32_t site, const float* sizes, int32_t n_id,
                          const int32_t* cols, int32_t n_cols, const void* centers, int32_t n_basis, double width,
                          double clip, double kbt, int32_t ld_feat, const void* box, int32_t bstride, int images,
                          void* R3, int out_dtype, hipStream_t stream) {
  if (!Fg || !Pg || !cg || !sizes || !R3 || (n_cols > 0 && !cols)) return fail(AGGF_ERR_ARG, "%s: NULL pointer", who);
  if (T <= 0 || G <= 0 || n_cols < 0 || n_id < 0 || n_id > G || n_id + n_cols <= 0 || site < 0 || site >= n_cg ||
      ld_feat < n_id + n_cols)
    return fail(AGGF_ERR_ARG, "%s: bad shape", who);
  int rc = check_gb(centers, n_basis, width);
  if (rc) return rc;
  const dim3 grid = feat_grid(T * (n_id + n_cols));
#define GB_REGMAT_COLS_OF(FORM)                                                                                     \
  AGGF_LAUNCH((gb_regmat_cols_pbc_kernel<TF, TG, TO, FORM>), grid, dim3(256), 0, stream, (const TF*)Fg,             \
              (const TG*)Pg, (const TG*)cg, T, G, n_cg, site, sizes, n_id, cols, n_cols, gp, kbt, ld_feat,          \
              (const TG*)box, bstride, (TO*)R3)
  if (box)
    AGGF_GB_DISPATCH(who, AGGF_GB_FORMS(images, GB_REGMAT_COLS_OF));
  else
    AGGF_GB_DISPATCH(who, AGGF_LAUNCH((gb_regmat_cols_kernel<TF, TG, TO>), grid, dim3(256), 0, stream, (const TF*)Fg,
                                      (const TG*)Pg, (const TG*)cg, T, G, n_cg, site, sizes, n_id, cols, n_cols, gp, kbt,
                                      ld_feat, (TO*)R3));
#undef GB_REGMAT_COLS_OF
  AGGF_LAUNCH_OK();
  return AGGF_OK;
}

extern "C" int aggf_gb_channels(const void* Pg, const void* cg, int g_dtype, int64_t T, int32_t G, int32_t n_cg,
                                int32_t site, const float* sizes, int32_t n_ch, const void* centers,
                                int32_t n_basis, double width, double clip, void* gauss, void* grad,
                                void* stream_v) {
  return gb_channels("aggf_gb_channels", Pg, cg, g_dtype, T, G, n_cg, site, sizes, n_ch, centers, n_basis, width, clip,
                     nullptr, 0, GB_BOX, gauss, grad, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_channels_pbc(const void* Pg, const void* cg, int g_dtype, int64_t T, int32_t G, int32_t n_cg,
                                    int32_t site, const float* sizes, int32_t n_ch, const void* centers,
                                    int32_t n_basis, double width, double clip, const void* box, int32_t box_stride,
                                    void* gauss, void* grad, void* stream_v) {
  const int rc = check_gb_box("aggf_gb_channels_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  return gb_channels("aggf_gb_channels_pbc", Pg, cg, g_dtype, T, G, n_cg, site, sizes, n_ch, centers, n_basis, width,
                     clip, box, box_stride, GB_BOX, gauss, grad, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_apply(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype, int64_t T,
                             int32_t G, int32_t n_cg, const float* sizes, int32_t n_id, int32_t n_ch,
                             const void* centers, int32_t n_basis, double width, double clip,
                             const double* coef, int32_t n_feat, double* out, void* stream_v) {
  return gb_apply("aggf_gb_apply", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, sizes, n_id, n_ch, centers, n_basis, width,
                  clip, coef, n_feat, nullptr, 0, GB_BOX, out, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_apply_pbc(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype, int64_t T,
                                 int32_t G, int32_t n_cg, const float* sizes, int32_t n_id, int32_t n_ch,
                                 const void* centers, int32_t n_basis, double width, double clip,
                                 const double* coef, int32_t n_feat, const void* box, int32_t box_stride, double* out,
                                 void* stream_v) {
  const int rc = check_gb_box("aggf_gb_apply_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  return gb_apply("aggf_gb_apply_pbc", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, sizes, n_id, n_ch, centers, n_basis,
                  width, clip, coef, n_feat, box, box_stride, GB_BOX, out, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_apply_cols(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype, int64_t T,
                                  int32_t G, int32_t n_cg, const float* sizes, int32_t n_id, const double* coef_id,
                                  const int32_t* col_ptr, const int32_t* col_idx, const double* col_val,
                                  const void* centers, int32_t n_basis, double width, double clip, double* out,
                                  void* stream_v) {
  return gb_apply_cols("aggf_gb_apply_cols", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, sizes, n_id, coef_id, col_ptr,
                       col_idx, col_val, centers, n_basis, width, clip, nullptr, 0, GB_BOX, out, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_apply_cols_pbc(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype,
                                      int64_t T, int32_t G, int32_t n_cg, const float* sizes, int32_t n_id,
                                      const double* coef_id, const int32_t* col_ptr, const int32_t* col_idx,
                                      const double* col_val, const void* centers, int32_t n_basis, double width,
                                      double clip, const void* box, int32_t box_stride, double* out, void* stream_v) {
  const int rc = check_gb_box("aggf_gb_apply_cols_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  return gb_apply_cols("aggf_gb_apply_cols_pbc", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, sizes, n_id, coef_id, col_ptr,
                       col_idx, col_val, centers, n_basis, width, clip, box, box_stride, GB_BOX, out, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_distance_range(const float* Pg, const float* cg, int64_t T, int32_t G, int32_t n_cg,
                                      int32_t n_ch, float* rmin, float* rmax, void* stream_v) {
  return gb_distance_range("aggf_gb_distance_range", Pg, cg, T, G, n_cg, n_ch, nullptr, 0, GB_BOX, rmin, rmax,
                           (hipStream_t)stream_v);
}

extern "C" int aggf_gb_distance_range_pbc(const float* Pg, const float* cg, int64_t T, int32_t G, int32_t n_cg,
                                          int32_t n_ch, const float* box, int32_t box_stride, float* rmin, float* rmax,
                                          void* stream_v) {
  const int rc = check_gb_box("aggf_gb_distance_range_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  return gb_distance_range("aggf_gb_distance_range_pbc", Pg, cg, T, G, n_cg, n_ch, box, box_stride, GB_BOX, rmin,
                           rmax, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_regmat_cols(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype, int64_t T,
                                   int32_t G, int32_t n_cg, int32_t site, const float* sizes, int32_t n_id,
                                   const int32_t* cols, int32_t n_cols, const void* centers, int32_t n_basis,
                                   double width, double clip, double kbt, int32_t ld_feat, void* R3,
                                   int out_dtype, void* stream_v) {
  return gb_regmat_cols("aggf_gb_regmat_cols", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, site, sizes, n_id, cols, n_cols,
                        centers, n_basis, width, clip, kbt, ld_feat, nullptr, 0, GB_BOX, R3, out_dtype, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_regmat_cols_pbc(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype,
                                       int64_t T, int32_t G, int32_t n_cg, int32_t site, const float* sizes,
                                       int32_t n_id, const int32_t* cols, int32_t n_cols, const void* centers,
                                       int32_t n_basis, double width, double clip, double kbt, int32_t ld_feat,
                                       const void* box, int32_t box_stride, void* R3, int out_dtype, void* stream_v) {
  const int rc = check_gb_box("aggf_gb_regmat_cols_pbc", box, box_stride);
  if (rc != AGGF_OK) return rc;
  return gb_regmat_cols("aggf_gb_regmat_cols_pbc", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, site, sizes, n_id, cols,
                        n_cols, centers, n_basis, width, clip, kbt, ld_feat, box, box_stride, GB_BOX, R3, out_dtype,
                        (hipStream_t)stream_v);
}

// ---- the _cell entries: `cell` (T, 9) in place of (box, box_stride), the selector `images` after the stream
extern "C" int aggf_gb_channels_cell(const void* Pg, const void* cg, int g_dtype, int64_t T, int32_t G, int32_t n_cg,
                                     int32_t site, const float* sizes, int32_t n_ch, const void* centers,
                                     int32_t n_basis, double width, double clip, const void* cell, void* gauss,
                                     void* grad, void* stream_v, int images) {
  const int rc = check_gb_cell("aggf_gb_channels_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return gb_channels("aggf_gb_channels_cell", Pg, cg, g_dtype, T, G, n_cg, site, sizes, n_ch, centers, n_basis, width,
                     clip, cell, 9, images, gauss, grad, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_distance_range_cell(const float* Pg, const float* cg, int64_t T, int32_t G, int32_t n_cg,
                                           int32_t n_ch, const float* cell, float* rmin, float* rmax, void* stream_v,
                                           int images) {
  const int rc = check_gb_cell("aggf_gb_distance_range_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return gb_distance_range("aggf_gb_distance_range_cell", Pg, cg, T, G, n_cg, n_ch, cell, 9, images, rmin, rmax,
                           (hipStream_t)stream_v);
}

extern "C" int aggf_gb_regmat_cols_cell(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype,
                                        int64_t T, int32_t G, int32_t n_cg, int32_t site, const float* sizes,
                                        int32_t n_id, const int32_t* cols, int32_t n_cols, const void* centers,
                                        int32_t n_basis, double width, double clip, double kbt, int32_t ld_feat,
                                        const void* cell, void* R3, int out_dtype, void* stream_v, int images) {
  const int rc = check_gb_cell("aggf_gb_regmat_cols_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return gb_regmat_cols("aggf_gb_regmat_cols_cell", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, site, sizes, n_id, cols,
                        n_cols, centers, n_basis, width, clip, kbt, ld_feat, cell, 9, images, R3, out_dtype,
                        (hipStream_t)stream_v);
}

extern "C" int aggf_gb_apply_cell(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype, int64_t T,
                                  int32_t G, int32_t n_cg, const float* sizes, int32_t n_id, int32_t n_ch,
                                  const void* centers, int32_t n_basis, double width, double clip, const double* coef,
                                  int32_t n_feat, const void* cell, double* out, void* stream_v, int images) {
  const int rc = check_gb_cell("aggf_gb_apply_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return gb_apply("aggf_gb_apply_cell", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, sizes, n_id, n_ch, centers, n_basis,
                  width, clip, coef, n_feat, cell, 9, images, out, (hipStream_t)stream_v);
}

extern "C" int aggf_gb_apply_cols_cell(const void* Fg, int f_dtype, const void* Pg, const void* cg, int g_dtype,
                                       int64_t T, int32_t G, int32_t n_cg, const float* sizes, int32_t n_id,
                                       const double* coef_id, const int32_t* col_ptr, const int32_t* col_idx,
                                       const double* col_val, const void* centers, int32_t n_basis, double width,
                                       double clip, const void* cell, double* out, void* stream_v, int images) {
  const int rc = check_gb_cell("aggf_gb_apply_cols_cell", cell, images);
  if (rc != AGGF_OK) return rc;
  return gb_apply_cols("aggf_gb_apply_cols_cell", Fg, f_dtype, Pg, cg, g_dtype, T, G, n_cg, sizes, n_id, coef_id,
                       col_ptr, col_idx, col_val, centers, n_basis, width, clip, cell, 9, images, out,
                       (hipStream_t)stream_v);
}
