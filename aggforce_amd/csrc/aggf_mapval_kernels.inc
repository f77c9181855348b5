// The three Gaussian kernels of K7 (aggf_mapval.hip includes this file twice): once as they have always been -- the open
// and periodic forms, AGGF_MV_IMAGE = brick_image, no further template parameter: the same tokens, so the same
// instructions and bits as before -- and once as the nearest-image forms, overloads with a further template parameter
// `int CELL` (CELL_NEAR the only value instantiated) and AGGF_MV_IMAGE = nearest_image.
// ---- one offset: G (T, n, 3) and per-(frame, site block) energy partials.  Thread = (frame, site i); a workgroup
// holds `fpb` frames x `iblk` sites (n <= 256: whole frames, 256 / n of them; else 1 frame x 256 sites) and stages
// the j sites of its frames in LDS, MV_JT at a time.  PBC: a thread holds the cell of its own frame.
template <typename TX, bool PBC AGGF_MV_FORM_PARAM>
__global__ __launch_bounds__(MV_THREADS) void gauss_site_forces_kernel(const TX* __restrict__ X, int64_t T, int32_t n,
                                                                        int32_t fpb, int32_t iblk, int32_t n_iblk,
                                                                        int64_t n_blocks, TX offset, TX k, double scale,
                                                                        TX* __restrict__ G, double* __restrict__ eslab,
                                                                        const TX* __restrict__ box, int32_t bstride) {
  __shared__ TX sx[MV_JT * 3];
  __shared__ double se[MV_THREADS];
  const int tid = threadIdx.x;
  const int f = tid / iblk, il = tid - f * iblk;
  for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
    const int64_t tb = b / n_iblk;
    const int ib = (int)(b - tb * n_iblk);
    const int64_t t0 = tb * fpb;
    const int nf = (int)(T - t0 < fpb ? T - t0 : fpb);
    const int64_t i = (int64_t)ib * iblk + il;
    const bool active = f < nf && il < iblk && i < n;
    const int64_t t = t0 + f;
    TX r0 = 0, r1 = 0, r2 = 0;
    if (active) {
      const TX* xi = X + (t * n + i) * 3;
      r0 = xi[0];
      r1 = xi[1];
      r2 = xi[2];
    }
    CellFrame<TX> h = {};
    if (PBC && active) mv_cell(box, bstride, t, h);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, e = 0.0;
    for (int64_t j0 = 0; j0 < n; j0 += MV_JT) {
      const int jn = (int)(n - j0 < MV_JT ? n - j0 : MV_JT);
      __syncthreads();
      for (int m = tid; m < nf * jn * 3; m += MV_THREADS) {
        const int ff = m / (jn * 3), q = m - ff * (jn * 3);
        sx[m] = X[((t0 + ff) * n + j0) * 3 + q];
      }
      __syncthreads();
      if (active) {
        const TX* base = sx + f * jn * 3;
        for (int j = 0; j < jn; ++j) {
          TX d0 = r0 - base[3 * j], d1 = r1 - base[3 * j + 1], d2 = r2 - base[3 * j + 2];
          if (PBC) AGGF_MV_IMAGE(d0, d1, d2, h);
          const TX tt = sq_norm3(d0, d1, d2) - offset;
          const TX g = Gauss<TX>::g(tt, k);
          const double c = (double)(tt * g);
          a0 += c * (double)d0;
          a1 += c * (double)d1;
          a2 += c * (double)d2;
          e += (double)g;
        }
      }
    }
    if (G && active) {
      TX* gi = G + (t * n + i) * 3;
      gi[0] = (TX)(scale * a0);
      gi[1] = (TX)(scale * a1);
      gi[2] = (TX)(scale * a2);
    }
    if (eslab) {
      se[tid] = active ? e : 0.0;
      __syncthreads();
      if (tid < nf) {
        double s = 0.0;
        for (int l = 0; l < iblk; ++l) s += se[tid * iblk + l];
        eslab[(t0 + tid) * n_iblk + ib] = s;
      }
    }
  }
}

// ---- S offsets, projection, pair form.  Grid (K splits of the T * n (n - 1) / 2 entries, offset chunks).
// slabs[k][s] = sum over split k of (x - o_s) g_s(x) u.  PBC: d is wrapped once per staged entry, under the cell of the
// entry's own frame (a stage, and a split, span several frames).
template <typename TX, typename TF, bool PBC AGGF_MV_FORM_PARAM>
__global__ __launch_bounds__(MV_THREADS) void gauss_proj_kernel(const TX* __restrict__ X, const TF* __restrict__ F,
                                                                 int64_t T, int32_t n,
                                                                 const double* __restrict__ offsets, int64_t S,
                                                                 double width, int64_t per_split,
                                                                 double* __restrict__ slabs,
                                                                 const TX* __restrict__ box, int32_t bstride) {
  typedef typename Promote<TX, TF>::type C;
  __shared__ C sx[MV_PL], su[MV_PL];
  const int tid = threadIdx.x;
  const int64_t P = (int64_t)n * (n - 1) / 2, n_entries = T * P;
  const int64_t e_begin = (int64_t)blockIdx.x * per_split;
  const int64_t e_end = e_begin + per_split < n_entries ? e_begin + per_split : n_entries;
  const int64_t s0 = (int64_t)blockIdx.y * MV_SCHUNK + tid;
  const C k = Gauss<C>::coef(width);
  C off[MV_SC];
  double acc[MV_SC];
#pragma unroll
  for (int q = 0; q < MV_SC; ++q) {
    const int64_t s = s0 + (int64_t)q * MV_THREADS;
    off[q] = s < S ? (C)offsets[s] : (C)0;
    acc[q] = 0.0;
  }
  for (int64_t e0 = e_begin; e0 < e_end; e0 += MV_PL) {
    const int ne = (int)(e_end - e0 < MV_PL ? e_end - e0 : MV_PL);
    __syncthreads();
    for (int m = tid; m < ne; m += MV_THREADS) {
      const int64_t e = e0 + m, t = e / P;
      int64_t i, j;
      pair_of(e - t * P, n, &i, &j);
      const TX* xi = X + (t * n + i) * 3;
      const TX* xj = X + (t * n + j) * 3;
      const TF* fi = F + (t * n + i) * 3;
      const TF* fj = F + (t * n + j) * 3;
      C d0 = (C)xi[0] - (C)xj[0], d1 = (C)xi[1] - (C)xj[1], d2 = (C)xi[2] - (C)xj[2];
      if (PBC) {
        CellFrame<C> h;
        mv_cell(box, bstride, t, h);
        AGGF_MV_IMAGE(d0, d1, d2, h);
      }
      sx[m] = sq_norm3(d0, d1, d2);
      su[m] = d0 * ((C)fi[0] - (C)fj[0]) + d1 * ((C)fi[1] - (C)fj[1]) + d2 * ((C)fi[2] - (C)fj[2]);
    }
    __syncthreads();
#pragma unroll 2
    for (int m = 0; m < ne; ++m) {
      const C x = sx[m], u = su[m];
#pragma unroll
      for (int q = 0; q < MV_SC; ++q) {
        const C tt = x - off[q];
        acc[q] += (double)(tt * Gauss<C>::g(tt, k) * u);
      }
    }
  }
  double* slab = slabs + (int64_t)blockIdx.x * S;
#pragma unroll
  for (int q = 0; q < MV_SC; ++q) {
    const int64_t s = s0 + (int64_t)q * MV_THREADS;
    if (s < S) slab[s] = acc[q];
  }
}

// ---- S offsets, residual shift, per-site form.  Grid (K splits of the frames, offset chunks).
// slabs[k][s][0] = sum F_i . G~_s,i, slabs[k][s][1] = sum |G~_s,i|^2 over split k's frames, G~ = G w^2 / 8.
// PBC: d is wrapped inside the j loop, under the cell of frame f (workgroup-uniform; a `whole` stage holds several).
template <typename TX, typename TF, bool PBC AGGF_MV_FORM_PARAM>
__global__ __launch_bounds__(MV_THREADS) void gauss_shift_kernel(const TX* __restrict__ X, const TF* __restrict__ F,
                                                                  int64_t T, int32_t n,
                                                                  const double* __restrict__ offsets, int64_t S,
                                                                  double width, int64_t frames_per_split,
                                                                  double* __restrict__ slabs,
                                                                  const TX* __restrict__ box, int32_t bstride) {
  typedef typename Promote<TX, TF>::type C;
  __shared__ C sx[MV_JT * 3];
  const int tid = threadIdx.x;
  const int64_t t_begin = (int64_t)blockIdx.x * frames_per_split;
  const int64_t t_end = t_begin + frames_per_split < T ? t_begin + frames_per_split : T;
  const int64_t s0 = (int64_t)blockIdx.y * MV_SCHUNK + tid;
  const C k = Gauss<C>::coef(width);
  C off[MV_SC];
  double ip[MV_SC], gs[MV_SC];
#pragma unroll
  for (int q = 0; q < MV_SC; ++q) {
    const int64_t s = s0 + (int64_t)q * MV_THREADS;
    off[q] = s < S ? (C)offsets[s] : (C)0;
    ip[q] = gs[q] = 0.0;
  }
  const bool whole = n <= MV_JT;      // whole frames in LDS, MV_JT / n of them per stage
  const int fb = whole ? MV_JT / n : 1;
  for (int64_t t0 = t_begin; t0 < t_end; t0 += fb) {
    const int nf = (int)(t_end - t0 < fb ? t_end - t0 : fb);
    if (whole) {
      __syncthreads();
      const TX* src = X + t0 * n * 3;
      for (int m = tid; m < nf * n * 3; m += MV_THREADS) sx[m] = (C)src[m];
      __syncthreads();
    }
    for (int f = 0; f < nf; ++f) {
      const int64_t t = t0 + f;
      CellFrame<C> h = {};
      if (PBC) mv_cell(box, bstride, t, h);
      for (int64_t i = 0; i < n; ++i) {
        const TX* xi = X + (t * n + i) * 3;
        const TF* fi = F + (t * n + i) * 3;
        C r0, r1, r2;
        if (whole) {
          r0 = sx[(f * n + i) * 3];
          r1 = sx[(f * n + i) * 3 + 1];
          r2 = sx[(f * n + i) * 3 + 2];
        } else {
          r0 = (C)xi[0];
          r1 = (C)xi[1];
          r2 = (C)xi[2];
        }
        double g[MV_SC][3];
#pragma unroll
        for (int q = 0; q < MV_SC; ++q) g[q][0] = g[q][1] = g[q][2] = 0.0;
        for (int64_t j0 = 0; j0 < n; j0 += MV_JT) {
          const int jn = (int)(n - j0 < MV_JT ? n - j0 : MV_JT);
          const C* base = sx + (whole ? f * n * 3 : 0);
          if (!whole) {
            __syncthreads();
            const TX* src = X + (t * n + j0) * 3;
            for (int m = tid; m < jn * 3; m += MV_THREADS) sx[m] = (C)src[m];
            __syncthreads();
          }
          for (int j = 0; j < jn; ++j) {
            C d0 = r0 - base[3 * j], d1 = r1 - base[3 * j + 1], d2 = r2 - base[3 * j + 2];
            if (PBC) AGGF_MV_IMAGE(d0, d1, d2, h);
            const C x = sq_norm3(d0, d1, d2);
            const double e0 = (double)d0, e1 = (double)d1, e2 = (double)d2;
#pragma unroll
            for (int q = 0; q < MV_SC; ++q) {
              const C tt = x - off[q];
              const double c = (double)(tt * Gauss<C>::g(tt, k));
              g[q][0] += c * e0;
              g[q][1] += c * e1;
              g[q][2] += c * e2;
            }
          }
        }
        const double f0 = (double)fi[0], f1 = (double)fi[1], f2 = (double)fi[2];
#pragma unroll
        for (int q = 0; q < MV_SC; ++q) {
          ip[q] += f0 * g[q][0] + f1 * g[q][1] + f2 * g[q][2];
          gs[q] += g[q][0] * g[q][0] + g[q][1] * g[q][1] + g[q][2] * g[q][2];
        }
      }
    }
  }
  double* slab = slabs + (int64_t)blockIdx.x * S * 2;
#pragma unroll
  for (int q = 0; q < MV_SC; ++q) {
    const int64_t s = s0 + (int64_t)q * MV_THREADS;
    if (s < S) {
      slab[2 * s] = ip[q];
      slab[2 * s + 1] = gs[q];
    }
  }
}

