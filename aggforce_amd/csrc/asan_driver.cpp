// Host-side sanitizer harness of the C ABI (`make asan`, CPU box, no GPU needed): libaggf's HOST code -- argument
// validation, launch planning, the hand-computed workspace layouts of its entry points -- built with
// -fsanitize=address,undefined (host pass only: the kernels are not compiled) and driven through
//   * every *_workspace_bytes query over a grid of shapes (empty, tiny, ragged, BASELINE-sized, absurd),
//   * every compute entry with NULL pointers and with bad shapes / dtypes: must refuse with an error code,
//   * every compute entry with plausible arguments and a workspace of the queried size: the host logic runs up to the
//     first HIP call, which fails cleanly without a device (the pointers are never dereferenced on the host).
// Exit code 0 = every call returned a documented status and the sanitizers stayed silent.
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/aggf.h"

static int n_calls = 0, n_bad = 0;
static void status(const char* what, int rc, bool must_fail) {
  ++n_calls;
  const bool known = rc == AGGF_OK || rc == AGGF_ERR_ARG || rc == AGGF_ERR_HIP || rc == AGGF_ERR_WORKSPACE || rc == AGGF_ERR_COMM;
  if (!known || (must_fail && rc == AGGF_OK)) {
    ++n_bad;
    printf("UNEXPECTED %s: rc %d (%s)\n", what, rc, aggf_last_error());
  }
}
#define REFUSED(call) status(#call, (call), true)
#define RUNS(call) status(#call, (call), false)

int main() {
  const size_t BUF = (size_t)64 << 20;
  char* raw = (char*)malloc(BUF + 512);
  char* buf = (char*)(((uintptr_t)raw + 255) & ~(uintptr_t)255);  // 256-byte aligned stand-in for every device pointer
  memset(buf, 0, 1 << 20);
  void *p = buf, *ws = buf + (1 << 20);
  double* d = (double*)buf;
  int32_t* i32 = (int32_t*)buf;
  const size_t WS = BUF - (1 << 20);
  printf("version %d\n", aggf_version());
  {
    // launch coverage: sizing call, a buffer that is too small (must stay NUL-terminated and in bounds), reset
    char small[8];
    const size_t need = aggf_coverage_dump(nullptr, 0);
    (void)aggf_coverage_dump(small, sizeof(small));
    if (small[sizeof(small) - 1] != 0 && need >= sizeof(small)) { /* (truncated text still ends inside the buffer) */ }
    RUNS(aggf_coverage_reset());
  }
  int32_t cu = 0;
  size_t fr = 0, tot = 0;
  RUNS(aggf_device_info(&cu, &fr, &tot));

  // ---- workspace queries over a grid of shapes
  const int64_t Ts[] = {0, 1, 7, 64, 1000, 100000, 1000000, (int64_t)1 << 40};
  const int32_t Ns[] = {0, 1, 3, 97, 128, 175, 1024, 4096, 20000};
  size_t sink = 0;
  for (int64_t T : Ts)
    for (int32_t N : Ns) {
      for (int in = 0; in < 2; ++in)
        for (int cd = 0; cd < 2; ++cd) {
          for (int g = 0; g < 2; ++g) sink += aggf_gram_workspace_bytes(T, N, N > 3 ? N - N / 3 : N, in, cd, g);
          for (int32_t fc : {0, 100, 128, 512}) sink += aggf_gram_from_column_workspace_bytes(T, N, N, in, cd, fc);
        }
      sink += aggf_linearmap_apply_workspace_bytes(T, N, N / 16 + 1);
      sink += aggf_gram_pair_workspace_bytes(T, N, 128, AGGF_F64);
      sink += aggf_pair_dist_var_workspace_bytes(T, N);
      sink += aggf_gauss_pair_forces_workspace_bytes(T, N);
      for (int64_t S : {(int64_t)0, (int64_t)1, (int64_t)37, (int64_t)1000, (int64_t)1 << 26, (int64_t)1 << 40}) {
        sink += aggf_gauss_proj_workspace_bytes(T, N, S);
        sink += aggf_gauss_shift_workspace_bytes(T, N, S);
      }
    }
  for (int32_t n : Ns)
    for (int32_t m : {0, 1, 10, 64, 256, 1300}) {
      sink += aggf_eq_qp_workspace_bytes(n, m, m);
      sink += aggf_eq_qp_batched_workspace_bytes(n, m, 1, 32);
      sink += aggf_eq_qp_pinned_workspace_bytes(n, m);
      sink += aggf_augmented_gram_workspace_bytes(n, m);
      sink += aggf_gram_quadform_workspace_bytes(n, m);
    }
  sink += aggf_sumsq_workspace_bytes();
  sink += aggf_dot_workspace_bytes();
  printf("workspace queries done (checksum %zu)\n", sink);

  // ---- NULL pointers / bad shapes must be refused
  REFUSED(aggf_gram(nullptr, 10, 10, 1, 1, nullptr, nullptr, 10, nullptr, 0, nullptr, 0, nullptr));
  REFUSED(aggf_gram(p, 0, 10, 1, 1, nullptr, nullptr, 10, d, 0, ws, WS, nullptr));
  REFUSED(aggf_gram(p, 10, 10, 7, 1, nullptr, nullptr, 10, d, 0, ws, WS, nullptr));
  REFUSED(aggf_gram(p, 10, 10, 1, 0, nullptr, nullptr, 10, d, 0, ws, WS, nullptr));       // f64 in, f32 products
  REFUSED(aggf_gram(p, 10, 10, 1, 1, i32, nullptr, 10, d, 0, ws, WS, nullptr));            // half a CSR
  REFUSED(aggf_gram(p, 10, 10, 1, 1, nullptr, nullptr, 11, d, 0, ws, WS, nullptr));        // n_red > N
  REFUSED(aggf_gram(p, 10, 10, 1, 1, nullptr, nullptr, 10, d, 0, (char*)ws + 8, WS, nullptr));  // misaligned workspace
  REFUSED(aggf_gram(p, 1000, 4096, 1, 1, nullptr, nullptr, 4096, d, 0, ws, 1024, nullptr));  // workspace too small
  REFUSED(aggf_gram_from_column(p, 100, 256, 1, 1, 256, 100, d, 0, ws, WS, nullptr));      // first_col % 128
  REFUSED(aggf_gram_from_column(p, 100, 256, 1, 1, 256, 128, d, 1, ws, WS, nullptr));      // accumulate with first_col
  REFUSED(aggf_eq_qp_solve(nullptr, 10, 0, nullptr, nullptr, 2, nullptr, 2, 0, 1, nullptr, nullptr, nullptr, 0, nullptr));
  REFUSED(aggf_eq_qp_solve(d, 10, -1.0, nullptr, d, 2, nullptr, 2, 0, 1, d, d, ws, WS, nullptr));
  REFUSED(aggf_eq_qp_solve(d, 10, 0.0, nullptr, d, 2, nullptr, 3, 0, 1, d, d, ws, WS, nullptr));   // B == NULL, nrhs != m
  REFUSED(aggf_eq_qp_solve(d, 10, 0.0, nullptr, d, 2, nullptr, 2, 0, 1, d, d, ws, 64, nullptr));
  REFUSED(aggf_eq_qp_solve_batched(d, 10, 0.0, nullptr, d, 2, nullptr, 2, 0, 1, 0, d, d, ws, WS, nullptr));
  REFUSED(aggf_eq_qp_solve_batched_shift(d, 10, 0.0, nullptr, d, d, i32, 11, 2, nullptr, 2, 0, 1, 2, d, d, ws, WS, nullptr));
  REFUSED(aggf_eq_qp_solve_pinned(d, 10, 0.0, nullptr, i32, 10, d, d, ws, WS, nullptr));  // m >= n
  REFUSED(aggf_eq_qp_solve_pinned(d, 10, 0.0, nullptr, nullptr, 2, d, d, ws, WS, nullptr));
  REFUSED(aggf_sym_pack_upper(nullptr, 10, 1, d, nullptr));
  REFUSED(aggf_sym_unpack_upper(d, 0, 1, d, nullptr));
  REFUSED(aggf_expand_map(nullptr, 2, 5, i32, 10, d, nullptr));
  REFUSED(aggf_linearmap_apply(nullptr, 10, 10, 1, p, 2, 1, 0, 0, p, nullptr, nullptr, ws, WS, nullptr));
  REFUSED(aggf_linearmap_apply(p, 10, 10, 1, p, 2, 1, 5, 0, p, nullptr, nullptr, ws, WS, nullptr));   // nan_mode
  REFUSED(aggf_linearmap_apply(p, 10, 10, 3, p, 2, 1, 0, 0, p, nullptr, nullptr, ws, WS, nullptr));   // dtype
  REFUSED(aggf_linearmap_apply(p, 100, 4096, 1, p, 256, 1, 0, 0, p, d, nullptr, ws, 8, nullptr));     // sumsq workspace
  REFUSED(aggf_slice_gather(p, 10, 10, 1, nullptr, 2, 1, p, nullptr, nullptr));
  REFUSED(aggf_slice_gather(p, 10, 10, 1, i32, 1 << 24, 1, p, nullptr, nullptr));
  REFUSED(aggf_has_nan(nullptr, 10, 1, i32, nullptr));
  REFUSED(aggf_not_close(p, nullptr, 10, 1, 1e-5, 1e-8, i32, nullptr));
  REFUSED(aggf_sumsq(nullptr, 10, 1, d, ws, WS, nullptr));
  REFUSED(aggf_condnormal_augment(p, p, 10, 10, 1, i32, i32, p, 2, 0, p, nullptr, 1, 0, -1.0, 1.0, p, p, nullptr));
  REFUSED(aggf_condnormal_augment(nullptr, p, 10, 10, 1, i32, i32, p, 2, 0, p, nullptr, 1, 0, 1.0, 1.0, p, p, nullptr));
  REFUSED(aggf_condnormal_sites(p, nullptr, 1, 0, 10, 2, 1, 1.0, 1.0, p, p, 0, nullptr));   // f64 sites into f32 outputs
  REFUSED(aggf_gram_pair(p, 100, p, 128, 10, 1, d, 0, ws, WS, nullptr));                     // N % 128
  REFUSED(aggf_gram_pair(p, 128, (char*)p + 8, 128, 10, 1, d, 0, ws, WS, nullptr));          // alignment
  REFUSED(aggf_augmented_gram(d, 10, 2, i32, i32, d, d, ws, WS, nullptr));                   // in place
  REFUSED(aggf_sym_group_reduce(d, 10, i32, i32, 11, d + 1000, nullptr));
  REFUSED(aggf_residual_over_var(p, 1, p, 1, 10, 0.0, p, p, 1, nullptr));
  REFUSED(aggf_residual_over_var(p, 1, p, 1, 10, 1.0, nullptr, nullptr, 1, nullptr));
  REFUSED(aggf_residual_over_var(p, 1, p, 1, 10, 1.0, p, p, 0, nullptr));
  REFUSED(aggf_frames_matmul(p, nullptr, 10, 0, p, 3, nullptr, 1.0, 1, (char*)p + 4096, nullptr));
  REFUSED(aggf_frames_matmul(p, nullptr, 10, 3, p, 3, nullptr, 1.0, 1, p, nullptr));          // out aliases X
  REFUSED(aggf_augment_concat(p, p, 1, p, p, nullptr, 1, 10, 5, 2, 1.0, p, p, nullptr));
  REFUSED(aggf_group_reduce(nullptr, 10, 10, 1, i32, i32, 3, 0, 1, p, nullptr));
  REFUSED(aggf_gb_channels(nullptr, p, 0, 10, 5, 2, 0, (float*)p, 4, p, 8, 1.0, 1e-5, p, p, nullptr));
  REFUSED(aggf_gb_regmat(nullptr, 0, p, p, 0, 10, 5, 2, 0, (float*)p, 5, 4, p, 8, 1.0, 1e-5, 0.6, 128, p, 1, nullptr));
  REFUSED(aggf_gb_distance_range(nullptr, (float*)p, 10, 5, 2, 4, (float*)p, (float*)p, nullptr));
  REFUSED(aggf_gb_regmat_cols(nullptr, 0, p, p, 0, 10, 5, 2, 0, (float*)p, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 128, p, 1, nullptr));
  REFUSED(aggf_gb_apply(nullptr, 0, p, p, 0, 10, 5, 2, (float*)p, 5, 4, p, 8, 1.0, 1e-5, d, 37, d, nullptr));
  REFUSED(aggf_gb_apply_cols(nullptr, 0, p, p, 0, 10, 5, 2, (float*)p, 5, d, i32, i32, d, p, 8, 1.0, 1e-5, d, nullptr));
  // K4 box forms: the box's own refusals (NULL, a stride other than 0 or 3), a bad dtype, a refusal of the open twin;
  // then with plausible arguments, (3,) and (T, 3), every dtype combination of the dispatch
  {
    float* fp = (float*)p;
    REFUSED(aggf_gb_channels_pbc(p, p, 0, 10, 5, 2, 0, fp, 4, p, 8, 1.0, 1e-5, nullptr, 3, p, p, nullptr));  // no box
    REFUSED(aggf_gb_channels_pbc(p, p, 0, 10, 5, 2, 0, fp, 4, p, 8, 1.0, 1e-5, p, 1, p, p, nullptr));        // stride
    REFUSED(aggf_gb_channels_pbc(p, p, 0, 10, 5, 2, 0, fp, 4, p, 8, 1.0, 1e-5, p, -3, p, p, nullptr));
    REFUSED(aggf_gb_channels_pbc(p, p, 7, 10, 5, 2, 0, fp, 4, p, 8, 1.0, 1e-5, p, 3, p, p, nullptr));        // dtype
    REFUSED(aggf_gb_channels_pbc(nullptr, p, 0, 10, 5, 2, 0, fp, 4, p, 8, 1.0, 1e-5, p, 3, p, p, nullptr));
    REFUSED(aggf_gb_channels_pbc(p, p, 0, 10, 5, 2, 2, fp, 4, p, 8, 1.0, 1e-5, p, 0, p, p, nullptr));        // site
    REFUSED(aggf_gb_distance_range_pbc(fp, fp, 10, 5, 2, 4, nullptr, 3, fp, fp, nullptr));
    REFUSED(aggf_gb_distance_range_pbc(fp, fp, 10, 5, 2, 4, fp, 6, fp, fp, nullptr));
    REFUSED(aggf_gb_distance_range_pbc(nullptr, fp, 10, 5, 2, 4, fp, 3, fp, fp, nullptr));
    REFUSED(aggf_gb_distance_range_pbc(fp, fp, 10, 5, 2, 6, fp, 0, fp, fp, nullptr));                        // n_ch > G
    REFUSED(aggf_gb_regmat_cols_pbc(p, 0, p, p, 0, 10, 5, 2, 0, fp, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 128, nullptr, 0, p, 1, nullptr));
    REFUSED(aggf_gb_regmat_cols_pbc(p, 0, p, p, 0, 10, 5, 2, 0, fp, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 128, p, 2, p, 1, nullptr));
    REFUSED(aggf_gb_regmat_cols_pbc(p, 0, p, p, 5, 10, 5, 2, 0, fp, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 128, p, 3, p, 1, nullptr));
    REFUSED(aggf_gb_regmat_cols_pbc(p, 1, p, p, 0, 10, 5, 2, 0, fp, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 128, p, 3, p, 0, nullptr));  // f64 products, f32 out
    REFUSED(aggf_gb_regmat_cols_pbc(p, 0, p, p, 0, 10, 5, 2, 0, fp, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 7, p, 3, p, 1, nullptr));    // ld_feat
    REFUSED(aggf_gb_apply_pbc(p, 0, p, p, 0, 10, 5, 2, fp, 5, 4, p, 8, 1.0, 1e-5, d, 37, nullptr, 3, d, nullptr));
    REFUSED(aggf_gb_apply_pbc(p, 0, p, p, 0, 10, 5, 2, fp, 5, 4, p, 8, 1.0, 1e-5, d, 37, p, 4, d, nullptr));
    REFUSED(aggf_gb_apply_pbc(p, 3, p, p, 0, 10, 5, 2, fp, 5, 4, p, 8, 1.0, 1e-5, d, 37, p, 3, d, nullptr));
    REFUSED(aggf_gb_apply_pbc(p, 0, p, p, 0, 10, 5, 2, fp, 5, 4, p, 8, 1.0, 1e-5, d, 36, p, 3, d, nullptr));  // n_feat
    REFUSED(aggf_gb_apply_cols_pbc(p, 0, p, p, 0, 10, 5, 2, fp, 5, d, i32, i32, d, p, 8, 1.0, 1e-5, nullptr, 0, d, nullptr));
    REFUSED(aggf_gb_apply_cols_pbc(p, 0, p, p, 0, 10, 5, 2, fp, 5, d, i32, i32, d, p, 8, 1.0, 1e-5, p, 1, d, nullptr));
    REFUSED(aggf_gb_apply_cols_pbc(p, 0, p, p, 2, 10, 5, 2, fp, 5, d, i32, i32, d, p, 8, 1.0, 1e-5, p, 3, d, nullptr));
    REFUSED(aggf_gb_apply_cols_pbc(p, 0, p, p, 0, 10, 5, 2, fp, 5, nullptr, i32, i32, d, p, 8, 1.0, 1e-5, p, 3, d, nullptr));  // id block missing
    for (int32_t bs : {0, 3}) {
      RUNS(aggf_gb_distance_range_pbc(fp, fp, 10, 5, 2, 4, fp, bs, fp, fp, nullptr));
      for (int gd = 0; gd < 2; ++gd) {
        RUNS(aggf_gb_channels_pbc(p, p, gd, 10, 5, 2, 1, fp, 4, p, 10, 1.0, 1e-3, p, bs, p, p, nullptr));
        for (int fd = 0; fd < 2; ++fd) {
          RUNS(aggf_gb_regmat_cols_pbc(p, fd, p, p, gd, 10, 5, 2, 1, fp, 5, i32, 3, p, 10, 1.0, 1e-3, 0.6, 128, p, bs, p, 1, nullptr));
          RUNS(aggf_gb_apply_pbc(p, fd, p, p, gd, 10, 5, 2, fp, 5, 4, p, 10, 1.0, 1e-3, d, 45, p, bs, d, nullptr));
          RUNS(aggf_gb_apply_cols_pbc(p, fd, p, p, gd, 10, 5, 2, fp, 5, d, i32, i32, d, p, 10, 1.0, 1e-3, p, bs, d, nullptr));
        }
      }
      RUNS(aggf_gb_regmat_cols_pbc(p, 0, p, p, 0, 10, 5, 2, 1, fp, 5, i32, 3, p, 10, 1.0, 1e-3, 0.6, 128, p, bs, p, 0, nullptr));
    }
    // the `_cell` entries: no cell, an image selector that is neither of the two, then both images over the dispatch
    REFUSED(aggf_gb_channels_cell(p, p, 0, 10, 5, 2, 0, fp, 4, p, 8, 1.0, 1e-5, nullptr, p, p, nullptr, AGGF_IMAGES_BRICK));
    REFUSED(aggf_gb_channels_cell(p, p, 0, 10, 5, 2, 0, fp, 4, p, 8, 1.0, 1e-5, p, p, p, nullptr, 2));
    REFUSED(aggf_gb_channels_cell(p, p, 7, 10, 5, 2, 0, fp, 4, p, 8, 1.0, 1e-5, p, p, p, nullptr, AGGF_IMAGES_NEAREST));  // dtype
    REFUSED(aggf_gb_distance_range_cell(fp, fp, 10, 5, 2, 4, nullptr, fp, fp, nullptr, AGGF_IMAGES_NEAREST));
    REFUSED(aggf_gb_distance_range_cell(fp, fp, 10, 5, 2, 4, fp, fp, fp, nullptr, -1));
    REFUSED(aggf_gb_distance_range_cell(fp, fp, 10, 5, 2, 6, fp, fp, fp, nullptr, AGGF_IMAGES_BRICK));  // n_ch > G
    REFUSED(aggf_gb_regmat_cols_cell(p, 0, p, p, 0, 10, 5, 2, 0, fp, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 128, nullptr, p, 1, nullptr, AGGF_IMAGES_BRICK));
    REFUSED(aggf_gb_regmat_cols_cell(p, 0, p, p, 0, 10, 5, 2, 0, fp, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 128, p, p, 1, nullptr, 3));
    REFUSED(aggf_gb_regmat_cols_cell(p, 0, p, p, 0, 10, 5, 2, 0, fp, 5, i32, 3, p, 8, 1.0, 1e-5, 0.6, 7, p, p, 1, nullptr, AGGF_IMAGES_NEAREST));  // ld_feat
    REFUSED(aggf_gb_apply_cell(p, 0, p, p, 0, 10, 5, 2, fp, 5, 4, p, 8, 1.0, 1e-5, d, 37, nullptr, d, nullptr, AGGF_IMAGES_NEAREST));
    REFUSED(aggf_gb_apply_cell(p, 0, p, p, 0, 10, 5, 2, fp, 5, 4, p, 8, 1.0, 1e-5, d, 37, p, d, nullptr, 7));
    REFUSED(aggf_gb_apply_cell(p, 0, p, p, 0, 10, 5, 2, fp, 5, 4, p, 8, 1.0, 1e-5, d, 36, p, d, nullptr, AGGF_IMAGES_BRICK));  // n_feat
    REFUSED(aggf_gb_apply_cols_cell(p, 0, p, p, 0, 10, 5, 2, fp, 5, d, i32, i32, d, p, 8, 1.0, 1e-5, nullptr, d, nullptr, AGGF_IMAGES_BRICK));
    REFUSED(aggf_gb_apply_cols_cell(p, 0, p, p, 0, 10, 5, 2, fp, 5, d, i32, i32, d, p, 8, 1.0, 1e-5, p, d, nullptr, -2));
    for (int images : {AGGF_IMAGES_BRICK, AGGF_IMAGES_NEAREST}) {
      RUNS(aggf_gb_distance_range_cell(fp, fp, 10, 5, 2, 4, fp, fp, fp, nullptr, images));
      for (int gd = 0; gd < 2; ++gd) {
        RUNS(aggf_gb_channels_cell(p, p, gd, 10, 5, 2, 1, fp, 4, p, 10, 1.0, 1e-3, p, p, p, nullptr, images));
        for (int fd = 0; fd < 2; ++fd) {
          RUNS(aggf_gb_regmat_cols_cell(p, fd, p, p, gd, 10, 5, 2, 1, fp, 5, i32, 3, p, 10, 1.0, 1e-3, 0.6, 128, p, p, 1, nullptr, images));
          RUNS(aggf_gb_apply_cell(p, fd, p, p, gd, 10, 5, 2, fp, 5, 4, p, 10, 1.0, 1e-3, d, 45, p, d, nullptr, images));
          RUNS(aggf_gb_apply_cols_cell(p, fd, p, p, gd, 10, 5, 2, fp, 5, d, i32, i32, d, p, 10, 1.0, 1e-3, p, d, nullptr, images));
        }
      }
      RUNS(aggf_gb_regmat_cols_cell(p, 0, p, p, 0, 10, 5, 2, 1, fp, 5, i32, 3, p, 10, 1.0, 1e-3, 0.6, 128, p, p, 0, nullptr, images));
    }
  }
  REFUSED(aggf_trjdot_frames(nullptr, 1, p, 1, 10, 5, 2, nullptr, p, 1, nullptr));
  REFUSED(aggf_feat_contract(nullptr, 0, p, p, 0, 1.0, 10, 5, 7, 128, p, 1, nullptr));
  REFUSED(aggf_feat_constraint_rows(nullptr, 0, 10, 5, 7, (int64_t*)p, 3, d, 2, 0, d, d, nullptr));
  REFUSED(aggf_gb_constraint_rows(nullptr, p, 0, 3, 2, 5, 5, 4, 8, i32, 3, 128, 0, d, d, nullptr));
  REFUSED(aggf_gb_group_overlap(nullptr, 2, 5, d, nullptr));
  REFUSED(aggf_gb_constraint_gram(nullptr, p, 0, 3, 5, 5, 4, 8, i32, 3, 128, d, nullptr));
  REFUSED(aggf_feat_weights(nullptr, 0, 10, 5, 7, d, 10, d, nullptr));
  REFUSED(aggf_pair_dist_var(nullptr, 10, 5, 1, d, ws, WS, nullptr));
  REFUSED(aggf_pair_dist_moments(p, 10, 5, 1, nullptr, d, ws, WS, nullptr));
  // K6 box forms: the box's own refusals (NULL, a stride other than 0 or 3), then those of the open twins
  REFUSED(aggf_pair_dist_var_pbc(p, 10, 5, 1, nullptr, 3, d, ws, WS, nullptr));  // no box
  REFUSED(aggf_pair_dist_var_pbc(p, 10, 5, 1, p, 1, d, ws, WS, nullptr));        // stride
  REFUSED(aggf_pair_dist_var_pbc(p, 10, 5, 1, p, -3, d, ws, WS, nullptr));
  REFUSED(aggf_pair_dist_var_pbc(nullptr, 10, 5, 1, p, 3, d, ws, WS, nullptr));
  REFUSED(aggf_pair_dist_var_pbc(p, 10, 5, 1, p, 3, nullptr, ws, WS, nullptr));
  REFUSED(aggf_pair_dist_var_pbc(p, 10, 5, 1, p, 0, d, nullptr, WS, nullptr));
  REFUSED(aggf_pair_dist_var_pbc(p, 0, 5, 1, p, 3, d, ws, WS, nullptr));
  REFUSED(aggf_pair_dist_var_pbc(p, 10, 5, 2, p, 3, d, ws, WS, nullptr));        // dtype
  REFUSED(aggf_pair_dist_var_pbc(p, 1000, 4096, 1, p, 3, d, ws, 1024, nullptr));  // workspace too small
  REFUSED(aggf_pair_dist_moments_pbc(p, 10, 5, 1, nullptr, 0, d, d + 4096, ws, WS, nullptr));  // no box
  REFUSED(aggf_pair_dist_moments_pbc(p, 10, 5, 1, p, 2, d, d + 4096, ws, WS, nullptr));        // stride
  REFUSED(aggf_pair_dist_moments_pbc(p, 10, 5, 1, p, 3, nullptr, d, ws, WS, nullptr));         // no mean
  REFUSED(aggf_pair_dist_moments_pbc(p, 10, 0, 0, p, 0, d, d + 4096, ws, WS, nullptr));
  // K7: NULL pointers, bad shapes / dtypes / sample counts, widths that are not positive, short workspaces
  REFUSED(aggf_gauss_pair_forces(nullptr, 10, 5, 1, 1.0, 0.5, nullptr, 0, p, nullptr, ws, WS, nullptr));
  REFUSED(aggf_gauss_pair_forces(p, 10, 5, 1, 1.0, 0.5, nullptr, 0, nullptr, nullptr, ws, WS, nullptr));  // no G, no E
  REFUSED(aggf_gauss_pair_forces(p, 10, 5, 1, 1.0, 0.5, nullptr, 0, nullptr, p, nullptr, WS, nullptr));  // E, no workspace
  REFUSED(aggf_gauss_pair_forces(p, 10, 5, 1, 1.0, 0.5, nullptr, 0, nullptr, p, ws, 8, nullptr));
  REFUSED(aggf_gauss_pair_forces(p, 0, 5, 1, 1.0, 0.5, nullptr, 0, p, nullptr, ws, WS, nullptr));
  REFUSED(aggf_gauss_pair_forces(p, 10, 0, 1, 1.0, 0.5, nullptr, 0, p, nullptr, ws, WS, nullptr));
  REFUSED(aggf_gauss_pair_forces(p, (int64_t)1 << 40, 20000, 1, 1.0, 0.5, nullptr, 0, p, nullptr, ws, WS, nullptr));
  REFUSED(aggf_gauss_pair_forces(p, 10, 5, 2, 1.0, 0.5, nullptr, 0, p, nullptr, ws, WS, nullptr));
  REFUSED(aggf_gauss_pair_forces(p, 10, 5, 1, 1.0, 0.0, nullptr, 0, p, nullptr, ws, WS, nullptr));
  REFUSED(aggf_gauss_pair_forces(p, 10, 5, 1, 1.0, -1.0, nullptr, 0, p, nullptr, ws, WS, nullptr));
  for (int32_t stride : {-3, 1, 2, 6, 12})  // a box whose stride is none of 0, 3 and 9
    REFUSED(aggf_gauss_pair_forces(p, 10, 5, 1, 1.0, 0.5, p, stride, p, nullptr, ws, WS, nullptr));
  for (int shift = 0; shift < 2; ++shift) {
    auto call = [&](const void* X, int xd, const void* F, int fd, int64_t T, int32_t n, const double* o, int64_t S,
                    double w, double* out, size_t wsb) {
      return shift ? aggf_gauss_shift(X, xd, F, fd, T, n, o, S, w, nullptr, 0, out, out ? d + 4096 : nullptr, ws, wsb,
                                      nullptr)
                   : aggf_gauss_proj(X, xd, F, fd, T, n, o, S, w, nullptr, 0, out, ws, wsb, nullptr);
    };
    for (int32_t stride : {-3, 1, 2, 6, 12})
      REFUSED(shift ? aggf_gauss_shift(p, 1, p, 1, 10, 5, d, 4, 0.5, p, stride, d, d + 4096, ws, WS, nullptr)
                    : aggf_gauss_proj(p, 1, p, 1, 10, 5, d, 4, 0.5, p, stride, d, ws, WS, nullptr));
    REFUSED(call(nullptr, 1, p, 1, 10, 5, d, 4, 0.5, d, WS));
    REFUSED(call(p, 1, nullptr, 1, 10, 5, d, 4, 0.5, d, WS));
    REFUSED(call(p, 1, p, 1, 10, 5, nullptr, 4, 0.5, d, WS));
    REFUSED(call(p, 1, p, 1, 10, 5, d, 4, 0.5, nullptr, WS));
    REFUSED(call(p, 3, p, 1, 10, 5, d, 4, 0.5, d, WS));
    REFUSED(call(p, 1, p, -1, 10, 5, d, 4, 0.5, d, WS));
    REFUSED(call(p, 1, p, 1, -1, 5, d, 4, 0.5, d, WS));
    REFUSED(call(p, 1, p, 1, 10, -5, d, 4, 0.5, d, WS));
    REFUSED(call(p, 1, p, 1, 10, 5, d, 0, 0.5, d, WS));
    REFUSED(call(p, 1, p, 1, 10, 5, d, (int64_t)1 << 40, 0.5, d, WS));
    REFUSED(call(p, 1, p, 1, 10, 5, d, 4, 0.0, d, WS));
    REFUSED(call(p, 1, p, 1, 10, 5, d, 4, __builtin_nan(""), d, WS));
    REFUSED(call(p, 1, p, 1, 100000, 256, d, 1000, 0.5, d, 64));
  }
  REFUSED(aggf_dot(nullptr, 1, p, 1, 10, d, ws, WS, nullptr));
  REFUSED(aggf_dot(p, 1, p, 1, 10, nullptr, ws, WS, nullptr));
  REFUSED(aggf_dot(p, 1, p, 7, 10, d, ws, WS, nullptr));
  REFUSED(aggf_dot(p, 1, p, 1, -1, d, ws, WS, nullptr));
  REFUSED(aggf_dot(p, 1, p, 1, 10, d, ws, 8, nullptr));
  REFUSED(aggf_pair_pool_term(nullptr, d, d, 1.0, 10, d, nullptr));
  REFUSED(aggf_gram_quadform(nullptr, 10, d, 2, d, ws, WS, nullptr));
  REFUSED(aggf_daxpby(10, 1.0, nullptr, 1.0, d, d, nullptr));
  REFUSED(aggf_comm_unique_id(nullptr, 128));
  REFUSED(aggf_comm_unique_id(p, 8));
  REFUSED(aggf_comm_init(p, 8, 0, 1, (void**)p));
  REFUSED(aggf_comm_init(p, 128, 3, 2, (void**)p));
  RUNS(aggf_comm_destroy(nullptr));  // (like free(NULL): nothing to do)
  REFUSED(aggf_allreduce_sum(nullptr, 4, 1, nullptr, nullptr));
  REFUSED(aggf_synth_normal(nullptr, 10, 5, 1, 1, 0, 0, 1, 0, nullptr));
  REFUSED(aggf_synth_normal(p, 10, 5, 9, 1, 0, 0, 1, 0, nullptr));

  // ---- plausible calls: planning and workspace arithmetic run; without a device the first HIP call fails cleanly
  struct Shape { int64_t T; int32_t N, n_red, n_cg; };
  const Shape shapes[] = {{500, 6, 6, 2}, {4000, 175, 97, 10}, {5000, 1024, 683, 64}, {3000, 4096, 4096, 256}, {777, 333, 200, 7}};
  for (const Shape& s : shapes) {
    for (int in = 0; in < 2; ++in)
      for (int cd = in; cd < 2; ++cd) {
        const bool groups = s.n_red != s.N;
        const size_t need = aggf_gram_workspace_bytes(s.T, s.N, s.n_red, in, cd, groups);
        if (need <= WS) RUNS(aggf_gram(p, s.T, s.N, in, cd, groups ? i32 : nullptr, groups ? i32 : nullptr, s.n_red, d, 0, ws, need, nullptr));
        if (need <= WS) RUNS(aggf_gram(p, s.T, s.N, in, cd, groups ? i32 : nullptr, groups ? i32 : nullptr, s.n_red, d, 1, ws, need / 2 + 4096 & ~(size_t)255, nullptr));
      }
    const size_t wa = aggf_linearmap_apply_workspace_bytes(s.T, s.N, s.n_cg);
    for (int in = 0; in < 2; ++in)
      for (int od = 0; od < 2; ++od)
        for (int nm = 0; nm < 2; ++nm)
          RUNS(aggf_linearmap_apply(p, s.T, s.N, in, p, s.n_cg, od, nm, -1.0, (char*)p + 4096, d, i32, ws, wa, nullptr));
    RUNS(aggf_slice_gather(p, s.T, s.N, 1, i32, s.n_cg, 1, (char*)p + 4096, i32, nullptr));
    if (s.n_red <= 1100) {
      const size_t w1 = aggf_eq_qp_workspace_bytes(s.n_red, s.n_cg, s.n_cg);
      if (w1 <= WS) RUNS(aggf_eq_qp_solve(d, s.n_red, 0.5, nullptr, d, s.n_cg, nullptr, s.n_cg, 1e-12, 2, d, d, ws, w1, nullptr));
      const size_t w2 = aggf_eq_qp_pinned_workspace_bytes(s.n_red, s.n_cg);
      if (w2 <= WS) RUNS(aggf_eq_qp_solve_pinned(d, s.n_red, 0.0, d, i32, s.n_cg, d, d, ws, w2, nullptr));
      const size_t w3 = aggf_eq_qp_batched_workspace_bytes(s.n_red, s.n_cg, 1, 3);
      if (w3 <= WS) RUNS(aggf_eq_qp_solve_batched(d, s.n_red, 10.0, nullptr, d, s.n_cg, d, 1, 1e-12, 3, 3, d, d, ws, w3, nullptr));
      if (w3 <= WS) RUNS(aggf_eq_qp_solve_batched_shift(d, s.n_red, 10.0, nullptr, d, d, i32, s.n_red / 2, s.n_cg, d, 1, 1e-12, 3, 3, d, d, ws, w3, nullptr));
    }
    RUNS(aggf_sumsq(p, s.T * s.N * 3, 1, d, ws, aggf_sumsq_workspace_bytes(), nullptr));
    RUNS(aggf_condnormal_sites(p, nullptr, 42100, 17, s.T, s.n_cg, 0, 0.01, 0.6955215, (char*)p + 4096, (char*)p + 8192, 1, nullptr));
    RUNS(aggf_condnormal_augment(p, p, s.T, s.N, 1, i32, i32, p, s.n_cg, 0, p, nullptr, 42100, 0, 0.01, 0.6955215, (char*)p + 4096, (char*)p + 8192, nullptr));
    RUNS(aggf_residual_over_var(p, 0, p, 0, s.T * s.n_cg * 3, 0.01, (char*)p + 4096, nullptr, 0, nullptr));
    RUNS(aggf_frames_matmul(p, p, s.T, 3 * s.n_cg, p, 3 * s.n_cg, nullptr, -1.0, 1, (char*)p + 4096, nullptr));
    RUNS(aggf_augment_concat(p, p, 1, p, p, p, 0, s.T, s.N, s.n_cg, 0.6955215, (char*)p + 4096, (char*)p + 8192, nullptr));
    const size_t wp = aggf_pair_dist_var_workspace_bytes(s.T, s.N);
    if (wp <= WS) RUNS(aggf_pair_dist_var(p, s.T, s.N, 1, d, ws, wp, nullptr));
    for (int in = 0; in < 2; ++in)
      for (int32_t bs : {0, 3}) {
        if (wp <= WS) RUNS(aggf_pair_dist_var_pbc(p, s.T, s.N, in, p, bs, d, ws, wp, nullptr));
        if (wp <= WS) RUNS(aggf_pair_dist_moments_pbc(p, s.T, s.N, in, p, bs, d, d + 4096, ws, wp, nullptr));
      }
    RUNS(aggf_synth_normal(p, s.T, s.N, 1, 42100, 5, 0.0, 30.0, 1.5, nullptr));
  }
  {
    const size_t wpair = aggf_gram_pair_workspace_bytes(2000, 2048, 128, AGGF_F32);
    if (wpair <= WS) RUNS(aggf_gram_pair(p, 2048, (char*)p + 4096, 128, 2000, AGGF_F32, d, 0, ws, wpair, nullptr));
    const size_t wag = aggf_augmented_gram_workspace_bytes(2048, 128);
    if (wag <= WS) RUNS(aggf_augmented_gram(d, 2048, 128, i32, i32, d, d + 4096, ws, wag, nullptr));
    const size_t wq = aggf_gram_quadform_workspace_bytes(4096, 256);
    if (wq <= WS) RUNS(aggf_gram_quadform(d, 4096, d, 256, d + 4096, ws, wq, nullptr));
    RUNS(aggf_sym_pack_upper(d, 4096, 1, d + 4096, nullptr));
    REFUSED(aggf_sym_unpack_upper(d, 4096, 1, d + 4096, nullptr));  // packed and G overlap
    RUNS(aggf_sym_unpack_upper(d, 64, 1, d + 4096, nullptr));
    RUNS(aggf_expand_map(d, 256, 2731, i32, 4096, d + 4096, nullptr));
    RUNS(aggf_has_nan(p, 1000, 0, i32, nullptr));
    RUNS(aggf_not_close(p, (char*)p + 4096, 1000, 1, 1e-5, 1e-6, i32, nullptr));
    RUNS(aggf_daxpby(1000, 1.0, d, -1.0, d + 1000, d + 2000, nullptr));
  }
  // K7 with plausible arguments and the queried workspace: every dtype pair, few and many sites, few and many samples
  for (int64_t T : {(int64_t)1, (int64_t)7, (int64_t)100000})
    for (int32_t n : {1, 2, 10, 256, 1025, 4096})
      for (int64_t S : {(int64_t)1, (int64_t)37, (int64_t)1000, (int64_t)70000}) {
        const size_t wf = aggf_gauss_pair_forces_workspace_bytes(T, n);
        const size_t wpj = aggf_gauss_proj_workspace_bytes(T, n, S), wsh = aggf_gauss_shift_workspace_bytes(T, n, S);
        for (int xd = 0; xd < 2; ++xd)
          for (int fd = 0; fd < 2; ++fd) {
            if (fd == 0 && S == 1) {
              if (wf <= WS)
                RUNS(aggf_gauss_pair_forces(p, T, n, xd, 37.0, 0.25, nullptr, 0, p, (char*)p + 4096, ws, wf, nullptr));
              RUNS(aggf_gauss_pair_forces(p, T, n, xd, 37.0, 0.25, nullptr, 0, p, nullptr, nullptr, 0, nullptr));
              for (int32_t stride : {0, 3, 9})  // under a box or a cell: the same plan and workspace
                RUNS(aggf_gauss_pair_forces(p, T, n, xd, 37.0, 0.25, p, stride, p, nullptr, nullptr, 0, nullptr));
            }
            for (int32_t stride : {-1, 0, 3, 9}) {  // (-1: open)
              const void* box = stride < 0 ? nullptr : p;
              if (wpj <= WS) RUNS(aggf_gauss_proj(p, xd, p, fd, T, n, d, S, 0.25, box, stride, d + 4096, ws, wpj, nullptr));
              if (wsh <= WS)
                RUNS(aggf_gauss_shift(p, xd, p, fd, T, n, d, S, 0.25, box, stride, d + 4096, d + 8192, ws, wsh, nullptr));
            }
            for (int images : {AGGF_IMAGES_BRICK, AGGF_IMAGES_NEAREST}) {  // the `_cell` entries: the same plans
              if (fd == 0 && S == 1)
                RUNS(aggf_gauss_pair_forces_cell(p, T, n, xd, 37.0, 0.25, p, p, nullptr, nullptr, 0, nullptr, images));
              if (wpj <= WS) RUNS(aggf_gauss_proj_cell(p, xd, p, fd, T, n, d, S, 0.25, p, d + 4096, ws, wpj, nullptr, images));
              if (wsh <= WS)
                RUNS(aggf_gauss_shift_cell(p, xd, p, fd, T, n, d, S, 0.25, p, d + 4096, d + 8192, ws, wsh, nullptr, images));
            }
            RUNS(aggf_dot(p, xd, (char*)p + 4096, fd, T * n * 3, d, ws, aggf_dot_workspace_bytes(), nullptr));
          }
      }
  // the `_cell` entries of K7: no cell, an image selector that is neither of the two
  REFUSED(aggf_gauss_pair_forces_cell(p, 10, 5, 1, 1.0, 0.5, nullptr, p, nullptr, ws, WS, nullptr, AGGF_IMAGES_NEAREST));
  REFUSED(aggf_gauss_pair_forces_cell(p, 10, 5, 1, 1.0, 0.5, p, p, nullptr, ws, WS, nullptr, 2));
  REFUSED(aggf_gauss_proj_cell(p, 1, p, 1, 10, 5, d, 4, 0.5, nullptr, d, ws, WS, nullptr, AGGF_IMAGES_NEAREST));
  REFUSED(aggf_gauss_proj_cell(p, 1, p, 1, 10, 5, d, 4, 0.5, p, d, ws, WS, nullptr, -1));
  REFUSED(aggf_gauss_shift_cell(p, 1, p, 1, 10, 5, d, 4, 0.5, nullptr, d, d + 4096, ws, WS, nullptr, AGGF_IMAGES_BRICK));
  REFUSED(aggf_gauss_shift_cell(p, 1, p, 1, 10, 5, d, 4, 0.5, p, d, d + 4096, ws, WS, nullptr, 9));
  REFUSED(aggf_gauss_proj_cell(p, 1, p, 1, 10, 5, d, 4, 0.0, p, d, ws, WS, nullptr, AGGF_IMAGES_NEAREST));  // width
  // K8: the workspace query over a grid of shapes, refusals, and plausible calls with the queried workspace
  for (int64_t T : Ts)
    for (int32_t N : Ns) sink += aggf_trjdot_cross_workspace_bytes(T, N / 16 + 1, N, 1) + aggf_trjdot_cross_workspace_bytes(T, N, N, 0);
  REFUSED(aggf_trjdot_cross(nullptr, p, 7, 3, 5, 1, d, 1, 0, ws, WS, nullptr));
  REFUSED(aggf_trjdot_cross(p, p, 0, 3, 5, 1, d, 1, 0, ws, WS, nullptr));
  REFUSED(aggf_trjdot_cross(p, p, 7, 3, 5, 2, d, 1, 0, ws, WS, nullptr));
  REFUSED(aggf_trjdot_cross(p, p, 7, 3, 5, 1, d, 1, 0, ws, 0, nullptr));
  REFUSED(aggf_trjdot_frames_t(p, nullptr, 1, 7, 3, 5, d, 1, nullptr));
  REFUSED(aggf_trjdot_frames_t(p, p, 0, 7, 3, 5, d, 1, nullptr));  // float32 in, float64 out
  REFUSED(aggf_trjdot_frames_outer(p, p, 1, 7, 0, 5, d, 1, nullptr));
  REFUSED(aggf_trjdot_frames_outer(p, p, 0, 7, 3, 5, d, 1, nullptr));
  for (int64_t T : {(int64_t)1, (int64_t)67, (int64_t)2000, (int64_t)100000, (int64_t)1000000})
    for (int32_t na : {1, 10, 257})
      for (int32_t nb : {1, 33, 166, 4096}) {
        const size_t wx = aggf_trjdot_cross_workspace_bytes(T, na, nb, 1);
        for (int in = 0; in < 2; ++in)
          for (int od = 0; od < 2; ++od) {
            if (wx <= WS) RUNS(aggf_trjdot_cross(p, (char*)p + 4096, T, na, nb, in, d, od, od, ws, wx, nullptr));
            if (in >= od) {
              RUNS(aggf_trjdot_frames_t(p, (char*)p + 4096, in, T, na, nb, d, od, nullptr));
              RUNS(aggf_trjdot_frames_outer(p, (char*)p + 4096, in, T, na, nb, d, od, nullptr));
            }
          }
      }
  // K9: the workspace query over the grid of shapes (overflowing ones included), refusals, empty shapes (no launch,
  // no pointer needed), and plausible calls in every mode / dtype pair / output selection with the queried workspace
  for (int64_t T : Ts)
    for (int32_t N : Ns) sink += aggf_pair_pull_workspace_bytes(T, N / 16 + 1, N, 0) + aggf_pair_pull_workspace_bytes(T, N, N / 16 + 1, 1);
  sink += aggf_pair_pull_workspace_bytes(INT64_MAX, 20000, 20000, 1) + aggf_pair_pull_workspace_bytes(-1, 5, 300, 0);
  REFUSED(aggf_pair_dist(nullptr, p, nullptr, nullptr, 7, 3, 5, 1, AGGF_PAIR_DIST, d, nullptr));
  REFUSED(aggf_pair_dist(p, p, nullptr, nullptr, 7, 3, 5, 1, AGGF_PAIR_DIST, nullptr, nullptr));
  REFUSED(aggf_pair_dist(p, p, p, nullptr, 7, 3, 5, 1, AGGF_PAIR_DOT, d, nullptr));      // DOT without Y
  REFUSED(aggf_pair_dist(p, p, nullptr, nullptr, 7, 3, 5, 2, AGGF_PAIR_DIST, d, nullptr));  // dtype
  REFUSED(aggf_pair_dist(p, p, nullptr, nullptr, 7, 3, 5, 1, 3, d, nullptr));             // mode
  REFUSED(aggf_pair_dist(p, p, nullptr, nullptr, -1, 3, 5, 1, AGGF_PAIR_DIST, d, nullptr));
  REFUSED(aggf_pair_dist(p, p, nullptr, nullptr, (int64_t)1 << 40, 20000, 20000, 1, AGGF_PAIR_DIST, d, nullptr));  // T m n
  RUNS(aggf_pair_dist(nullptr, nullptr, nullptr, nullptr, 0, 3, 5, 1, AGGF_PAIR_DIST, nullptr, nullptr));
  RUNS(aggf_pair_dist(nullptr, nullptr, nullptr, nullptr, 7, 3, 0, 0, AGGF_PAIR_DOT, nullptr, nullptr));
  REFUSED(aggf_pair_pull(nullptr, nullptr, p, p, 7, 3, 5, 1, d, d, 1, ws, WS, nullptr));
  REFUSED(aggf_pair_pull(p, nullptr, p, nullptr, 7, 3, 5, 1, d, d, 1, ws, WS, nullptr));
  REFUSED(aggf_pair_pull(p, nullptr, p, p, 7, 3, 5, 0, d, d, 1, ws, WS, nullptr));        // float32 in, float64 out
  REFUSED(aggf_pair_pull(p, nullptr, p, p, 7, 3, 5, 1, d, d, 5, ws, WS, nullptr));
  REFUSED(aggf_pair_pull(p, nullptr, p, p, 7, -3, 5, 1, d, d, 1, ws, WS, nullptr));
  REFUSED(aggf_pair_pull(p, nullptr, p, p, 7, 3, 300, 1, d, d, 1, ws, 0, nullptr));       // two panels, no workspace
  REFUSED(aggf_pair_pull(p, nullptr, p, p, 7, 3, 300, 1, d, d, 1, nullptr, WS, nullptr));
  REFUSED(aggf_pair_pull(p, nullptr, p, p, 7, 3, 300, 1, d, d, 1, (char*)ws + 4, WS - 4, nullptr));  // misaligned partials
  REFUSED(aggf_pair_pull(p, nullptr, p, p, INT64_MAX / 4, 1, 3, 1, d, d, 1, ws, WS, nullptr));
  RUNS(aggf_pair_pull(nullptr, nullptr, nullptr, nullptr, 7, 0, 5, 1, nullptr, nullptr, 1, nullptr, 0, nullptr));
  RUNS(aggf_pair_pull(p, nullptr, p, p, 7, 3, 5, 1, nullptr, nullptr, 1, nullptr, 0, nullptr));  // neither output
  RUNS(aggf_pair_pull(p, nullptr, p, p, 7, 3, 300, 1, d, nullptr, 1, nullptr, 0, nullptr));      // A alone: no partials
  for (int64_t T : {(int64_t)1, (int64_t)67, (int64_t)100000})
    for (int32_t m : {1, 17, 257, 8200})
      for (int32_t n : {1, 65, 256, 257, 8200}) {
        for (int in = 0; in < 2; ++in) {
          const size_t wpl = aggf_pair_pull_workspace_bytes(T, m, n, in);
          for (int mode : {AGGF_PAIR_DIST, AGGF_PAIR_SQDIST, AGGF_PAIR_DOT})
            RUNS(aggf_pair_dist(p, (char*)p + 4096, p, (char*)p + 4096, T, m, n, in, mode, d, nullptr));
          for (int od = 0; od <= in; ++od)
            for (int sel = 1; sel < 4; ++sel)
              if (wpl <= WS)
                RUNS(aggf_pair_pull(p, sel == 3 ? p : nullptr, p, (char*)p + 4096, T, m, n, in, sel & 1 ? d : nullptr,
                                    sel & 2 ? d + 4096 : nullptr, od, ws, wpl, nullptr));
        }
      }
  // K9c / K9d: refusals (NULL pointers, bad dtype / mode, negative or oversized shapes, an output without its table),
  // empty problems (no launch, no pointer needed), and plausible calls in every mode / dtype pair / output selection /
  // form of the pull kernel (the degrees on either side of its threshold)
  REFUSED(aggf_pair_list_dist(nullptr, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, d, nullptr));
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, nullptr, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, d, nullptr));  // no list
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, nullptr, nullptr));
  REFUSED(aggf_pair_list_dist(p, p, p, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DOT, d, nullptr));            // DOT without Y
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 2, AGGF_PAIR_DIST, d, nullptr));     // dtype
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, 3, d, nullptr));                  // mode
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, i32, -1, 3, 5, 9, 1, AGGF_PAIR_DIST, d, nullptr));
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, i32, 7, 3, 5, -9, 1, AGGF_PAIR_DIST, d, nullptr));
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, i32, 7, 3, 5, (int64_t)1 << 31, 1, AGGF_PAIR_DIST, d, nullptr));  // P
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, i32, (int64_t)1 << 40, 3, 5, 1 << 30, 1, AGGF_PAIR_DIST, d, nullptr));  // T P
  REFUSED(aggf_pair_list_dist(p, p, nullptr, nullptr, i32, INT64_MAX / 4, 3, 5, 1, 1, AGGF_PAIR_DIST, d, nullptr));     // T n
  RUNS(aggf_pair_list_dist(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3, 5, 9, 1, AGGF_PAIR_DIST, nullptr, nullptr));
  RUNS(aggf_pair_list_dist(nullptr, nullptr, nullptr, nullptr, nullptr, 7, 3, 5, 0, 0, AGGF_PAIR_DOT, nullptr, nullptr));
  REFUSED(aggf_pair_list_pull(nullptr, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull(p, nullptr, p, nullptr, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, nullptr, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, d, d, 1, nullptr));  // no list
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, i32, nullptr, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, d, d, 1, nullptr));  // A, no table
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, i32, nullptr, 2, 2, 7, 3, 5, 9, 1, d, d, 1, nullptr));  // B, no table
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 0, d, d, 1, nullptr));  // float32 in, float64 out
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, d, d, 5, nullptr));
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, -3, 5, 9, 1, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, i32, i32, -1, 2, 7, 3, 5, 9, 1, d, d, 1, nullptr));  // degree
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, (int64_t)1 << 31, 1, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, INT64_MAX / 4, 3, 5, 9, 1, d, d, 1, nullptr));
  RUNS(aggf_pair_list_pull(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 7, 3, 5, 0, 1, nullptr, nullptr, 1, nullptr));
  RUNS(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, nullptr, nullptr, 1, nullptr));  // neither output
  RUNS(aggf_pair_list_pull(p, nullptr, p, p, i32, i32, i32, nullptr, nullptr, 2, 2, 7, 3, 5, 9, 1, d, nullptr, 1, nullptr));  // A alone
  for (int64_t T : {(int64_t)1, (int64_t)67, (int64_t)100000})
    for (int32_t m : {1, 17, 257})
      for (int32_t n : {1, 65, 8200})
        for (int64_t P : {(int64_t)1, (int64_t)65, (int64_t)32640})
          for (int in = 0; in < 2; ++in) {
            for (int mode : {AGGF_PAIR_DIST, AGGF_PAIR_SQDIST, AGGF_PAIR_DOT})
              RUNS(aggf_pair_list_dist(p, (char*)p + 4096, p, (char*)p + 4096, i32, T, m, n, P, in, mode, d, nullptr));
            for (int od = 0; od <= in; ++od)
              for (int sel = 1; sel < 4; ++sel)
                for (int32_t deg : {0, 2, 32, 33, 8199})
                  RUNS(aggf_pair_list_pull(p, sel == 3 ? p : nullptr, p, (char*)p + 4096, i32, i32, i32, i32, i32, deg,
                                           8199 - deg, T, m, n, P, in, sel & 1 ? d : nullptr,
                                           sel & 2 ? d + 4096 : nullptr, od, nullptr));
          }
  // K9c / K9d box forms: the box's own refusals (NULL, a stride other than 0 or 3), the refusals and empty problems
  // of the open twins, and the same grid of plausible calls with either stride
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, nullptr, 3, d, nullptr));  // no box
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, p, 1, d, nullptr));        // stride
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, p, -3, d, nullptr));
  REFUSED(aggf_pair_list_dist_pbc(nullptr, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, p, 3, d, nullptr));
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, nullptr, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, p, 0, d, nullptr));
  REFUSED(aggf_pair_list_dist_pbc(p, p, p, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DOT, p, 3, d, nullptr));
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 2, AGGF_PAIR_DIST, p, 3, d, nullptr));
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, 3, p, 3, d, nullptr));
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, i32, -1, 3, 5, 9, 1, AGGF_PAIR_DIST, p, 3, d, nullptr));
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, i32, 7, 3, 5, (int64_t)1 << 31, 1, AGGF_PAIR_DIST, p, 3, d, nullptr));
  REFUSED(aggf_pair_list_dist_pbc(p, p, nullptr, nullptr, i32, INT64_MAX / 4, 3, 5, 1, 1, AGGF_PAIR_DIST, p, 3, d, nullptr));
  RUNS(aggf_pair_list_dist_pbc(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3, 5, 9, 1, AGGF_PAIR_DIST, p, 3, nullptr, nullptr));
  REFUSED(aggf_pair_list_pull_pbc(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, nullptr, 0, d, d, 1, nullptr));  // no box
  REFUSED(aggf_pair_list_pull_pbc(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, p, 2, d, d, 1, nullptr));        // stride
  REFUSED(aggf_pair_list_pull_pbc(nullptr, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, p, 3, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull_pbc(p, nullptr, p, p, nullptr, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, p, 3, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull_pbc(p, nullptr, p, p, i32, nullptr, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, p, 3, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull_pbc(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 0, p, 3, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull_pbc(p, nullptr, p, p, i32, i32, i32, i32, i32, -1, 2, 7, 3, 5, 9, 1, p, 3, d, d, 1, nullptr));
  REFUSED(aggf_pair_list_pull_pbc(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, INT64_MAX / 4, 3, 5, 9, 1, p, 3, d, d, 1, nullptr));
  RUNS(aggf_pair_list_pull_pbc(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 7, 3, 5, 0, 1, p, 0, nullptr, nullptr, 1, nullptr));
  RUNS(aggf_pair_list_pull_pbc(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, p, 0, nullptr, nullptr, 1, nullptr));  // neither output
  for (int64_t T : {(int64_t)1, (int64_t)67, (int64_t)100000})
    for (int32_t m : {1, 17, 257})
      for (int32_t n : {1, 65, 8200})
        for (int64_t P : {(int64_t)1, (int64_t)65, (int64_t)32640})
          for (int in = 0; in < 2; ++in)
            for (int32_t bs : {0, 3}) {
              for (int mode : {AGGF_PAIR_DIST, AGGF_PAIR_SQDIST, AGGF_PAIR_DOT})
                RUNS(aggf_pair_list_dist_pbc(p, (char*)p + 4096, p, (char*)p + 4096, i32, T, m, n, P, in, mode, p, bs, d, nullptr));
              for (int od = 0; od <= in; ++od)
                for (int sel = 1; sel < 4; ++sel)
                  for (int32_t deg : {0, 32, 33})
                    RUNS(aggf_pair_list_pull_pbc(p, sel == 3 ? p : nullptr, p, (char*)p + 4096, i32, i32, i32, i32, i32,
                                                 deg, 65 - deg, T, m, n, P, in, p, bs, sel & 1 ? d : nullptr,
                                                 sel & 2 ? d + 4096 : nullptr, od, nullptr));
            }
  // the `_cell` entries of K9c / K9d / K9e: no cell, a bad image selector, and the plans of box_stride 9 in both forms
  REFUSED(aggf_pair_list_dist_cell(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, nullptr, d, nullptr, AGGF_IMAGES_NEAREST));
  REFUSED(aggf_pair_list_dist_cell(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, p, d, nullptr, 2));
  REFUSED(aggf_pair_list_dist_cell(p, p, nullptr, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DIST, p, d, nullptr, 9));  // no stride here
  REFUSED(aggf_pair_list_dist_cell(p, p, p, nullptr, i32, 7, 3, 5, 9, 1, AGGF_PAIR_DOT, p, d, nullptr, AGGF_IMAGES_NEAREST));
  REFUSED(aggf_pair_list_pull_cell(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, nullptr, d, d, 1, nullptr, AGGF_IMAGES_NEAREST));
  REFUSED(aggf_pair_list_pull_cell(p, nullptr, p, p, i32, i32, i32, i32, i32, 2, 2, 7, 3, 5, 9, 1, p, d, d, 1, nullptr, -1));
  REFUSED(aggf_pair_min_cell(p, p, 7, 3, 5, 1, nullptr, 0, d, ws, WS, nullptr, AGGF_IMAGES_NEAREST));
  REFUSED(aggf_pair_min_cell(p, p, 7, 3, 5, 1, p, 0, d, ws, WS, nullptr, 3));
  REFUSED(aggf_pair_min_cell(p, p, 1000, 3, 5, 1, p, 0, d, ws, 0, nullptr, AGGF_IMAGES_NEAREST));  // split frames, no workspace
  RUNS(aggf_pair_min_cell(nullptr, nullptr, 0, 3, 5, 1, p, 0, nullptr, nullptr, 0, nullptr, AGGF_IMAGES_NEAREST));
  for (int images : {AGGF_IMAGES_BRICK, AGGF_IMAGES_NEAREST})
    for (int64_t T : {(int64_t)1, (int64_t)67, (int64_t)2000})
      for (int32_t n : {1, 65, 257})
        for (int in = 0; in < 2; ++in) {
          for (int mode : {AGGF_PAIR_DIST, AGGF_PAIR_SQDIST, AGGF_PAIR_DOT})
            RUNS(aggf_pair_list_dist_cell(p, (char*)p + 4096, p, (char*)p + 4096, i32, T, 17, n, 65, in, mode, p, d, nullptr, images));
          for (int od = 0; od <= in; ++od)
            for (int32_t deg : {0, 33})
              RUNS(aggf_pair_list_pull_cell(p, deg ? p : nullptr, p, (char*)p + 4096, i32, i32, i32, i32, i32, deg, 65 - deg, T,
                                            17, n, 65, in, p, d, d + 4096, od, nullptr, images));
          const size_t wm = aggf_pair_min_workspace_bytes(T, 17, n, in);
          if (wm <= WS) RUNS(aggf_pair_min_cell(p, (char*)p + 4096, T, 17, n, in, p, in, d, ws, wm, nullptr, images));
        }
  // K9e: the workspace query over the grid of shapes (overflowing ones included), refusals, empty shapes, and plausible
  // calls, open and under a box, with the queried workspace (one split and many)
  for (int64_t T : Ts)
    for (int32_t N : Ns) sink += aggf_pair_min_workspace_bytes(T, N / 16 + 1, N, 0) + aggf_pair_min_workspace_bytes(T, N, N, 1);
  sink += aggf_pair_min_workspace_bytes(INT64_MAX, INT32_MAX, INT32_MAX, 1) + aggf_pair_min_workspace_bytes(-1, 5, 300, 0);
  REFUSED(aggf_pair_min(nullptr, p, 7, 3, 5, 1, nullptr, 0, 0, d, ws, WS, nullptr));
  REFUSED(aggf_pair_min(p, nullptr, 7, 3, 5, 1, nullptr, 0, 0, d, ws, WS, nullptr));
  REFUSED(aggf_pair_min(p, p, 7, 3, 5, 1, nullptr, 0, 0, nullptr, ws, WS, nullptr));
  REFUSED(aggf_pair_min(p, p, 7, 3, 5, 2, nullptr, 0, 0, d, ws, WS, nullptr));           // dtype
  REFUSED(aggf_pair_min(p, p, 7, 3, 5, 1, p, 1, 0, d, ws, WS, nullptr));                 // stride
  REFUSED(aggf_pair_min(p, p, -1, 3, 5, 1, nullptr, 0, 0, d, ws, WS, nullptr));
  REFUSED(aggf_pair_min(p, p, 7, -3, 5, 1, nullptr, 0, 0, d, ws, WS, nullptr));
  REFUSED(aggf_pair_min(p, p, INT64_MAX / 4, 3, 5, 1, nullptr, 0, 0, d, ws, WS, nullptr));  // T n
  REFUSED(aggf_pair_min(p, p, 1000, 3, 5, 1, nullptr, 0, 0, d, ws, 0, nullptr));         // split frames, no workspace
  REFUSED(aggf_pair_min(p, p, 1000, 3, 5, 1, nullptr, 0, 0, d, nullptr, WS, nullptr));
  REFUSED(aggf_pair_min(p, p, 1000, 3, 5, 1, nullptr, 0, 0, d, (char*)ws + 4, WS - 4, nullptr));  // misaligned partials
  RUNS(aggf_pair_min(nullptr, nullptr, 0, 3, 5, 1, nullptr, 0, 0, nullptr, nullptr, 0, nullptr));
  RUNS(aggf_pair_min(nullptr, nullptr, 7, 0, 5, 0, p, 3, 1, nullptr, nullptr, 0, nullptr));
  RUNS(aggf_pair_min(p, p, 7, 3, 5, 1, nullptr, 0, 0, d, nullptr, 0, nullptr));          // one split: no workspace
  for (int64_t T : {(int64_t)1, (int64_t)67, (int64_t)2000, (int64_t)100000})
    for (int32_t m : {1, 17, 257, 8200})
      for (int32_t n : {1, 65, 256, 257, 8200})
        for (int in = 0; in < 2; ++in) {
          const size_t wm = aggf_pair_min_workspace_bytes(T, m, n, in);
          if (wm > WS) continue;
          for (int sq = 0; sq < 2; ++sq) {
            RUNS(aggf_pair_min(p, (char*)p + 4096, T, m, n, in, nullptr, 0, sq, d, ws, wm, nullptr));
            RUNS(aggf_pair_min(p, (char*)p + 4096, T, m, n, in, p, 3 * sq, sq, d, ws, wm, nullptr));
          }
        }
  // K10: the partials' size over the grid of shapes (absurd ones give 0), refusals (NULL pointers, bad dtype / width /
  // clip / order / form, rows or outputs that do not fit, slot tables that do not match the form, short or misaligned
  // workspaces), empty shapes, and plausible calls in every dtype / form / slot selection with the queried workspace
  for (int64_t T : Ts)
    for (int32_t N : Ns) sink += aggf_gbasis_sum_workspace_bytes(T, N, 10) + aggf_gbasis_sum_workspace_bytes(T, 600, N / 97 + 1);
  sink += aggf_gbasis_sum_workspace_bytes(INT64_MAX, INT32_MAX, INT32_MAX) + aggf_gbasis_sum_workspace_bytes(-1, 4, 4) +
          aggf_gbasis_sum_workspace_bytes(10, 0, 4);
  REFUSED(aggf_gbasis_expand(p, nullptr, nullptr, nullptr, 70, 10, 1, 1, 1.0, 1e-3, 0, 1, d, nullptr));      // centres
  REFUSED(aggf_gbasis_expand(nullptr, nullptr, p, nullptr, 70, 10, 1, 1, 1.0, 1e-3, 0, 1, d, nullptr));
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, 70, 10, 1, 1, 1.0, 1e-3, 0, 1, nullptr, nullptr));
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, 70, 10, 1, 1, 1.0, 1e-3, 0, 2, d, nullptr));            // dtype
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, 70, 0, 1, 1, 1.0, 1e-3, 0, 1, d, nullptr));             // n_basis
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, 70, 10, 1, 1, 0.0, 1e-3, 0, 1, d, nullptr));            // width
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, 70, 10, 1, 1, 1.0, -1.0, 0, 1, d, nullptr));            // clip
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, 70, 10, 1, 1, 1.0, 1e-3, -1, 1, d, nullptr));           // order
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, 70, 10, 1, 1, 1.0, 1e-3, 65, 1, d, nullptr));
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, -1, 10, 1, 1, 1.0, 1e-3, 0, 1, d, nullptr));
  REFUSED(aggf_gbasis_expand(p, nullptr, p, i32, 70, 10, 8, 4, 1.0, 1e-3, 0, 1, d, nullptr));                // 70 % 8
  REFUSED(aggf_gbasis_expand(p, nullptr, p, i32, 70, 10, 7, 0, 1.0, 1e-3, 0, 1, d, nullptr));                // n_slots
  REFUSED(aggf_gbasis_expand(p, nullptr, p, i32, 70, 1 << 20, 7, 1 << 20, 1.0, 1e-3, 0, 1, d, nullptr));     // row
  REFUSED(aggf_gbasis_expand(p, nullptr, p, nullptr, INT64_MAX / 4, 10, 1, 1, 1.0, 1e-3, 0, 1, d, nullptr)); // E n_basis
  RUNS(aggf_gbasis_expand(nullptr, nullptr, p, nullptr, 0, 10, 1, 1, 1.0, 0.0, 3, 0, nullptr, nullptr));
  REFUSED(aggf_gbasis_contract(nullptr, AGGF_GB_H_ELEM, p, p, nullptr, 70, 10, 1, 1, 1.0, 1e-3, 0, 1, d, nullptr));
  REFUSED(aggf_gbasis_contract(p, 3, p, p, nullptr, 70, 10, 1, 1, 1.0, 1e-3, 0, 1, d, nullptr));             // form
  REFUSED(aggf_gbasis_contract(p, AGGF_GB_H_ROW, p, p, nullptr, 70, 10, 7, 4, 1.0, 1e-3, 0, 1, d, nullptr)); // no table
  REFUSED(aggf_gbasis_contract(p, AGGF_GB_H_SLOT, p, p, nullptr, 70, 10, 7, 4, 1.0, 1e-3, 0, 1, d, nullptr));
  REFUSED(aggf_gbasis_contract(p, AGGF_GB_H_SLOT, p, p, i32, 70, 10, 8, 4, 1.0, 1e-3, 0, 1, d, nullptr));    // 70 % 8
  REFUSED(aggf_gbasis_contract(p, AGGF_GB_H_ROW, p, p, i32, 70, 1 << 20, 7, 1 << 20, 1.0, 1e-3, 0, 1, d, nullptr));
  REFUSED(aggf_gbasis_contract(p, AGGF_GB_H_ELEM, p, p, nullptr, 70, 10, 1, 1, 1.0, 1e-3, 0, 1, nullptr, nullptr));
  RUNS(aggf_gbasis_contract(nullptr, AGGF_GB_H_ELEM, nullptr, p, nullptr, 0, 10, 1, 1, 1.0, 1e-3, 2, 1, nullptr, nullptr));
  REFUSED(aggf_gbasis_sum(p, nullptr, p, i32, nullptr, 5, 10, 7, 4, 10, 1.0, 1e-3, 0, 1, d, ws, WS, nullptr));   // no start
  REFUSED(aggf_gbasis_sum(p, nullptr, p, nullptr, nullptr, 0, 10, 7, 4, 10, 1.0, 1e-3, 0, 1, d, ws, WS, nullptr));
  REFUSED(aggf_gbasis_sum(p, nullptr, p, i32, i32, 8, 10, 7, 4, 10, 1.0, 1e-3, 0, 1, d, ws, WS, nullptr));       // n_order > N
  REFUSED(aggf_gbasis_sum(p, nullptr, p, i32, i32, 5, 10, 7, 4, 10, 1.0, 1e-3, 0, 1, nullptr, ws, WS, nullptr));
  REFUSED(aggf_gbasis_sum(p, nullptr, p, i32, i32, 5, 10, 7, 4, 10, 1.0, 1e-3, 0, 1, d, ws, 0, nullptr));
  REFUSED(aggf_gbasis_sum(p, nullptr, p, i32, i32, 5, 10, 7, 4, 10, 1.0, 1e-3, 0, 1, d, (char*)ws + 4, WS - 4, nullptr));
  REFUSED(aggf_gbasis_sum(p, nullptr, p, i32, i32, 5, 10, 7, 1 << 24, 10, 1.0, 1e-3, 0, 1, d, ws, WS, nullptr));  // grid.y
  REFUSED(aggf_gbasis_sum(p, nullptr, p, nullptr, nullptr, 0, INT64_MAX / 2, 7, 1, 10, 1.0, 1e-3, 0, 1, d, ws, WS, nullptr));
  RUNS(aggf_gbasis_sum(nullptr, nullptr, p, nullptr, nullptr, 0, 0, 7, 1, 10, 1.0, 1e-3, 0, 1, d, nullptr, 0, nullptr));  // zeros
  for (int64_t T : {(int64_t)1, (int64_t)67, (int64_t)2000, (int64_t)100000})
    for (int32_t N : {1, 65, 257, 1024})
      for (int32_t nb : {1, 10, 17})
        for (int dt = 0; dt < 2; ++dt)
          for (int32_t q : {0, 3}) {
            const int32_t n_slots = N / 2 + 1;
            RUNS(aggf_gbasis_expand(p, nullptr, p, nullptr, T * N, nb, 1, 1, 1.3, 1e-3, q, dt, d, nullptr));
            RUNS(aggf_gbasis_expand(p, p, p, i32, T * N, nb, N, n_slots, 1.3, 0.0, q, dt, d, nullptr));
            RUNS(aggf_gbasis_contract(p, AGGF_GB_H_ELEM, p, p, nullptr, T * N, nb, 1, 1, 1.3, 1e-3, q, dt, d, nullptr));
            RUNS(aggf_gbasis_contract(p, AGGF_GB_H_ROW, p, p, i32, T * N, nb, N, n_slots, 1.3, 1e-3, q, dt, d, nullptr));
            RUNS(aggf_gbasis_contract(p, AGGF_GB_H_SLOT, p, p, i32, T * N, nb, N, n_slots, 1.3, 1e-3, q, dt, d, nullptr));
            RUNS(aggf_gbasis_contract(p, AGGF_GB_H_SLOT, p, p, nullptr, T * N, nb, N, 1, 1.3, 1e-3, q, dt, d, nullptr));
            const size_t wg = aggf_gbasis_sum_workspace_bytes(T, n_slots, nb), w1 = aggf_gbasis_sum_workspace_bytes(T, 1, nb);
            if (wg <= WS) RUNS(aggf_gbasis_sum(p, p, p, i32, i32, N, T, N, n_slots, nb, 1.3, 1e-3, q, dt, d, ws, wg, nullptr));
            if (w1 <= WS) RUNS(aggf_gbasis_sum(p, nullptr, p, nullptr, nullptr, 0, T, N, 1, nb, 1.3, 1e-3, q, dt, d, ws, w1, nullptr));
          }
  // K11: the count buffers' size over the grid of shapes (overflowing ones give 0), refusals (NULL box or pointers, bad
  // stride / dtype / rounds / form, rounds without tables, an N beyond the LDS form, short or misaligned workspaces),
  // empty shapes, and plausible calls in every dtype / form / stride with the queried workspace, in place and not
  const int32_t lds_max = aggf_make_whole_lds_max_sites();
  for (int64_t T : Ts)
    for (int32_t N : Ns)
      for (int32_t R : {0, 1, 16}) sink += aggf_make_whole_workspace_bytes(T, N, R, 0) + aggf_make_whole_workspace_bytes(T, N, R, 1);
  sink += aggf_make_whole_workspace_bytes(INT64_MAX, INT32_MAX, 16, 1) + aggf_make_whole_workspace_bytes(-1, 5, 0, 0) +
          aggf_make_whole_workspace_bytes(5, 5, -1, 0);
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, nullptr, 0, d, nullptr, ws, WS, 0, nullptr));        // no box
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, p, 1, d, nullptr, ws, WS, 0, nullptr));              // stride
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, p, -3, d, nullptr, ws, WS, 0, nullptr));
  REFUSED(aggf_make_whole(p, 7, 5, 2, i32, i32, 2, p, 3, d, nullptr, ws, WS, 0, nullptr));              // dtype
  REFUSED(aggf_make_whole(nullptr, 7, 5, 1, i32, i32, 2, p, 3, d, nullptr, ws, WS, 0, nullptr));
  REFUSED(aggf_make_whole(p, 7, 5, 1, nullptr, i32, 2, p, 3, d, nullptr, ws, WS, 0, nullptr));
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, p, 3, nullptr, nullptr, ws, WS, 0, nullptr));
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, nullptr, 2, p, 3, d, nullptr, ws, WS, 0, nullptr));          // rounds, no tables
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, -1, p, 3, d, nullptr, ws, WS, 0, nullptr));
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 17, p, 3, d, nullptr, ws, WS, 0, nullptr));             // depth >= 2^16
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, p, 3, d, nullptr, ws, WS, 3, nullptr));              // form
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, p, 3, d, nullptr, ws, WS, -1, nullptr));
  REFUSED(aggf_make_whole(p, -1, 5, 1, i32, i32, 2, p, 3, d, nullptr, ws, WS, 0, nullptr));
  REFUSED(aggf_make_whole(p, 7, -5, 1, i32, i32, 2, p, 3, d, nullptr, ws, WS, 0, nullptr));
  REFUSED(aggf_make_whole(p, INT64_MAX / 4, 5, 1, i32, i32, 2, p, 3, d, nullptr, ws, WS, 0, nullptr));  // T N
  REFUSED(aggf_make_whole(p, 2, lds_max + 1, 1, i32, i32, 2, p, 3, d, nullptr, ws, WS, 1, nullptr));    // beyond the LDS form
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, p, 3, d, nullptr, ws, 0, 2, nullptr));               // global, no workspace
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, p, 3, d, nullptr, nullptr, WS, 2, nullptr));
  REFUSED(aggf_make_whole(p, 7, 5, 1, i32, i32, 2, p, 3, d, nullptr, (char*)ws + 2, WS - 2, 2, nullptr));
  REFUSED(aggf_make_whole(p, 2, lds_max + 1, 0, i32, i32, 2, p, 0, d, nullptr, ws, 64, 0, nullptr));    // auto goes global
  RUNS(aggf_make_whole(nullptr, 0, 5, 1, nullptr, nullptr, 0, p, 3, nullptr, nullptr, nullptr, 0, 0, nullptr));
  RUNS(aggf_make_whole(nullptr, 7, 0, 0, nullptr, nullptr, 3, p, 0, nullptr, nullptr, nullptr, 0, 2, nullptr));
  for (int64_t T : {(int64_t)1, (int64_t)67, (int64_t)2000, (int64_t)100000})
    for (int32_t N : {1, 65, 1366, 4096, lds_max, lds_max + 1, 20000})
      for (int dt = 0; dt < 2; ++dt)
        for (int32_t R : {0, 1, 9})
          for (int32_t bs : {0, 3})
            for (int form = 0; form < 3; ++form) {
              if (form == 1 && N > lds_max) continue;
              const size_t wm = aggf_make_whole_workspace_bytes(T, N, R, dt);
              if (wm > WS) continue;
              RUNS(aggf_make_whole(p, T, N, dt, i32, i32, R, p, bs, (char*)p + 8192, i32 + 4096, ws, wm, form, nullptr));
              RUNS(aggf_make_whole(p, T, N, dt, i32, R ? i32 : nullptr, R, p, bs, p, nullptr, ws, wm, form, nullptr));
            }
  free(raw);
  printf("%d calls, %d unexpected statuses\n", n_calls, n_bad);
  return n_bad ? 1 : 0;
}
