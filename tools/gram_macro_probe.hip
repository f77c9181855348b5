// The forms of the macro-tile Gram kernel (gram_tile_dma_kernel_x2, aggforce_amd/csrc/aggf_gram.hip) side by side with
// the single-tile kernel, on one set of float64 frames: ring depth, frames per stage, DMA placement and the barrier
// stagger of waves 8-15.  Every form is checked against the single-tile route's G before it is timed.  The library
// compiles MacroShipped only; this probe instantiates the others.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/gram_macro_probe.hip aggforce_amd/csrc/aggf_util.hip \
//       -o gram_macro_probe -ldl && ./gram_macro_probe [tile_rows = 32] [frames = 200003] [repeats = 3]
// One JSON line per form: ms = best of the repeats (table + tile kernel + reducer), rel_err against the single-tile G.
#include "../aggforce_amd/csrc/aggf_gram.hip"

#include <vector>

struct Probe {
  const double* F;
  int64_t T;
  int32_t N;
  GramPlan plan;
  char* ws;
  double* G;
  std::vector<double> ref, got;
  double scale;
  int reps;
  hipEvent_t e0, e1;
};

template <typename FORM>
static void run_form(Probe& pr, const char* name) {
  float best = 1e30f;
  int rc = 0;
  for (int rep = 0; rep < pr.reps + 1 && rc == 0; ++rep) {
    hipEventRecord(pr.e0);
    rc = launch_gram_macro<FORM>(pr.F, pr.T, (int64_t)pr.N * 3, pr.plan, pr.ws, pr.G, pr.N, 0, nullptr);
    hipEventRecord(pr.e1);
    if (hipEventSynchronize(pr.e1) != hipSuccess) rc = -1;
    float ms = 0.f;
    hipEventElapsedTime(&ms, pr.e0, pr.e1);
    if (rep > 0 && ms < best) best = ms;
  }
  double err = -1.0;
  if (rc == 0 && hipMemcpy(pr.got.data(), pr.G, pr.got.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
    err = 0.0;
    for (size_t i = 0; i < pr.got.size(); ++i) {
      const double d = fabs(pr.got[i] - pr.ref[i]);
      if (!(d <= err)) err = d;  // (a NaN sticks)
    }
    err /= pr.scale;
  }
  printf("{\"form\": \"%s\", \"slots\": %d, \"frames_per_stage\": %d, \"ahead\": %d, \"burst\": %s, \"stagger\": %s, \"rc\": %d, "
         "\"ksplit\": %d, \"ms\": %.3f, \"rel_err_vs_single\": %.3e}\n",
         name, FORM::NBUF, FORM::KB, FORM::AHEAD, FORM::BURST ? "true" : "false", FORM::STAGGER ? "true" : "false", rc,
         pr.plan.ksplit, best, err);
  fflush(stdout);
}

int main(int argc, char** argv) {
  const int nt1 = argc > 1 ? atoi(argv[1]) : 32;
  const int64_t T = argc > 2 ? atoll(argv[2]) : 200003;
  Probe pr;
  pr.reps = argc > 3 ? atoi(argv[3]) : 3;
  pr.T = T;
  pr.N = nt1 * TILE;
  const int32_t N = pr.N;
  double* F;
  if (hipMalloc(&F, (size_t)T * N * 3 * 8) != hipSuccess || hipMalloc(&pr.G, (size_t)N * N * 8) != hipSuccess) {
    printf("{\"error\": \"hipMalloc\"}\n");
    return 1;
  }
  pr.F = F;
  aggf_synth_normal(F, T, N, AGGF_F64, 1, 0, 0.0, 30.0, 0.0, nullptr);
  const size_t need = aggf_gram_workspace_bytes(T, N, N, AGGF_F64, AGGF_F64, 0);
  if (hipMalloc(&pr.ws, need) != hipSuccess) return 1;
  hipEventCreate(&pr.e0);
  hipEventCreate(&pr.e1);
  pr.ref.resize((size_t)N * N);
  pr.got.resize((size_t)N * N);

  // the single-tile kernel through the library's own route
  setenv("AGGF_GRAM_ROUTE", "single", 1);
  float best = 1e30f;
  int rc = 0;
  for (int rep = 0; rep < pr.reps + 1 && rc == 0; ++rep) {
    hipEventRecord(pr.e0);
    rc = aggf_gram(F, T, N, AGGF_F64, AGGF_F64, nullptr, nullptr, N, pr.G, 0, pr.ws, need, nullptr);
    hipEventRecord(pr.e1);
    if (hipEventSynchronize(pr.e1) != hipSuccess) rc = -1;
    float ms = 0.f;
    hipEventElapsedTime(&ms, pr.e0, pr.e1);
    if (rep > 0 && ms < best) best = ms;
  }
  unsetenv("AGGF_GRAM_ROUTE");
  if (rc != 0 || hipMemcpy(pr.ref.data(), pr.G, pr.ref.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) {
    printf("{\"error\": \"single-tile route\", \"rc\": %d}\n", rc);
    return 1;
  }
  pr.scale = 0.0;
  for (double x : pr.ref) pr.scale = fabs(x) > pr.scale ? fabs(x) : pr.scale;
  printf("{\"form\": \"single-tile kernel (gram_tile_dma_kernel)\", \"tile_rows\": %d, \"frames\": %lld, \"rc\": %d, \"ms\": %.3f}\n", nt1,
         (long long)T, rc, best);
  fflush(stdout);

  if (make_plan({T, N, N, AGGF_F64, AGGF_F64, false}, need, &pr.plan) != 0 || !pr.plan.macro) {
    printf("{\"error\": \"no macro-tile plan for %d tile rows\"}\n", nt1);
    return 1;
  }
  run_form<MacroForm<3, 4, 2, false, false>>(pr, "3 slots x 4 frames");
  run_form<MacroForm<4, 4, 3, false, false>>(pr, "4 slots x 4 frames");
  run_form<MacroForm<3, 4, 2, true, true>>(pr, "3 slots x 4 frames, stagger, pieces behind the barrier");
  run_form<MacroForm<4, 4, 2, false, true>>(pr, "4 slots x 4 frames, stagger, two stages ahead");
  run_form<MacroForm<4, 4, 3, true, true>>(pr, "4 slots x 4 frames, stagger, pieces behind the barrier");
  run_form<MacroForm<3, 4, 2, true, false>>(pr, "3 slots x 4 frames, pieces behind the barrier");
  run_form<MacroForm<2, 8, 1, false, false, 3>>(pr, "2 slots x 8 frames, pieces beside groups 0-2 of 6");
  run_form<MacroForm<2, 8, 1, false, false, 2>>(pr, "2 slots x 8 frames, pieces beside groups 0-1");
  run_form<MacroForm<2, 8, 1, false, false, 4>>(pr, "2 slots x 8 frames, pieces beside groups 0-3");
  run_form<MacroForm<2, 8, 1, false, false, 5>>(pr, "2 slots x 8 frames, pieces beside groups 0-4");
  run_form<MacroForm<4, 4, 2, false, false>>(pr, "4 slots x 4 frames, two stages ahead");
  return 0;
}
