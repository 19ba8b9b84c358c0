// Store rate of k_product_state (dse_init.hip) beside hipMemsetAsync of the same buffer in the same
// process: the yardstick DESIGN.md §4.5c quotes (not a pass/fail bound).
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I quantumsimulations_amd/csrc -I include \
//         tools/probe_product.cpp quantumsimulations_amd/csrc/dse_init.hip -o tools/bin/probe_product
//   probe_product [n = 28] [reps = 5]
//
// Prints one JSON line: the best and median time of each over reps runs after one warm-up, GB/s of
// the 16 * 2^n bytes written, and one spot check of the kernel's output against the host product.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dse_internal.h"

#define CK(x)                                                              \
  do {                                                                     \
    hipError_t e_ = (x);                                                   \
    if (e_ != hipSuccess) {                                                \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      std::exit(2);                                                        \
    }                                                                      \
  } while (0)

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 28;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
  if (n < 1 || n > 30 || reps < 1 || reps > 100) {
    std::fprintf(stderr, "usage: probe_product [n 1..30] [reps 1..100]\n");
    return 1;
  }
  const size_t dim = size_t(1) << n, bytes = dim * sizeof(double2);
  std::vector<double> amp(4 * n);
  for (int i = 0; i < 4 * n; ++i) amp[i] = std::cos(0.37 * i + 0.1) * (0.9 + 0.01 * i);
  double2* psi = nullptr;
  double* d_amp = nullptr;
  CK(hipMalloc(&psi, bytes));
  CK(hipMalloc(&d_amp, amp.size() * sizeof(double)));
  CK(hipMemcpy(d_amp, amp.data(), amp.size() * sizeof(double), hipMemcpyHostToDevice));
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> tk, tm;
  for (int r = 0; r <= reps; ++r) {  // r = 0: warm-up of both
    float ms = 0.f;
    CK(hipEventRecord(e0, st));
    CK(hipMemsetAsync(psi, 0, bytes, st));
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (r) tm.push_back(ms);
    CK(hipEventRecord(e0, st));
    CK(dse::launch_product_state(psi, d_amp, n, n, 0, st));
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (r) tk.push_back(ms);
  }
  // spot check: a few amplitudes against the host product
  double worst = 0.0;
  for (size_t x : {size_t(0), dim - 1, dim / 3, (dim / 7) | 1}) {
    double2 got;
    CK(hipMemcpy(&got, psi + x, sizeof(double2), hipMemcpyDeviceToHost));
    std::complex<double> ref(1.0, 0.0);
    for (int b = 0; b < n; ++b) {
      const int v = (int)((x >> b) & 1);
      ref *= std::complex<double>(amp[4 * b + 2 * v], amp[4 * b + 2 * v + 1]);
    }
    worst = std::max(worst, std::abs(std::complex<double>(got.x, got.y) - ref) / std::abs(ref));
  }
  std::sort(tk.begin(), tk.end());
  std::sort(tm.begin(), tm.end());
  const double gb = (double)bytes / 1e9;
  std::printf("{\"n\": %d, \"bytes\": %zu, \"reps\": %d, \"product_ms_best\": %.4f, \"product_ms_median\": %.4f, "
              "\"memset_ms_best\": %.4f, \"memset_ms_median\": %.4f, \"product_GBps_best\": %.1f, "
              "\"product_GBps_median\": %.1f, \"memset_GBps_best\": %.1f, \"memset_GBps_median\": %.1f, "
              "\"spot_check_rel_err\": %.3e}\n",
              n, bytes, reps, tk.front(), tk[tk.size() / 2], tm.front(), tm[tm.size() / 2], gb / (tk.front() * 1e-3),
              gb / (tk[tk.size() / 2] * 1e-3), gb / (tm.front() * 1e-3), gb / (tm[tm.size() / 2] * 1e-3), worst);
  CK(hipFree(psi));
  CK(hipFree(d_amp));
  return worst < 1e-13 ? 0 : 3;
}
