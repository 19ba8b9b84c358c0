// Read rate of k_obs_overlap<13> (dse_overlap.hip) on one register, beside launch_dot (dse_kernels.hip)
// on the same buffers in the same process: the yardstick DESIGN.md §4.5e quotes (not a pass/fail bound).
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I quantumsimulations_amd/csrc -I include \
//         tools/probe_overlap.cpp quantumsimulations_amd/csrc/dse_overlap.hip \
//         quantumsimulations_amd/csrc/dse_kernels.hip -o tools/bin/probe_overlap
//   probe_overlap [n = 26] [reps = 7]
//
// Prints one JSON line per K in {1, 4}: the best and median time over reps runs after one warm-up of
// the overlap kernel (one launch: psi once, K references) and of K launch_dot calls (psi K times, K
// references: what the engine had before), TB/s of the algorithmic (1 + K) 16 B per amplitude for
// both, and the kernel's Re <phi_0|psi> and ||psi||^2 against launch_dot's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

__global__ void k_fill(double2* v, size_t n, double a, double b) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double x = (double)(i % 1021) * (1.0 / 1021.0);
    v[i] = make_double2(a * (x - 0.5), b * (0.25 - x * x));
  }
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 26;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 7;
  constexpr int L = 13, KMAX = 4;
  if (n < L || n > 28 || reps < 1 || reps > 100) {
    std::fprintf(stderr, "usage: probe_overlap [n 13..28] [reps 1..100]\n");
    return 1;
  }
  const size_t dim = size_t(1) << n, bytes = dim * sizeof(double2);
  const int tiles = 1 << (n - L), dot_blocks = 2048;
  double2* psi = nullptr;
  double2* ref[KMAX];
  CK(hipMalloc(&psi, bytes));
  hipLaunchKernelGGL(k_fill, dim3(2048), dim3(256), 0, 0, psi, dim, 1.0, 0.7);
  for (int k = 0; k < KMAX; ++k) {
    CK(hipMalloc(&ref[k], bytes));
    hipLaunchKernelGGL(k_fill, dim3(2048), dim3(256), 0, 0, ref[k], dim, 0.3 + k, 1.1 - 0.2 * k);
  }
  const double2** d_tab = nullptr;
  CK(hipMalloc(&d_tab, dse::kMaxOverlapRefs * sizeof(double2*)));
  CK(hipMemset(d_tab, 0, dse::kMaxOverlapRefs * sizeof(double2*)));
  CK(hipMemcpy(d_tab, ref, KMAX * sizeof(double2*), hipMemcpyHostToDevice));
  std::vector<int2> items(tiles);
  for (int t = 0; t < tiles; ++t) items[t] = make_int2(0, t);
  int2* d_items = nullptr;
  CK(hipMalloc(&d_items, tiles * sizeof(int2)));
  CK(hipMemcpy(d_items, items.data(), tiles * sizeof(int2), hipMemcpyHostToDevice));
  dse::DevProb* d_prob = nullptr;
  CK(hipMalloc(&d_prob, sizeof(dse::DevProb)));
  const int S = dse::overlap_stride(KMAX);
  double *d_part = nullptr, *d_dot = nullptr;
  CK(hipMalloc(&d_part, (size_t)tiles * S * sizeof(double)));
  CK(hipMalloc(&d_dot, (size_t)2 * dot_blocks * sizeof(double)));
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipDeviceSynchronize());
  int bad = 0;
  for (int K : {1, KMAX}) {
    dse::DevProb P;
    std::memset(&P, 0, sizeof(P));
    P.buf[0] = psi;
    P.n = n, P.L = L, P.tbl = n - L;
    P.ovl_refs = d_tab;
    P.ovl_k = K;
    CK(hipMemcpy(d_prob, &P, sizeof(P), hipMemcpyHostToDevice));
    std::vector<float> tk, td;
    for (int r = 0; r <= reps; ++r) {  // r = 0: warm-up of both
      float ms = 0.f;
      CK(hipEventRecord(e0, st));
      CK(dse::launch_obs_overlap(L, d_prob, d_items, tiles, 0, d_part, S, st));
      CK(hipEventRecord(e1, st));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r) tk.push_back(ms);
      CK(hipEventRecord(e0, st));
      for (int k = K - 1; k >= 0; --k) CK(dse::launch_dot(psi, ref[k], dim, d_dot, dot_blocks, st));
      CK(hipEventRecord(e1, st));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r) td.push_back(ms);
    }
    std::vector<double> hp((size_t)tiles * S), hd(2 * dot_blocks);
    CK(hipMemcpy(hp.data(), d_part, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hd.data(), d_dot, hd.size() * sizeof(double), hipMemcpyDeviceToHost));
    double re = 0.0, n2 = 0.0, dre = 0.0, dn2 = 0.0;
    for (int t = 0; t < tiles; ++t) re += hp[(size_t)t * S], n2 += hp[(size_t)t * S + S - 2];
    for (int b = 0; b < dot_blocks; ++b) dre += hd[2 * b], dn2 += hd[2 * b + 1];  // launch_dot(psi, ref[0]) ran last
    const double err = std::max(std::fabs(re - dre) / std::fabs(dn2), std::fabs(n2 - dn2) / std::fabs(dn2));
    bad += !(err < 1e-12);
    std::sort(tk.begin(), tk.end());
    std::sort(td.begin(), td.end());
    const double tb = (1.0 + K) * (double)bytes / 1e12, tb_dot = 2.0 * K * (double)bytes / 1e12;
    std::printf("{\"n\": %d, \"K\": %d, \"reps\": %d, \"overlap_ms_best\": %.4f, \"overlap_ms_median\": %.4f, "
                "\"dot_ms_best\": %.4f, \"dot_ms_median\": %.4f, \"overlap_TBps_best\": %.3f, \"overlap_TBps_median\": %.3f, "
                "\"dot_TBps_of_same_bytes_best\": %.3f, \"dot_TBps_of_its_own_bytes_best\": %.3f, \"check_rel_err\": %.3e}\n",
                n, K, reps, tk.front(), tk[tk.size() / 2], td.front(), td[td.size() / 2], tb / (tk.front() * 1e-3),
                tb / (tk[tk.size() / 2] * 1e-3), tb / (td.front() * 1e-3), tb_dot / (td.front() * 1e-3), err);
  }
  return bad ? 3 : 0;
}
