// Time and byte rate of k_obs_strings<13> (dse_strings.hip) on one register, beside k_obs_pairs<13>
// (dse_pairs.hip) on the same register in the same process, per pair: the yardstick DESIGN.md §4.5g
// quotes (not a pass/fail bound).  The pair kernel does the same partner reads for fixed masks.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I quantumsimulations_amd/csrc -I include \
//         tools/probe_strings.cpp quantumsimulations_amd/csrc/dse_strings.hip \
//         quantumsimulations_amd/csrc/dse_pairs.hip -o tools/bin/probe_strings
//   probe_strings [n = 26] [reps = 7]
//
// Prints one JSON line for the pair kernel (all n (n - 1) / 2 pairs: time, time per pair) and one per
// class and K in {1, 8, 64}: the best and median time over reps runs after one warm-up, TB/s of the
// bytes the class moves (16 B per amplitude once, plus 16 B per amplitude and cross-tile string), the
// time per string over the pair kernel's time per pair, and a check of string 0 of the cross-tile class
// (Ix_0 Ix_13 = (Re ZQ + Re DQ) / 2 of the pair (0, 13)) against the pair kernel's sums.
//   diagonal     Iz Iz on two bits anywhere in the register
//   in-tile      Ix Ix on two bits below 13 (thread and row bits)
//   cross-tile   Ix on a bit below 13 and Ix on a bit at or above 13
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
  constexpr int L = 13, KMAX = dse::kMaxOpStrings;
  if (n < L + 1 || n > 28 || reps < 1 || reps > 100) {
    std::fprintf(stderr, "usage: probe_strings [n 14..28] [reps 1..100]\n");
    return 1;
  }
  const size_t dim = size_t(1) << n, bytes = dim * sizeof(double2);
  const int tiles = 1 << (n - L), np = n * (n - 1) / 2;
  double2* psi = nullptr;
  CK(hipMalloc(&psi, bytes));
  hipLaunchKernelGGL(k_fill, dim3(2048), dim3(256), 0, 0, psi, dim, 1.0, 0.7);
  std::vector<int2> items(tiles);
  for (int t = 0; t < tiles; ++t) items[t] = make_int2(0, t);
  int2* d_items = nullptr;
  CK(hipMalloc(&d_items, tiles * sizeof(int2)));
  CK(hipMemcpy(d_items, items.data(), tiles * sizeof(int2), hipMemcpyHostToDevice));
  dse::DevProb* d_prob = nullptr;
  CK(hipMalloc(&d_prob, sizeof(dse::DevProb)));
  dse::StringEntry* d_tab = nullptr;
  CK(hipMalloc(&d_tab, KMAX * sizeof(dse::StringEntry)));
  const int S = dse::string_stride(KMAX), SP = dse::pair_stride(n);
  double *d_part = nullptr, *d_pair = nullptr;
  CK(hipMalloc(&d_part, (size_t)tiles * S * sizeof(double)));
  CK(hipMalloc(&d_pair, (size_t)tiles * SP * sizeof(double)));
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  dse::DevProb P;
  std::memset(&P, 0, sizeof(P));
  P.buf[0] = psi;
  P.n = n, P.L = L, P.tbl = n - L;
  P.str_tab = d_tab;
  CK(hipMemcpy(d_prob, &P, sizeof(P), hipMemcpyHostToDevice));
  CK(hipDeviceSynchronize());

  // the yardstick: every pair of the register in one launch
  std::vector<float> tp;
  for (int r = 0; r <= reps; ++r) {  // r = 0: warm-up
    float ms = 0.f;
    CK(hipEventRecord(e0, st));
    CK(dse::launch_obs_pairs(L, d_prob, d_items, tiles, 0, d_pair, SP, st));
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (r) tp.push_back(ms);
  }
  std::sort(tp.begin(), tp.end());
  const double pair_ms = tp.front() / np;
  std::vector<double> hpair((size_t)tiles * SP);
  CK(hipMemcpy(hpair.data(), d_pair, hpair.size() * sizeof(double), hipMemcpyDeviceToHost));
  double zq = 0.0, dq = 0.0, pn2 = 0.0;
  const int p013 = dse::pair_index(0, L);
  for (int t = 0; t < tiles; ++t) {
    zq += hpair[(size_t)t * SP + 5 * p013 + 1];
    dq += hpair[(size_t)t * SP + 5 * p013 + 3];
    pn2 += hpair[(size_t)t * SP + 5 * np];
  }
  std::printf("{\"n\": %d, \"kernel\": \"k_obs_pairs<13>\", \"pairs\": %d, \"reps\": %d, \"ms_best\": %.4f, \"ms_median\": %.4f, "
              "\"ms_per_pair_best\": %.5f}\n", n, np, reps, tp.front(), tp[tp.size() / 2], pair_ms);

  int bad = 0;
  const char* names[3] = {"diagonal", "in-tile", "cross-tile"};
  for (int cls = 0; cls < 3; ++cls) {
    std::vector<dse::StringEntry> tab(KMAX);
    for (int k = 0; k < KMAX; ++k) {
      dse::StringEntry e{0, 0, 0, 0, 0.25, 0.0};
      const int a = k % L, b = (a + 1 + (k / L) % (L - 1)) % L;  // two distinct bits below L
      if (cls == 0)
        e.zm = (uint64_t(1) << (k % n)) | (uint64_t(1) << ((k % n + 1 + (k / n) % (n - 1)) % n));
      else if (cls == 1)
        e.xm = (uint64_t(1) << a) | (uint64_t(1) << b);
      else
        e.xm = (uint64_t(1) << a) | (uint64_t(1) << (L + (k / L + k) % (n - L)));
      tab[k] = e;
    }
    CK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(dse::StringEntry), hipMemcpyHostToDevice));
    for (int K : {1, 8, KMAX}) {
      P.str_k = K;
      CK(hipMemcpy(d_prob, &P, sizeof(P), hipMemcpyHostToDevice));
      std::vector<float> tk;
      for (int r = 0; r <= reps; ++r) {
        float ms = 0.f;
        CK(hipEventRecord(e0, st));
        CK(dse::launch_obs_strings(L, d_prob, d_items, tiles, 0, d_part, S, st));
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r) tk.push_back(ms);
      }
      std::sort(tk.begin(), tk.end());
      std::vector<double> hp((size_t)tiles * S);
      CK(hipMemcpy(hp.data(), d_part, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
      double re = 0.0, n2 = 0.0;
      for (int t = 0; t < tiles; ++t) re += hp[(size_t)t * S], n2 += hp[(size_t)t * S + S - 2];
      double err = std::fabs(n2 - pn2) / pn2;
      if (cls == 2) err = std::max(err, std::fabs(re - 0.5 * (zq + dq)) / pn2);  // string 0: Ix_0 Ix_13
      bad += !(err < 1e-12);
      const double tb = (1.0 + (cls == 2 ? K : 0)) * (double)bytes / 1e12;
      std::printf("{\"n\": %d, \"kernel\": \"k_obs_strings<13>\", \"class\": \"%s\", \"K\": %d, \"reps\": %d, \"ms_best\": %.4f, "
                  "\"ms_median\": %.4f, \"TBps_best\": %.3f, \"TBps_median\": %.3f, \"ms_per_string_best\": %.5f, "
                  "\"per_string_over_per_pair\": %.3f, \"check_rel_err\": %.3e}\n",
                  n, names[cls], K, reps, tk.front(), tk[tk.size() / 2], tb / (tk.front() * 1e-3),
                  tb / (tk[tk.size() / 2] * 1e-3), tk.front() / K, tk.front() / K / pair_ms, err);
    }
  }
  return bad ? 3 : 0;
}
