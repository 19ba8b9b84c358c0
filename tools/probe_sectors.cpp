// Time of k_obs_sectors<13> (dse_sectors.hip) on one register, beside k_obs_strings<13>
// (dse_strings.hip) with as many diagonal strings on the same register in the same process: the
// yardstick DESIGN.md §4.5h quotes (not a pass/fail bound).  The strings' K = 1 time is one read of the
// state; their per-string time prices the alternative to a set of B bins, one selection pass per bin.
//
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I quantumsimulations_amd/csrc -I include \
//         tools/probe_sectors.cpp quantumsimulations_amd/csrc/dse_sectors.hip \
//         quantumsimulations_amd/csrc/dse_strings.hip -o tools/bin/probe_sectors
//   probe_sectors [n = 26] [reps = 7]
//
// Prints one JSON line per K in {1, 4, 16} for the strings (diagonal: Iz Iz on two bits) and one per
// kind of counted mask and K: the best and median time over reps runs after one warm-up, the time per
// set, the same over the strings' time per string, and a check: every set's bins sum to ||psi||^2 and
// the mean of the first set, sum_j j bin_j, equals sum_b (||psi||^2 / 2 - <Iz_b> sum) over its bits
// from one-bit diagonal strings.
//   thread bits      m within the 9 thread bits (set k counts 3 + k % 7 of them)
//   above the tile   m within the bits at or above 13
//   all bits         m = every bit of the register (n + 1 bins)
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
  constexpr int L = 13, KMAX = dse::kMaxSectorSets;
  if (n < L + 1 || n > 28 || reps < 1 || reps > 100) {
    std::fprintf(stderr, "usage: probe_sectors [n 14..28] [reps 1..100]\n");
    return 1;
  }
  const size_t dim = size_t(1) << n, bytes = dim * sizeof(double2);
  const int tiles = 1 << (n - L);
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
  const int KS = 32;  // strings: up to 16 for the timing, n <= 28 one-bit strings for the check
  dse::StringEntry* d_str = nullptr;
  CK(hipMalloc(&d_str, KS * sizeof(dse::StringEntry)));
  dse::SectorEntry* d_sec = nullptr;
  CK(hipMalloc(&d_sec, KMAX * sizeof(dse::SectorEntry)));
  const int SS = dse::string_stride(KS), SU = dse::sector_stride(KMAX * (n + 1));
  double *d_ps = nullptr, *d_pu = nullptr;
  CK(hipMalloc(&d_ps, (size_t)tiles * SS * sizeof(double)));
  CK(hipMalloc(&d_pu, (size_t)tiles * SU * sizeof(double)));
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  dse::DevProb P;
  std::memset(&P, 0, sizeof(P));
  P.buf[0] = psi;
  P.n = n, P.L = L, P.tbl = n - L;
  P.str_tab = d_str;
  P.sec_tab = d_sec;
  CK(hipDeviceSynchronize());

  auto time_strings = [&](int K, std::vector<float>& tk) {
    P.str_k = K;
    CK(hipMemcpy(d_prob, &P, sizeof(P), hipMemcpyHostToDevice));
    for (int r = 0; r <= reps; ++r) {  // r = 0: warm-up
      float ms = 0.f;
      CK(hipEventRecord(e0, st));
      CK(dse::launch_obs_strings(L, d_prob, d_items, tiles, 0, d_ps, SS, st));
      CK(hipEventRecord(e1, st));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r) tk.push_back(ms);
    }
    std::sort(tk.begin(), tk.end());
  };

  // one-bit diagonal strings: sum_x (-1)^{x_b} |psi_x|^2 / 2 per bit, for the check of the means
  std::vector<dse::StringEntry> one(KS, dse::StringEntry{0, 0, 0, 0, 0.5, 0.0});
  for (int b = 0; b < n; ++b) one[b].zm = uint64_t(1) << b;
  CK(hipMemcpy(d_str, one.data(), one.size() * sizeof(dse::StringEntry), hipMemcpyHostToDevice));
  std::vector<float> tmp;
  time_strings(n, tmp);
  std::vector<double> hs((size_t)tiles * SS);
  CK(hipMemcpy(hs.data(), d_ps, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> iz(n, 0.0);
  double n2 = 0.0;
  for (int t = 0; t < tiles; ++t) {
    for (int b = 0; b < n; ++b) iz[b] += hs[(size_t)t * SS + 2 * b];
    n2 += hs[(size_t)t * SS + SS - 2];
  }

  // the yardstick: K diagonal two-bit strings
  std::vector<dse::StringEntry> tab(KS, dse::StringEntry{0, 0, 0, 0, 0.25, 0.0});
  for (int k = 0; k < KS; ++k)
    tab[k].zm = (uint64_t(1) << (k % n)) | (uint64_t(1) << ((k % n + 1 + (k / n) % (n - 1)) % n));
  CK(hipMemcpy(d_str, tab.data(), tab.size() * sizeof(dse::StringEntry), hipMemcpyHostToDevice));
  double per_string[3] = {0, 0, 0};
  int ki = 0;
  for (int K : {1, 4, KMAX}) {
    std::vector<float> tk;
    time_strings(K, tk);
    per_string[ki++] = tk.front() / K;
    std::printf("{\"n\": %d, \"kernel\": \"k_obs_strings<13>\", \"class\": \"diagonal\", \"K\": %d, \"reps\": %d, "
                "\"ms_best\": %.4f, \"ms_median\": %.4f, \"ms_per_string_best\": %.5f, \"TBps_best\": %.3f}\n",
                n, K, reps, tk.front(), tk[tk.size() / 2], tk.front() / K, (double)bytes / 1e12 / (tk.front() * 1e-3));
  }

  int bad = 0;
  const char* names[3] = {"thread bits", "above the tile", "all bits"};
  const uint64_t allb = (uint64_t(1) << n) - 1, hi = allb & ~((uint64_t(1) << L) - 1);
  for (int cls = 0; cls < 3; ++cls) {
    std::vector<dse::SectorEntry> sec(KMAX);
    int off = 0;
    for (int k = 0; k < KMAX; ++k) {
      uint64_t m = allb;
      if (cls == 0) m = ((uint64_t(1) << (3 + k % 7)) - 1) << (k % 3);  // within bits 0 .. 8
      if (cls == 1) m = k == 0 ? hi : hi & ~(uint64_t(1) << (L + k % (n - L)));
      const int bins = __builtin_popcountll(m) + 1;
      sec[k] = dse::SectorEntry{m, 0, 0, off, bins};
      off += bins;
    }
    CK(hipMemcpy(d_sec, sec.data(), sec.size() * sizeof(dse::SectorEntry), hipMemcpyHostToDevice));
    ki = 0;
    for (int K : {1, 4, KMAX}) {
      P.sec_k = K;
      CK(hipMemcpy(d_prob, &P, sizeof(P), hipMemcpyHostToDevice));
      const int U = sec[K - 1].off + sec[K - 1].bins, S = dse::sector_stride(U);
      std::vector<float> tk;
      for (int r = 0; r <= reps; ++r) {
        float ms = 0.f;
        CK(hipEventRecord(e0, st));
        CK(dse::launch_obs_sectors(L, d_prob, d_items, tiles, 0, d_pu, S, st));
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r) tk.push_back(ms);
      }
      std::sort(tk.begin(), tk.end());
      std::vector<double> hp((size_t)tiles * S), v(S, 0.0);
      CK(hipMemcpy(hp.data(), d_pu, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (int t = 0; t < tiles; ++t)
        for (int i = 0; i < S; ++i) v[i] += hp[(size_t)t * S + i];
      double err = std::fabs(v[S - 2] - n2) / n2;
      for (int k = 0; k < K; ++k) {
        double sum = 0.0;
        for (int j = 0; j < sec[k].bins; ++j) sum += v[sec[k].off + j];
        err = std::max(err, std::fabs(sum - n2) / n2);
      }
      double mean = 0.0, want = 0.0;
      for (int j = 0; j < sec[0].bins; ++j) mean += j * v[j];
      for (int b = 0; b < n; ++b)
        if (sec[0].m >> b & 1) want += 0.5 * n2 - iz[b];
      err = std::max(err, std::fabs(mean - want) / (n * n2));
      bad += !(err < 1e-12);
      const double per_set = tk.front() / K;
      std::printf("{\"n\": %d, \"kernel\": \"k_obs_sectors<13>\", \"class\": \"%s\", \"K\": %d, \"units\": %d, \"reps\": %d, "
                  "\"ms_best\": %.4f, \"ms_median\": %.4f, \"ms_per_set_best\": %.5f, \"per_set_over_per_string\": %.3f, "
                  "\"bins_of_set0\": %d, \"check_rel_err\": %.3e}\n",
                  n, names[cls], K, U, reps, tk.front(), tk[tk.size() / 2], per_set, per_set / per_string[ki],
                  sec[0].bins, err);
      ++ki;
    }
  }
  return bad ? 3 : 0;
}
