// dse_small.hip -- persistent engine for small registers (n <= 9 qubits: the reference's default
// sweep, n_sea = 6 -> N = 7, sweep_sea_detuning.py:1240).
//
// A register of n <= 9 qubits is at most 512 amplitudes (8 KiB): one wave holds it.  Workgroup =
// one wave = one problem; lane l owns the amplitudes x = r * 64 + l, r < R = 2^(n-6) (n >= 6; a
// smaller register uses its first 2^n lanes).  One launch runs a chunk of output intervals of
// every small problem of the context completely on chip:
//   LDS        w_{k-1} of the register (the operand of H)
//   registers  o (w_k being formed: starts as -w_{k-2} / (2 s1), see k_interval), the propagator
//              sum acc of the interval (ONE output per series: the coarse-grid regime these
//              registers live in, alpha dt ~ 1e3..1e4 on the reference's 30 s grid), D(x) - beta
// At each output time acc = psi(t_m) goes to LDS, the 7 observable sums are reduced over the wave
// and written to out[problem][m][8], and acc becomes w_0 of the next interval.  Between launches
// the state lives in the problem's buffer.  Every term is compile-time structure (the masks of
// all n drives and n (n - 1) / 2 pairs are known for a given n; coefficients come from LDS), so
// a term costs n + n(n-1)/2 LDS partner reads per amplitude and no other memory traffic.
// Launches: ceil((n_t - 1) / chunk), independent of the Chebyshev degree (the per-term streaming
// kernels would need one launch per term: ~1e8 for a 30 s N = 7 evolution).
#include "dse_device.h"
#include "dse_small.h"

namespace dse {
namespace {

template <int N>
struct SmallGeo {
  static constexpr int DIM = 1 << N;
  static constexpr int R = N >= 6 ? (1 << (N - 6)) : 1;
  static constexpr int NP = N * (N - 1) / 2;
};

// Site-resolved sums of the state in LDS w (option site_obs): X_b Y_b Z_b at o[3 b + c] for every
// bit b < N, ||psi||^2 at o[3 N], zero up to kSmallSiteStride; each sum one wave butterfly.
template <int N>
__device__ __forceinline__ void small_site_sums(const double2* w, int lane, bool live, double* o) {
  constexpr int R = SmallGeo<N>::R;
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double2 p = live ? w[r * 64 + lane] : make_double2(0.0, 0.0);
    n2 += p.x * p.x + p.y * p.y;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off, 64);
  if (lane == 0) o[3 * N] = n2;
  if (lane > 0 && 3 * N + lane < kSmallSiteStride) o[3 * N + lane] = 0.0;
  for (int b = 0; b < N; ++b) {
    double v[3] = {0, 0, 0};
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int x = r * 64 + lane;
      if (!live) continue;
      const double2 p = w[x];
      const double p2 = p.x * p.x + p.y * p.y;
      if ((x >> b) & 1) {
        v[2] -= 0.5 * p2;
        continue;
      }
      v[2] += 0.5 * p2;
      const double2 s = w[x ^ (1 << b)];
      v[0] += p.x * s.x + p.y * s.y;
      v[1] += p.x * s.y - p.y * s.x;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    if (lane == 0) {
      o[3 * b] = v[0];
      o[3 * b + 1] = v[1];
      o[3 * b + 2] = v[2];
    }
  }
}

// Two-spin sums of the state in LDS w (option pair_obs; the record of dse_pairs.hip): for every pair
// i < j the amplitudes with bit_i = 0 read their partner x ^ e_i ^ e_j, bit_j sends the product to ZQ
// or DQ; each sum one wave butterfly, pairs in index order.
template <int N>
__device__ __forceinline__ void small_pair_sums(const double2* w, int lane, bool live, double* o) {
  constexpr int R = SmallGeo<N>::R, NP = SmallGeo<N>::NP;
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double2 p = live ? w[r * 64 + lane] : make_double2(0.0, 0.0);
    n2 += p.x * p.x + p.y * p.y;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off, 64);
  if (lane == 0) o[5 * NP] = n2;
  for (int i = 5 * NP + 1 + lane; i < kSmallPairStride; i += 64) o[i] = 0.0;
  int e = 0;
  for (int j = 1; j < N; ++j)
    for (int i = 0; i < j; ++i, ++e) {
      double v[5] = {0, 0, 0, 0, 0};
      const int m = (1 << i) | (1 << j);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int x = r * 64 + lane;
        if (!live) continue;
        const double2 p = w[x];
        const double p2 = p.x * p.x + p.y * p.y;
        const bool i1 = (x >> i) & 1, j1 = (x >> j) & 1;
        v[0] += (i1 != j1 ? -0.25 : 0.25) * p2;
        if (i1) continue;
        const double2 s = w[x ^ m];
        const double re = p.x * s.x + p.y * s.y, im = p.x * s.y - p.y * s.x;
        if (j1)
          v[1] += re, v[2] += im;
        else
          v[3] += re, v[4] += im;
      }
#pragma unroll
      for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
      if (lane < 5) o[5 * e + lane] = lane == 0 ? v[0] : lane == 1 ? v[1] : lane == 2 ? v[2] : lane == 3 ? v[3] : v[4];
    }
}

// Overlaps of the state in LDS w with the problem's K reference states (the record of
// dse_overlap.hip at the stride kSmallOverlapStride): the wave reads each reference from memory (2^N
// x 16 B <= 8 KiB, 16-byte loads) and dots it with the state, one wave butterfly per sum, references
// in order.  K = 0: nothing is written.
template <int N>
__device__ __forceinline__ void small_overlap_sums(const double2* w, int lane, bool live,
                                                   const double2* const* refs, int K, double* o) {
  constexpr int R = SmallGeo<N>::R;
  if (K <= 0) return;
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double2 p = live ? w[r * 64 + lane] : make_double2(0.0, 0.0);
    n2 += p.x * p.x + p.y * p.y;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off, 64);
  if (2 * K + lane < kSmallOverlapStride) o[2 * K + lane] = (2 * K + lane == kSmallOverlapStride - 2) ? n2 : 0.0;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const gd2* gref = gptr(refs[k]);
    double re = 0.0, im = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!live) continue;
      const double2 f = gld(gref, r * 64 + lane);
      const double2 p = w[r * 64 + lane];
      re += f.x * p.x + f.y * p.y;  // conj(phi) psi
      im += f.x * p.y - f.y * p.x;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      re += __shfl_xor(re, off, 64);
      im += __shfl_xor(im, off, 64);
    }
    if (lane < 2) o[2 * k + lane] = lane == 0 ? re : im;
  }
}

// Operator strings of the state in LDS w (the record of dse_strings.hip at the stride
// kSmallStringStride): strings in table order, the partner from LDS at x ^ xm, one wave butterfly per
// sum, the prefactor applied when storing.  K = 0: nothing is written.
template <int N>
__device__ __forceinline__ void small_string_sums(const double2* w, int lane, bool live,
                                                  const StringEntry* __restrict__ tab, int K, double* o) {
  constexpr int R = SmallGeo<N>::R;
  if (K <= 0) return;
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double2 p = live ? w[r * 64 + lane] : make_double2(0.0, 0.0);
    n2 += p.x * p.x + p.y * p.y;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off, 64);
  for (int i = 2 * K + lane; i < kSmallStringStride; i += 64) o[i] = (i == kSmallStringStride - 2) ? n2 : 0.0;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const uint32_t xm = (uint32_t)tab[k].xm, zm = (uint32_t)tab[k].zm, cm = (uint32_t)tab[k].cm, cv = (uint32_t)tab[k].cv;
    double re = 0.0, im = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t x = (uint32_t)(r * 64 + lane);
      if (!live || (x & cm) != cv) continue;
      const double2 p = w[x], s = w[x ^ xm];
      const double zr = p.x * s.x + p.y * s.y, zi = p.x * s.y - p.y * s.x;  // conj(p) s
      const bool neg = __popc(x & zm) & 1;
      re += neg ? -zr : zr;
      im += neg ? -zi : zi;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      re += __shfl_xor(re, off, 64);
      im += __shfl_xor(im, off, 64);
    }
    const double pr = tab[k].pre_re, pi = tab[k].pre_im;
    if (lane < 2) o[2 * k + lane] = lane == 0 ? pr * re - pi * im : pr * im + pi * re;
  }
}

// Sector populations of the state in LDS w (the record of dse_sectors.hip at the stride
// kSmallSectorStride): sets in table order, the selection applied per amplitude, then
// sector_wave_bins over the row bits (register bits 6 ..) and the lane bits; lane 0 holds the set's
// bins under compile-time indices and stores them.  K = 0: nothing is written.
template <int N>
__device__ __forceinline__ void small_sector_sums(const double2* w, int lane, bool live,
                                                  const SectorEntry* __restrict__ tab, int K, double* o) {
  constexpr int R = SmallGeo<N>::R, LR = N >= 6 ? N - 6 : 0, VL = LR + 7;
  if (K <= 0) return;
  double p2[R];
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const double2 p = live ? w[r * 64 + lane] : make_double2(0.0, 0.0);
    p2[r] = p.x * p.x + p.y * p.y;
    n2 += p2[r];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off, 64);
  const int U = tab[K - 1].off + tab[K - 1].bins;
  for (int i = U + lane; i < kSmallSectorStride; i += 64) o[i] = (i == kSmallSectorStride - 2) ? n2 : 0.0;
#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const uint32_t m = (uint32_t)tab[k].m, cm = (uint32_t)tab[k].cm, cv = (uint32_t)tab[k].cv;
    double q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) q[r] = (((uint32_t)(r * 64 + lane)) & cm) == cv ? p2[r] : 0.0;
    double v[VL];
    sector_wave_bins<LR>(q, m >> 6, m & 63u, v);
    if (lane == 0) {
      const int bins = tab[k].bins;
      double* ok = o + tab[k].off;
#pragma unroll
      for (int c = 0; c < VL; ++c)
        if (c < bins) ok[c] = v[c];
    }
  }
}

#define DSE_SMALL_OVL 0
#include "dse_small_kernels.inc"
#undef DSE_SMALL_OVL
#define DSE_SMALL_OVL 1
#include "dse_small_kernels.inc"
#undef DSE_SMALL_OVL
#define DSE_SMALL_OVL 2
#include "dse_small_kernels.inc"
#undef DSE_SMALL_OVL
#define DSE_SMALL_OVL 3
#include "dse_small_kernels.inc"
#undef DSE_SMALL_OVL

}  // namespace

#define DSE_SMALL_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9)

// (SITES, PAIRS) of a launch from the two output pointers; with ovl the _ovl kernel of the same two,
// with strs the _str kernel (ovl then optional at run time), with secs the _sec kernel (ovl and strs
// then optional at run time)
#define DSE_SMALL_LAUNCH(K, q, S_, P_, ...)                                                                  \
  do {                                                                                                       \
    if (secs)                                                                                                \
      hipLaunchKernelGGL((K##_sec<q, S_, P_>), dim3(count), dim3(64), 0, st, __VA_ARGS__, sites, pairs, ovl, strs, secs); \
    else if (strs)                                                                                                \
      hipLaunchKernelGGL((K##_str<q, S_, P_>), dim3(count), dim3(64), 0, st, __VA_ARGS__, sites, pairs, ovl, strs); \
    else if (ovl)                                                                                               \
      hipLaunchKernelGGL((K##_ovl<q, S_, P_>), dim3(count), dim3(64), 0, st, __VA_ARGS__, sites, pairs, ovl); \
    else                                                                                                     \
      hipLaunchKernelGGL((K<q, S_, P_>), dim3(count), dim3(64), 0, st, __VA_ARGS__, sites, pairs);           \
  } while (0)
#define DSE_SMALL_VARIANT(K, q, ...)                     \
  do {                                                   \
    if (sites && pairs)                                  \
      DSE_SMALL_LAUNCH(K, q, true, true, __VA_ARGS__);   \
    else if (pairs)                                      \
      DSE_SMALL_LAUNCH(K, q, false, true, __VA_ARGS__);  \
    else if (sites)                                      \
      DSE_SMALL_LAUNCH(K, q, true, false, __VA_ARGS__);  \
    else                                                 \
      DSE_SMALL_LAUNCH(K, q, false, false, __VA_ARGS__); \
  } while (0)

hipError_t launch_small(int n, const SmallProb* probs, const int* sel, int count, int m0, int n_int,
                        const int* iv_set, double* out, hipStream_t st, double* sites, double* pairs,
                        double* ovl, double* strs, double* secs) {
  if (count <= 0) return hipSuccess;
  switch (n) {
#define X(q) \
  case q: DSE_SMALL_VARIANT(k_small, q, probs, sel, m0, n_int, iv_set, out); break;
    DSE_SMALL_CASES(X)
#undef X
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_small_obs0(int n, const SmallProb* probs, const int* sel, int count, double* out,
                             hipStream_t st, double* sites, double* pairs, double* ovl, double* strs,
                             double* secs) {
  if (count <= 0) return hipSuccess;
  switch (n) {
#define X(q) \
  case q: DSE_SMALL_VARIANT(k_small_obs0, q, probs, sel, out); break;
    DSE_SMALL_CASES(X)
#undef X
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace dse
