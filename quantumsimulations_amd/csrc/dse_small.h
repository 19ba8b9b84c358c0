// dse_small.h -- the small-register engine (dse_small.hip): registers of n <= 9 qubits, one wave
// per problem, all Chebyshev terms and the observables of a chunk of output intervals per launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dse_internal.h"  // StringEntry

namespace dse {

constexpr int kSmallMaxQubits = 9;
// site-resolved sums per problem and output (option site_obs): X_b Y_b Z_b at [3 b + c], ||psi||^2
// at [3 n], padded to an even count for n = 9
constexpr int kSmallSiteStride = 28;
// two-spin sums per problem and output (option pair_obs): ZZ, Re ZQ, Im ZQ, Re DQ, Im DQ of pair p at
// [5 p + c], ||psi||^2 at [5 NP], padded to an even count for n = 9 (pair_stride(9))
constexpr int kSmallPairStride = 182;
// overlaps with reference states per problem and output: Re, Im of <phi_k|psi> at [2 k], [2 k + 1],
// ||psi||^2 at [32] (overlap_stride(16): every register's record is sized for the cap)
constexpr int kSmallOverlapStride = 2 * 16 + 2;
// operator strings per problem and output: Re, Im of string k at [2 k], [2 k + 1], ||psi||^2 at [128]
// (string_stride(64): every register's record is sized for the cap)
constexpr int kSmallStringStride = 2 * 64 + 2;
// sector populations per problem and output: set k's bins from [off_k], ||psi||^2 at [160]
// (sector_stride(16 x 10): 16 sets of at most 9 counted bits; every register's record is sized for that)
constexpr int kSmallSectorStride = 16 * 10 + 2;

struct SmallProb {
  double2* state;          // [2^n] the state at the start of the next launch
  const double* field;     // [n]
  const double* zz;        // [n*n]
  const double* pair;      // [n*n]
  const double* flip;      // [4n] re0 im0 re1 im1 (output bit value 0 / 1)
  const double2* coef;     // [n_sets][kcap1] a_k = e^{-i beta tau} (2 - d_k0) (-i)^k J_k(alpha tau)
  const int* deg;          // [n_sets] Chebyshev degree K of each interval length
  uint64_t sea_mask;
  double shift, beta, s1;
  int n, rare_bit, kcap1, n_t;
  // the register's ovl_k reference states, 2^n amplitudes each (null, 0: none)
  const double2* const* ovl_refs;
  int ovl_k;
  // the register's compiled operator strings (null, 0: none)
  const StringEntry* str_tab;
  int str_k;
  // the register's sector sets (null, 0: none)
  const SectorEntry* sec_tab;
  int sec_k;
};

// One launch: intervals m0 .. m0 + n_int - 1 of problems sel[0 .. count) (all with n qubits);
// out[problem][m + 1][8] = raw observable sums of psi(t_{m+1}) (dse_runtime.hip finish_obs).
hipError_t launch_small(int n, const SmallProb* probs, const int* sel, int count, int m0, int n_int,
                        const int* iv_set, double* out, hipStream_t st, double* sites = nullptr,
                        double* pairs = nullptr, double* ovl = nullptr, double* strs = nullptr,
                        double* secs = nullptr);
// out[problem][0][8] = observable sums of the state buffer (psi0)
// sites non-null (both launches): also sites[problem][m][kSmallSiteStride], the site-resolved sums
// pairs non-null (both launches): also pairs[problem][m][kSmallPairStride], the two-spin sums
// ovl non-null (both launches): also ovl[problem][m][kSmallOverlapStride], the overlaps with the
// problem's reference states (a problem without references: its records are left unwritten)
// strs non-null (both launches): also strs[problem][m][kSmallStringStride], the operator strings of
// the problem's table (a problem without strings: its records are left unwritten); the kernels are
// then k_small_str / k_small_obs0_str, which take ovl and strs as run-time-optional pointers
// secs non-null (both launches): also secs[problem][m][kSmallSectorStride], the sector populations of
// the problem's sets (a problem without sets: its records are left unwritten); the kernels are then
// k_small_sec / k_small_obs0_sec, which take ovl, strs and secs as run-time-optional pointers
hipError_t launch_small_obs0(int n, const SmallProb* probs, const int* sel, int count, double* out,
                             hipStream_t st, double* sites = nullptr, double* pairs = nullptr,
                             double* ovl = nullptr, double* strs = nullptr, double* secs = nullptr);

}  // namespace dse
