// dse_host.cpp -- device-independent pieces of libdse: spectral bounds and Chebyshev
// (Bessel) coefficients.  Pure C++, callable without a GPU (tests use them on CPU).
//
// The reference integrates i d/dt psi = H psi with QuTiP's sesolve (ZVODE-Adams,
// dipolar_ensemble_with_rare.py:653-666).  H is time independent (the rf drive is static in
// the rotating frame, :469-471, :514-530), so the engine propagates each output interval
// exactly:  exp(-i H dt) = exp(-i beta dt) sum_k (2 - delta_k0) (-i)^k J_k(alpha dt) T_k(Ht),
// Ht = (H - beta)/alpha with spectrum(H) inside [beta - alpha, beta + alpha].
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/dse.h"

extern "C" int dse_abi_version(void) { return DSE_ABI_VERSION; }
extern "C" int dse_abi_minor(void) { return DSE_ABI_MINOR; }

extern "C" int dse_spectral_bounds(int n, const double* field, const double* zz, const double* pair,
                                   const double* flip, double shift, double* e_min, double* e_max) {
  if (n < 1 || n > DSE_MAX_QUBITS || !field || !zz || !pair || !flip || !e_min || !e_max)
    return DSE_ERR_ARG;
  // Weyl: lambda_min(sum A_k) >= sum lambda_min(A_k), same for max.
  double lo = shift, hi = shift;
  for (int k = 0; k < n; ++k) {
    const double c = std::hypot(flip[4 * k + 2], flip[4 * k + 3]);
    const double r = std::sqrt(0.25 * field[k] * field[k] + c * c);  // field*s_k + drive: +-r
    lo -= r;
    hi += r;
  }
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      // zz s_i s_j + pair flip on {00,11}: zz/4 +- |g|; on {01,10}: -zz/4
      const double q = 0.25 * zz[i * n + j], g = std::fabs(pair[i * n + j]);
      lo += std::fmin(q - g, -q);
      hi += std::fmax(q + g, -q);
    }
  *e_min = lo;
  *e_max = hi;
  return DSE_OK;
}

// J_k(z) for k = 0..kmax by Miller's backward recurrence J_{k-1} = (2k/z) J_k - J_{k+1},
// started far above max(kmax, z) and normalised with J_0 + 2 sum_{k>=1} J_{2k} = 1.
extern "C" int dse_bessel_j(double z, int kmax, double* out, double tol, int* degree) {
  if (kmax < 1 || !out || !(z >= 0.0) || !std::isfinite(z)) return DSE_ERR_ARG;
  if (z == 0.0) {
    out[0] = 1.0;
    for (int k = 1; k <= kmax; ++k) out[k] = 0.0;
    if (degree) *degree = 1;
    return DSE_OK;
  }
  if (z < 1e-40) {
    // The recurrence below multiplies values of up to 1e250 by 2k/z and overflows (inf - inf: NaN
    // in every coefficient) for z below ~1e-58 k.  A register whose spectral half-width is zero
    // (H a multiple of 1: alpha clamped to 1e-300) has such a z.  Here the ascending series'
    // first term J_k = (z/2)^k / k! is exact in fp64 (the next is smaller by z^2 / 4(k + 1)).
    out[0] = 1.0;
    for (int k = 1; k <= kmax; ++k) out[k] = out[k - 1] * (0.5 * z / k);  // underflows to 0
    if (degree) {
      int d = 1;
      while (d < kmax && out[d + 1] > tol) ++d;  // decreasing in k
      *degree = d;
    }
    return DSE_OK;
  }
  // start index: beyond both kmax and the turning point z, plus a margin for decay below 1e-300
  const int m0 = (int)std::ceil(std::fmax((double)kmax, z) + 60.0 + 12.0 * std::cbrt(z + 1.0));
  const int m = m0 + (m0 & 1);  // even
  std::vector<double> j(m + 2, 0.0);
  j[m] = 1e-300;
  for (int k = m; k >= 1; --k) {
    j[k - 1] = (2.0 * k / z) * j[k] - j[k + 1];
    if (std::fabs(j[k - 1]) > 1e250)  // rescale everything computed so far
      for (int q = k - 1; q <= m + 1; ++q) j[q] *= 1e-250;
  }
  double norm = j[0];
  for (int k = 2; k <= m; k += 2) norm += 2.0 * j[k];
  const double inv = 1.0 / norm;
  for (int k = 0; k <= kmax; ++k) out[k] = j[k] * inv;
  if (degree) {
    int d = 1;
    for (int k = (int)std::fmin((double)m, (double)kmax); k >= 1; --k)
      if (std::fabs(j[k] * inv) > tol) { d = k; break; }
    // the tail beyond d sums below ~tol because |J_k| decays super-exponentially past z
    *degree = d < 1 ? 1 : d;
  }
  return DSE_OK;
}

// cheb_series and cheb_rows (declared in dse_internal.h, not exported): a_k = e^{-i beta tau}
// (2 - delta_k0) (-i)^k J_k(alpha tau), of one offset tau and of every offset of every set
namespace dse {
__attribute__((visibility("hidden")))
int cheb_series(double alpha, double beta, double tau, double tol, double max_degree, int* deg,
                std::vector<std::pair<double, double>>* a, int* kmax_over, std::vector<double>* J) {
  const double z = alpha * tau;
  const int kmax = (int)std::ceil(z + 12.0 * std::cbrt(z + 1.0) + 60.0);
  if (kmax > max_degree) {
    *kmax_over = kmax;
    return DSE_ERR_CONVERGENCE;
  }
  std::vector<double> Jv(kmax + 1);
  int d = 1;
  if (dse_bessel_j(z, kmax, Jv.data(), tol, &d) != DSE_OK) return DSE_ERR_ARG;
  *deg = d;
  const double ph = -beta * tau;
  const std::complex<double> e(std::cos(ph), std::sin(ph));
  std::complex<double> mi(1.0, 0.0);  // (-i)^k
  a->assign((size_t)d + 1, std::make_pair(0.0, 0.0));
  for (int k = 0; k <= d; ++k) {
    const std::complex<double> ak = e * mi * ((k == 0 ? 1.0 : 2.0) * Jv[k]);
    (*a)[k] = std::make_pair(ak.real(), ak.imag());
    mi *= std::complex<double>(0.0, -1.0);
  }
  const double* j0 = Jv.data();
  if (J) J->assign(j0, j0 + d + 1);
  return DSE_OK;
}

__attribute__((visibility("hidden")))
int cheb_rows(double alpha, double beta, const std::vector<std::vector<double>>& set_tau, int M, double tol,
              double max_degree, int* deg_out, std::vector<std::pair<double, double>>* rows, int* kmax_over) {
  const int n_sets = (int)set_tau.size();
  int deg = 1;
  std::vector<std::vector<std::pair<double, double>>> a((size_t)n_sets * M);
  for (int s = 0; s < n_sets; ++s)
    for (size_t j = 0; j < set_tau[s].size(); ++j) {
      int d = 1;
      if (int rc = cheb_series(alpha, beta, set_tau[s][j], tol, max_degree, &d, &a[(size_t)s * M + j], kmax_over, nullptr))
        return rc;
      deg = std::max(deg, d);
    }
  *deg_out = deg;
  const int kcap1 = deg + 1;
  rows->assign((size_t)n_sets * M * (kcap1 + 1), std::make_pair(0.0, 0.0));
  for (int s = 0; s < n_sets; ++s)
    for (size_t j = 0; j < set_tau[s].size(); ++j) {
      const std::vector<std::pair<double, double>>& aj = a[(size_t)s * M + j];
      std::pair<double, double>* row = rows->data() + ((size_t)s * M + j) * (kcap1 + 1);
      row[0] = std::make_pair((double)(aj.size() - 1), 0.0);
      std::copy(aj.begin(), aj.end(), row + 1);
    }
  return DSE_OK;
}
}  // namespace dse
