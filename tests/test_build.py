"""Build-level checks of the HIP sources (CPU only: hipcc cross-compiles for gfx950)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantumsimulations_amd", "csrc")


def _hipcc():
    for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    pytest.skip("hipcc not available")


def _resources(stderr):
    """(function name, VGPR spill count, scratch bytes per lane) per kernel of a
    -Rpass-analysis=kernel-resource-usage compile."""
    rows = {}
    name = None
    for line in stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            rows[name] = [None, None]
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            rows[name][0] = int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            rows[name][1] = int(m.group(1))
    return [(n, sp, sc) for n, (sp, sc) in rows.items()]


def test_interval_kernel_does_not_spill(tmp_path):
    """k_interval holds w_{k-2} and w_k (16 amplitudes each) in registers at 2 waves per SIMD:
    every variant must fit the 256-VGPR budget without scratch spills (a spilling build gave
    run-to-run differences of ~1e-9 on 2-tile problems)."""
    res = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
         "--cuda-device-only", "-c", os.path.join(CSRC, "dse_interval.hip"), "-o",
         str(tmp_path / "iv.o"), "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = [k for k in _resources(res.stderr) if "k_interval" in k[0]]
    assert len(kernels) == 8, kernels
    assert all(sp == 0 and sc == 0 for _, sp, sc in kernels), kernels


def test_wht_passes_do_not_spill(tmp_path):
    """The Walsh-Hadamard passes (2 tile sizes x 5 passes x 3 modes, FWD / MID / INV also per
    vector of a partitioned register; the half-LDS forms of option wht_half within 128 VGPRs) stay spill-free and keep their tile arrays out of scratch
    (a run-time vector selector once put them there: N = 30 went from 68 to 353 ms per H); the
    one-thread-per-tile table kernels run once per problem and may use scratch."""
    res = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
         "--cuda-device-only", "-c", os.path.join(CSRC, "dse_wht.hip"), "-o",
         str(tmp_path / "wht.o"), "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = [k for k in _resources(res.stderr) if "k_wht" in k[0]]
    persistent = [k for k in kernels if "k_wht_mid_p" in k[0]]
    half = [k for k in kernels if "k_wht_h" in k[0]]
    passes = [k for k in kernels if "k_wht_tables" not in k[0] and "k_wht_qtab" not in k[0] and k not in persistent
              and k not in half]
    assert len(passes) == 2 * (3 * 3 + 3 * 3 * 3), [k[0] for k in passes]  # FIRST, FINAL, FINAL_NEXT x mode
    assert len(persistent) == 2 * 3 * 3, [k[0] for k in persistent]  # tile x mode x vectors
    assert len(half) == 3 + 3 * 3 * 3, [k[0] for k in half]  # 13-bit tiles: FIRST x mode, FWD/MID/INV x mode x vectors
    passes += persistent + half
    assert all(sp == 0 for _, sp, _ in kernels), kernels
    assert all(sc == 0 for _, _, sc in passes), passes


def test_span_kernel_does_not_spill(tmp_path):
    """k_span (dse_span.hip) keeps out, w_{k-2} and the pipelined partner rows in registers at two
    waves per SIMD for the 512-thread configurations (2^11 tiles x 4 rows, 2^10 x 2 rows)."""
    res = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c",
         os.path.join(CSRC, "dse_span.hip"), "-o", str(tmp_path / "span.o"), "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = [k for k in _resources(res.stderr) if "k_span" in k[0]]
    assert len(kernels) >= 4, kernels
    assert all(sp == 0 and sc == 0 for _, sp, sc in kernels), kernels


def test_real_kernel_does_not_spill(tmp_path):
    """k_real (dse_real.hip, option real): the production instantiation k_real<0> holds out and
    w_{k-2} (32 real rows each) in registers at two waves per SIMD without scratch spills (the
    diagnostic ablation instantiations may spill)."""
    res = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-c",
         os.path.join(CSRC, "dse_real.hip"), "-o", str(tmp_path / "real.o"), "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = [k for k in _resources(res.stderr) if "k_realILi0E" in k[0]]
    assert len(kernels) == 1, _resources(res.stderr)
    assert all(sp == 0 and sc == 0 for _, sp, sc in kernels), kernels


def test_coef_schedule_covers_every_term_once(tmp_path):
    """coef_nterm (dse_internal.h): for every update phase (k_span staggers output j to phase
    j % 3) and series degree d, the terms accumulated at k = 1..d are exactly a_0..a_d, each once,
    and no update reaches further back than w_{k-2}; phase 0 is the k_interval / k_real schedule
    (updates at k = 1, 4, 7, ... and the remainder at k = d)."""
    src = tmp_path / "sched.cpp"
    src.write_text(r'''
#include "dse_internal.h"
#include <cstdio>
int main() {
  for (int ph = 0; ph < 3; ++ph)
    for (int d = 1; d <= 400; ++d) {
      int next = 0;  // first term not yet accumulated
      for (int k = 1; k <= d + 1; ++k) {
        const int n = dse::coef_nterm(k, d, ph);
        if (k > d) { if (n) return 1; continue; }
        if (n > 3 || (k == 1 && n != 2)) return 2;
        if (n == 0) continue;
        if (k - n + 1 != (k == 1 ? 0 : next) && !(k == 1 && next == 0)) return 3;
        next = k + 1;
      }
      if (next != d + 1) return 4;
      if (ph == 0)
        for (int k = 2; k <= d; ++k)
          if ((dse::coef_nterm(k, d, 0) == 3) != ((k - 1) % 3 == 0)) return 5;
    }
  std::puts("ok");
  return 0;
}
''')
    exe = tmp_path / "sched"
    res = subprocess.run([_hipcc(), "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                          "-x", "hip", "--offload-arch=gfx950", str(src), "-o", str(exe)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr)


CHEB_ROWS_SRC = r'''
#include "dse_internal.h"
#include "dse.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
int main() {
  const double alphas[3] = {std::max(0.0, 1e-300), 3e4, 2e6};  // 0 as coef_one clamps it
  const double beta = 1.5e5, tol = 1e-14;
  const int M = 4;
  const std::vector<std::vector<double>> sets = {{1e-5}, {1e-5, 2e-5}, {2.5e-4, 5e-4, 7.5e-4, 1e-3}};
  const long double pi = 3.141592653589793238462643383279502884L;
  double worst = 0.0;
  for (double alpha : alphas) {
    int deg = 0, over = 0;
    std::vector<std::pair<double, double>> rows;
    if (dse::cheb_rows(alpha, beta, sets, M, tol, 2e6, &deg, &rows, &over) != DSE_OK) return 1;
    const size_t w = (size_t)deg + 2;  // kcap1 + 1
    if (rows.size() != sets.size() * M * w) return 2;
    int dmax = 1;
    for (size_t s = 0; s < sets.size(); ++s)
      for (int j = 0; j < M; ++j) {
        const std::pair<double, double>* row = rows.data() + (s * M + j) * w;
        if (j >= (int)sets[s].size()) {  // a set shorter than M: zero-filled rows
          for (size_t e = 0; e < w; ++e)
            if (row[e].first != 0.0 || row[e].second != 0.0) return 3;
          continue;
        }
        const double tau = sets[s][j], z = alpha * tau;
        const int kmax = (int)std::ceil(z + 12.0 * std::cbrt(z + 1.0) + 60.0);
        std::vector<double> J(kmax + 1);
        int d = 0;
        if (dse_bessel_j(z, kmax, J.data(), tol, &d) != DSE_OK) return 4;
        if (row[0].first != (double)d || row[0].second != 0.0) return 5;  // (a)
        dmax = std::max(dmax, d);
        {  // (e) cheb_series of this tau: bit for bit the one row of cheb_rows with M = 1, and J dse_bessel_j's
          int d1 = 0, ds = 0, over1 = 0;
          std::vector<std::pair<double, double>> one, a;
          std::vector<double> Js;
          const std::vector<std::vector<double>> lone(1, std::vector<double>(1, tau));
          if (dse::cheb_rows(alpha, beta, lone, 1, tol, 2e6, &d1, &one, &over1) != DSE_OK) return 9;
          if (dse::cheb_series(alpha, beta, tau, tol, 2e6, &ds, &a, &over1, &Js) != DSE_OK) return 10;
          if (ds != d || d1 != std::max(d, 1) || a.size() != (size_t)d + 1 || Js.size() != a.size()) return 11;
          if (one.size() != (size_t)d1 + 2 || one[0].first != (double)d || one[0].second != 0.0) return 12;
          for (int k = 0; k <= d; ++k)
            if (!(a[k].first == one[1 + k].first && a[k].second == one[1 + k].second && Js[k] == J[k] &&
                  a[k].first == row[1 + k].first && a[k].second == row[1 + k].second))
              return 13;
        }
        for (size_t k = (size_t)d + 1; k + 1 < w; ++k)  // (c)
          if (row[1 + k].first != 0.0 || row[1 + k].second != 0.0) return 6;
        for (int i = 0; i < 33; ++i) {  // (d)
          const long double x = std::cos(pi * (i + 0.5L) / 33.0L);
          long double t0 = 1.0L, t1 = x, re = row[1].first, im = row[1].second;
          for (int k = 1; k <= d; ++k) {
            re += row[1 + k].first * t1;
            im += row[1 + k].second * t1;
            const long double t2 = 2.0L * x * t1 - t0;
            t0 = t1;
            t1 = t2;
          }
          const long double ph = -((long double)alpha * x + (long double)beta) * (long double)tau;
          const double err = (double)std::hypot(re - std::cos(ph), im - std::sin(ph));
          worst = std::max(worst, err);
          if (!(err <= 1e-12)) {
            std::printf("alpha %g tau %g x %g: error %.3e\n", alpha, tau, (double)x, err);
            return 7;
          }
        }
      }
    if (deg != dmax) return 8;  // (b)
  }
  std::printf("ok %.3e\n", worst);
  return 0;
}
'''


def test_cheb_rows_match_bessel_and_the_propagator(tmp_path):
    """cheb_rows (dse_host.cpp: the coefficient rows every Chebyshev engine of dse_evolve uploads) for a
    zero, a moderate and a stiff spectral half-width (z = alpha tau up to 2000), M = 4 with sets shorter
    than M: every row's degree is dse_bessel_j's, deg their maximum, the entries past a row's degree
    and the rows past a set's length are zero, and at 33 Chebyshev nodes sum_k a_k T_k(x) is
    exp(-i (alpha x + beta) tau) to 1e-12.  The bound: the dropped tail is below ~tol = 1e-14, and at
    most ~2,100 terms of magnitude <= 2, each coefficient rounded in fp64, sum to an error of at most
    2,100 * 2 * 2.2e-16 ~ 1e-12.  T_k by the three-term recurrence, carried with the reference phase
    in long double, so the figure is the rows' error and not the recurrence's.  cheb_series, the
    series of one offset that cheb_rows, the small-register engine (small_launch) and the propagator-
    matrix mode (matrix_run) are all built on, equals for every alpha and tau the row of cheb_rows with
    M = 1 bit for bit (== on the doubles), and its J_k are dse_bessel_j's: the 1e-12 bound covers all
    three users."""
    src = tmp_path / "rows.cpp"
    src.write_text(CHEB_ROWS_SRC)
    exe = tmp_path / "rows"
    res = subprocess.run([_hipcc(), "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                          "-x", "hip", "--offload-arch=gfx950", str(src), os.path.join(CSRC, "dse_host.cpp"),
                          "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.returncode, run.stdout, run.stderr)
