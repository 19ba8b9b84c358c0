// dse_init.hip -- kernels behind a custom initial state (dse_set_initial_state,
// dse_set_initial_product, dse_continue_from_final; include/dse.h, ABI 14.1).
//
// The propagators are linear in psi, so a general psi(t0) only changes how a register's first
// vector is filled.  Three one-shot, bandwidth-bound kernels:
//   k_product_state   psi(x) = prod_b a_b[bit_b(x)] straight into the state buffer
//   k_real_split      k_real's rotated-frame input [a | b] = [Re phi0 | Im phi0], phi0_x = i^|x| psi0_x
//   k_dense_project   the dense engine's coefficients c = V^T phi0 (complex), one column per workgroup
// Every sum runs in a fixed order (no atomics): repeated runs are bitwise equal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "dse_dense.h"
#include "dse_device.h"  // wave_sum

namespace dse {

namespace {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// i^p z
__device__ __forceinline__ double2 irot(int p, double2 z) {
  p &= 3;
  return p == 0 ? z : p == 1 ? make_double2(-z.y, z.x) : p == 2 ? make_double2(-z.x, -z.y) : make_double2(z.y, -z.x);
}
// a_b[v] of the amplitude table (re a_b0, im a_b0, re a_b1, im a_b1 per bit)
__device__ __forceinline__ double2 amp_at(const double* __restrict__ amp, int b, uint64_t v) {
  const double* p = amp + 4 * b + 2 * (int)(v & 1u);
  return make_double2(p[0], p[1]);
}

constexpr int kProdLoBits = 8;     // bits of the per-thread factor (x mod 256 = thread)
constexpr int kProdChunkBits = 16; // amplitudes per workgroup: 2^16 (1 MiB of stores)

// One workgroup writes the 2^C amplitudes x = (block << C) + r * 256 + t, C = min(n_local, 16), of
// the shard whose global indices are g = g_base | x.  Thread t keeps the factor of bits 0..7 (its
// own low bits) in registers; the LDS table holds, per row r, the factor of bits 8..C-1 times the
// workgroup's factor of the bits >= C (formed once per workgroup): one complex multiply, one LDS
// broadcast read and one 16-byte store per amplitude, at most n - 1 multiplies behind each value.
__global__ void __launch_bounds__(256)
k_product_state(double2* __restrict__ out, const double* __restrict__ amp, int n, int n_local, uint64_t g_base) {
  __shared__ double2 row_s[256];
  const int t = threadIdx.x;
  const int C = n_local < kProdChunkBits ? n_local : kProdChunkBits;
  const int nlo = n_local < kProdLoBits ? n_local : kProdLoBits;
  const uint64_t base = (uint64_t)blockIdx.x << C;
  const uint64_t g = g_base | base;
  double2 lo = amp_at(amp, 0, (uint64_t)t);
  for (int b = 1; b < nlo; ++b) lo = cmul(lo, amp_at(amp, b, (uint64_t)t >> b));
  const int rows = 1 << (C - nlo);
  if (t < rows) {
    // bits nlo..C-1 from the row index, bits >= C from the workgroup's global index
    const uint64_t gr = g | ((uint64_t)t << nlo);
    double2 f = make_double2(1.0, 0.0);
    bool first = true;
    for (int b = nlo; b < n; ++b) {
      const double2 a = amp_at(amp, b, gr >> b);
      f = first ? a : cmul(f, a);
      first = false;
    }
    row_s[t] = f;
  }
  __syncthreads();
  const uint64_t dim = uint64_t(1) << n_local;
  const bool lone = nlo == n;  // no factor beyond the thread's own
  for (int r = 0; r < rows; ++r) {
    const uint64_t x = base + ((uint64_t)r << nlo) + (uint64_t)t;
    if (t < (1 << nlo) && x < dim) out[x] = lone ? lo : cmul(row_s[r], lo);
  }
}

// [a | b] = [Re phi0 | Im phi0], phi0_x = i^|x| psi0_x, of the listed real-mode registers whose
// table says "psi0 from the state buffer" (RealTab::x0 == kRealFromBuffer); the others keep
// k_real_init's [e_x0 | 0].  grid: (2^n / 256 strided, problems of the list)
__global__ void __launch_bounds__(256)
k_real_split(const DevProb* __restrict__ probs, const int2* __restrict__ items) {
  const DevProb& P = probs[items[blockIdx.y].x];
  if (P.rtab->x0 != kRealFromBuffer) return;
  const size_t nn = size_t(1) << P.n;
  const double2* __restrict__ psi0 = P.buf[0];
  for (size_t x = (size_t)blockIdx.x * 256 + threadIdx.x; x < nn; x += (size_t)gridDim.x * 256) {
    const double2 phi = irot(__popcll((unsigned long long)x), psi0[x]);
    P.rin[x] = phi.x;
    P.rin[nn + x] = phi.y;
  }
}

// c_a = sum_x V[x + a dim] phi0_x for column a = blockIdx.x of every problem with a coefficient
// buffer (DenseProb::c; null: the basis state, whose c is a row of V).  phi0 = i^|x| psi0 in the
// rotated frame (rot), psi0 else; psi0 is read from DenseProb::init.  Each thread sums its rows
// x = t, t + 256, ... in order, the wave by butterflies, the four waves in order.
__global__ void __launch_bounds__(256)
k_dense_project(const DenseProb* __restrict__ probs, int dim) {
  __shared__ double red[4][2];
  const DenseProb& P = probs[blockIdx.y];
  if (!P.c) return;
  const uint32_t a = blockIdx.x;
  const double* __restrict__ col = P.V + (size_t)a * dim;
  const double2* __restrict__ psi0 = P.init;
  double sr = 0.0, si = 0.0;
  for (uint32_t x = threadIdx.x; x < (uint32_t)dim; x += 256u) {
    const double2 phi = P.rot ? irot(__popc(x), psi0[x]) : psi0[x];
    const double v = col[x];
    sr = fma(v, phi.x, sr);
    si = fma(v, phi.y, si);
  }
  wave_sum(sr, si);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = sr, red[threadIdx.x >> 6][1] = si;
  __syncthreads();
  if (threadIdx.x == 0) {
    P.c[a] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    P.c[(size_t)dim + a] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
  }
}

}  // namespace

hipError_t launch_product_state(double2* out, const double* amp, int n, int n_local, uint64_t shard,
                                hipStream_t st) {
  if (n < 1 || n_local < 1 || n_local > n) return hipErrorInvalidValue;
  const int C = std::min(n_local, kProdChunkBits);
  const uint64_t blocks = uint64_t(1) << (n_local - C);
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_product_state, dim3((unsigned)blocks), dim3(256), 0, st, out, amp, n, n_local,
                     shard << n_local);
  return hipGetLastError();
}

hipError_t launch_real_split(const DevProb* probs, const int2* items, int n_items, hipStream_t st) {
  if (n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_real_split, dim3(32, n_items), dim3(256), 0, st, probs, items);
  return hipGetLastError();
}

hipError_t launch_dense_project(const DenseProb* d, int count, int dim, hipStream_t st) {
  hipLaunchKernelGGL(k_dense_project, dim3(dim, count), dim3(256), 0, st, d, dim);
  return hipGetLastError();
}

}  // namespace dse
