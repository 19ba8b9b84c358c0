// dse_pulse.hip -- hard pulses on the device state (dse_apply_pulse, dse_pulse_plan; include/dse.h,
// feature "pulse"): U = (x)_b U_b, one complex 2x2 matrix per register bit, applied in place to a
// state of 2^n amplitudes in one buffer or in the 2^S buffers of a loopback register.
//
// A pass is one plain launch of k_pulse.  Every workgroup owns the 2^12 amplitudes that differ in the
// pass's 12 tile bits only: a set closed under flips of those bits, so a pass runs in place and no
// workgroup waits for another (no flags, no polls, no cooperative launch).  The tile is read once
// and written once (32 B per amplitude).  The host plan (pulse_plan) puts the low 12 bits in group 0
// and the higher bits with a non-diagonal matrix in groups of up to 10, each completed by the lowest
// c >= 2 bits (carried, not transformed) so that global accesses stay in runs of 16 c-bit = 64 B or
// more; shard bits are high bits that select one of the base pointers.  A group without a
// non-diagonal bit is not launched.  Diagonal matrices never need a butterfly: all of them are
// folded into one phase per amplitude in the first pass that runs (a factor per thread for the bits
// it holds fixed, times one complex multiply per register bit), and a pulse of diagonal matrices
// only is one pass without any LDS traffic.
//
// Inside a tile a thread holds 16 amplitudes and transforms four tile bits at a time in registers:
//   round 1  registers = tile bits 8..11, thread = tile bits 0..7 (the load layout: lanes along the
//            low bits, 16-B loads, a wave instruction covers whole runs)
//   round 2  registers = tile bits 0..3,  thread = tile bits 4..11
//   round 3  registers = tile bits 4..7,  thread = tile bits 0..3 | 8..11 (the store layout: 16
//            lanes along the low bits)
// with one LDS exchange between two rounds (two per pass: 4 x 64 KiB of LDS traffic per 128 KiB of
// HBM traffic; one exchange per bit would be 24 x).  An exchange that no butterfly needs is skipped.
// The LDS slot of tile index i is i ^ ((i >> 4) & 15): in each of the four access patterns the lanes
// that a 16-B LDS access serves together (the four 16-lane groups of a read, the eight runs of 8
// lanes of a write) then fall on distinct banks, by construction (not measured with counters).
// 64 KiB of LDS per workgroup: two workgroups share a CU, one's loads run under the other's rounds.
//
// Every sum runs in a fixed order and there are no atomics: repeated runs are bitwise equal.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/dse.h"
#include "dse_internal.h"

namespace dse {

namespace {

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// (a, b) <- U (a, b), u = (re u00, im u00, re u01, im u01, re u10, im u10, re u11, im u11)
__device__ __forceinline__ void bfly(double2& a, double2& b, const double* u) {
  const double2 x = a, y = b;
  a.x = fma(u[2], y.x, fma(-u[3], y.y, fma(u[0], x.x, -(u[1] * x.y))));
  a.y = fma(u[2], y.y, fma(u[3], y.x, fma(u[0], x.y, u[1] * x.x)));
  b.x = fma(u[6], y.x, fma(-u[7], y.y, fma(u[4], x.x, -(u[5] * x.y))));
  b.y = fma(u[6], y.y, fma(u[7], y.x, fma(u[4], x.y, u[5] * x.x)));
}

// the butterflies of the four register bits whose tile bits are q0 .. q0 + 3
template <int q0>
__device__ __forceinline__ void round_bits(double2 (&a)[16], const PulsePass& P) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!((P.bfly >> (q0 + j)) & 1u)) continue;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (!((k >> j) & 1)) bfly(a[k], a[k | (1 << j)], P.u[q0 + j]);
  }
}

__device__ __forceinline__ int slot(int i) { return i ^ ((i >> 4) & 15); }

// the amplitude of global index g (bits >= n_local: the shard)
__device__ __forceinline__ double2* amp_ptr(const PulseTab* __restrict__ tab, const PulsePass& P, uint64_t g) {
  if (P.shard_bits == 0) return P.base0 + g;
  return tab->base[g >> P.n_local] + (g & ((uint64_t(1) << P.n_local) - 1));
}

// the register-bit offsets of the 16 amplitudes of a thread: register bit j = tile bit q0 + j
template <int q0>
__device__ __forceinline__ uint64_t reg_off(const PulsePass& P, int k) {
  uint64_t o = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) o |= (uint64_t)((k >> j) & 1) << P.pos[q0 + j];
  return o;
}

__global__ void __launch_bounds__(256)
k_pulse(const PulseTab* __restrict__ tab, const PulsePass P) {
  __shared__ double2 lds[kPulseTile];
  const int t = threadIdx.x;
  // the workgroup's bits: blockIdx.x spread over the register bits outside the tile
  uint64_t wg = 0;
  {
    uint64_t m = P.outer, b = blockIdx.x;
    while (m) {
      const uint64_t low = m & (~m + 1);
      if (b & 1) wg |= low;
      b >>= 1;
      m ^= low;
    }
  }
  uint64_t gt = wg;
#pragma unroll
  for (int j = 0; j < 8; ++j) gt |= (uint64_t)((t >> j) & 1) << P.pos[j];
  double2 a[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) a[k] = *amp_ptr(tab, P, gt | reg_off<8>(P, k));

  if (P.diag) {  // the phase of every diagonal matrix, in the first pass that runs
    uint64_t regmask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) regmask |= uint64_t(1) << P.pos[8 + j];
    const uint64_t fixed = P.diag & ~regmask;  // the bits this thread holds fixed
    if (fixed) {
      double2 f = make_double2(1.0, 0.0);
      uint64_t m = fixed;
      while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        const double* d = tab->d[b] + 2 * (int)((gt >> b) & 1);
        f = cmul(f, make_double2(d[0], d[1]));
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = cmul(a[k], f);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = P.pos[8 + j];
      if (!((P.diag >> b) & 1)) continue;
      const double2 d0 = make_double2(tab->d[b][0], tab->d[b][1]), d1 = make_double2(tab->d[b][2], tab->d[b][3]);
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = cmul(a[k], ((k >> j) & 1) ? d1 : d0);
    }
  }

  round_bits<8>(a, P);
  if ((P.bfly & 0xffu) == 0) {  // nothing left: store in the load layout
#pragma unroll
    for (int k = 0; k < 16; ++k) *amp_ptr(tab, P, gt | reg_off<8>(P, k)) = a[k];
    return;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) lds[slot(k * 256 + t)] = a[k];
  __syncthreads();
  if (P.bfly & 0x00fu) {
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = lds[slot(t * 16 + k)];
    round_bits<0>(a, P);
#pragma unroll
    for (int k = 0; k < 16; ++k) lds[slot(t * 16 + k)] = a[k];
    __syncthreads();
  }
  const int hi = t >> 4, lo = t & 15;
#pragma unroll
  for (int k = 0; k < 16; ++k) a[k] = lds[slot((hi << 8) | (k << 4) | lo)];
  round_bits<4>(a, P);
  uint64_t gs = wg;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    gs |= (uint64_t)((lo >> j) & 1) << P.pos[j];
    gs |= (uint64_t)((hi >> j) & 1) << P.pos[8 + j];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) *amp_ptr(tab, P, gs | reg_off<4>(P, k)) = a[k];
}

// Registers of fewer than 2^12 amplitudes: one workgroup, the state in LDS, one bit after another.
__global__ void __launch_bounds__(256)
k_pulse_small(const PulseTab* __restrict__ tab, int n, int n_local, uint64_t bfly_mask, uint64_t diag) {
  __shared__ double2 s[kPulseTile / 2];
  const int t = threadIdx.x;
  const int dim = 1 << n;
  const int lmask = (1 << n_local) - 1;
  for (int x = t; x < dim; x += 256) {
    double2 v = tab->base[x >> n_local][x & lmask];
    uint64_t m = diag;
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      const double* d = tab->d[b] + 2 * ((x >> b) & 1);
      v = cmul(v, make_double2(d[0], d[1]));
    }
    s[x] = v;
  }
  __syncthreads();
  for (int b = 0; b < n; ++b) {
    if (!((bfly_mask >> b) & 1)) continue;
    for (int p = t; p < dim / 2; p += 256) {
      const int x0 = ((p >> b) << (b + 1)) | (p & ((1 << b) - 1));
      bfly(s[x0], s[x0 | (1 << b)], tab->u[b]);
    }
    __syncthreads();
  }
  for (int x = t; x < dim; x += 256) tab->base[x >> n_local][x & lmask] = s[x];
}

}  // namespace

// The passes of a pulse on a register of n_local local and shard_bits shard bits (bit b >= n_local:
// shard bit b - n_local).  active: the bits whose matrix is not the identity; diag: those of them whose
// matrix is diagonal.  Returns the number of passes (0: the identity).
int pulse_plan(int n_local, int shard_bits, uint64_t active, uint64_t diag, PulsePlan& plan) {
  std::memset(&plan, 0, sizeof(plan));
  const int n = n_local + shard_bits;
  const uint64_t nd = active & ~diag;
  if (!active) return 0;
  if (n < kPulseTB) {  // k_pulse_small
    PulseGroup& G = plan.grp[0];
    for (int q = 0; q < kPulseTB; ++q) G.pos[q] = q < n ? q : -1;
    G.bfly = (uint32_t)nd;
    G.active = active;
    plan.small = true;
    return plan.passes = 1;
  }
  const uint64_t low = (uint64_t(1) << kPulseTB) - 1;
  int g = 0;
  if ((nd & low) || !(nd & ~low)) {  // group 0, also the pass of a pulse of diagonal matrices only
    PulseGroup& G = plan.grp[g++];
    for (int q = 0; q < kPulseTB; ++q) G.pos[q] = q;
    G.bfly = (uint32_t)(nd & low);
    G.active = nd & low ? nd & low : diag;
  }
  int high[kMaxQubits], nh = 0;
  for (int b = kPulseTB; b < n; ++b)
    if ((nd >> b) & 1) high[nh++] = b;
  const int per = kPulseTB - kPulseMinCarry;
  const int ng = (nh + per - 1) / per;
  for (int i = 0, at = 0; i < ng; ++i) {  // the high bits spread evenly over the fewest groups
    const int h = (nh - at + (ng - i) - 1) / (ng - i);
    PulseGroup& G = plan.grp[g++];
    G.c = kPulseTB - h;
    for (int q = 0; q < G.c; ++q) G.pos[q] = q;
    for (int q = G.c; q < kPulseTB; ++q) {
      G.pos[q] = high[at++];
      G.bfly |= 1u << q;
      G.active |= uint64_t(1) << G.pos[q];
    }
  }
  return plan.passes = g;
}

// Applies the pulse u[8 n] to the state in base[0 .. 2^shard_bits) (2^n_local amplitudes each) on st.
// tab: device memory of the call (sizeof(PulseTab)), written here with a blocking copy.
hipError_t launch_pulse(double2* const* base, int n_local, int shard_bits, const double* u, uint64_t active,
                        uint64_t diag, PulseTab* tab, hipStream_t st, int* passes) {
  const int n = n_local + shard_bits;
  *passes = 0;
  if (n < 1 || n > kMaxQubits || shard_bits < 0 || shard_bits > kMaxShardBits || n_local < 1)
    return hipErrorInvalidValue;
  PulsePlan plan;
  const int np = pulse_plan(n_local, shard_bits, active, diag, plan);
  if (np == 0) return hipSuccess;
  PulseTab h;
  std::memset(&h, 0, sizeof(h));
  for (int i = 0; i < (1 << shard_bits); ++i) h.base[i] = base[i];
  for (int b = 0; b < n; ++b) {
    std::memcpy(h.u[b], u + 8 * b, 8 * sizeof(double));
    h.d[b][0] = u[8 * b], h.d[b][1] = u[8 * b + 1], h.d[b][2] = u[8 * b + 6], h.d[b][3] = u[8 * b + 7];
  }
  hipError_t e = hipMemcpy(tab, &h, sizeof(h), hipMemcpyHostToDevice);
  if (e != hipSuccess) return e;
  if (plan.small) {
    hipLaunchKernelGGL(k_pulse_small, dim3(1), dim3(256), 0, st, tab, n, n_local, (uint64_t)plan.grp[0].bfly, diag);
    *passes = 1;
    return hipGetLastError();
  }
  const uint64_t all = (uint64_t(1) << n) - 1;
  for (int g = 0; g < np; ++g) {
    const PulseGroup& G = plan.grp[g];
    PulsePass P;
    std::memset(&P, 0, sizeof(P));
    uint64_t tile = 0;
    for (int q = 0; q < kPulseTB; ++q) {
      P.pos[q] = G.pos[q];
      tile |= uint64_t(1) << G.pos[q];
      std::memcpy(P.u[q], u + 8 * G.pos[q], 8 * sizeof(double));
    }
    P.base0 = base[0];
    P.outer = all & ~tile;
    P.diag = g == 0 ? diag : 0;
    P.bfly = G.bfly;
    P.n_local = n_local;
    P.shard_bits = shard_bits;
    const uint64_t blocks = uint64_t(1) << (n - kPulseTB);
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pulse, dim3((unsigned)blocks), dim3(256), 0, st, (const PulseTab*)tab, P);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++*passes;
  }
  return hipSuccess;
}

}  // namespace dse

extern "C" int dse_pulse_plan(int n_local, int shard_bits, uint64_t active_mask, uint64_t diag_mask, int32_t* groups_out) {
  using namespace dse;
  const int n = n_local + shard_bits;
  if (!groups_out || n_local < 1 || shard_bits < 0 || shard_bits > kMaxShardBits || n > kMaxQubits) return DSE_ERR_ARG;
  const uint64_t all = (uint64_t(1) << n) - 1;
  if ((active_mask & ~all) || (diag_mask & ~active_mask)) return DSE_ERR_ARG;
  PulsePlan plan;
  const int np = pulse_plan(n_local, shard_bits, active_mask, diag_mask, plan);
  for (int g = 0; g < np; ++g) {
    int32_t* o = groups_out + 14 * g;
    o[0] = plan.grp[g].c;
    for (int q = 0; q < kPulseTB; ++q) o[1 + q] = plan.grp[g].pos[q];
    o[13] = (int32_t)plan.grp[g].bfly;
  }
  return np;
}
