// dse_overlap.hip -- overlaps of a register's state with its stored reference states
// (dse_set_overlap_refs, dse_overlaps, dse_get_overlaps).
//
// A register carries K <= kMaxOverlapRefs reference states phi_0 .. phi_{K-1} (DevProb::ovl_refs: K
// device pointers, each to the 2^n_local amplitudes of this register or shard).  The raw sums of a
// state psi are
//   [2 k], [2 k + 1]   Re, Im of sum_x conj(phi_k(x)) psi_x
//   [S - 2]            ||psi||^2                      (S = overlap_stride(K_max) of the context)
// and zero elsewhere up to S.  Unlike every other observable of the engine the sum is not invariant
// under psi -> e^{i theta} psi: it carries the phase of the state the engine defines.
//
//   k_obs_overlap<L>    tiled registers: arguments and addressing are ObsTile's (dse_device.h)
// (the dense engine's columns: k_dense_obs_overlap, dse_dense.hip, beside the phases it restores;
// the small engine: small_overlap_sums, dse_small.hip)
#include "dse_device.h"

namespace dse {
namespace {

// A streaming kernel: thread t of the tile's NT loads its R amplitudes x = r * NT + t of psi once
// (16-byte loads, consecutive lanes consecutive amplitudes) and keeps them in registers, then the K
// reference tiles stream past them the same way: (1 + K) 16 B per amplitude, no partner tile, no
// LDS but the reduction scratch.  Each reference's two sums are reduced over the wave when formed
// (xor butterfly), lane 0 leaves them in s_red[k][wave]; after one barrier thread i adds entry i
// over the waves in order.  No atomics: bitwise reproducible.  A register without references
// returns at once (uniform: K is the problem's).
template <int L>
__global__ void __launch_bounds__(Geo<L>::NT)
k_obs_overlap(const DevProb* __restrict__ probs, const int2* __restrict__ items, int bsel_last,
              double* __restrict__ partial, size_t out_stride, int xq, int S) {
  using G = Geo<L>;
  constexpr int NT = G::NT, R = G::R, NW = NT / 64;
  __shared__ double s_red[2 * kMaxOverlapRefs + 1][NW];

  const ObsTile<L> V = obs_tile<L>(probs, items, bsel_last, partial, out_stride, xq, S);
  const DevProb& P = V.P;
  const int K = P.ovl_k;
  if (K <= 0) return;
  const int tid = V.tid;
  const gd2* gpsi = gptr(V.psi + V.base);

  double2 own[R];
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    own[r] = V.live ? gld(gpsi, r * NT + tid) : make_double2(0.0, 0.0);
    n2 += own[r].x * own[r].x + own[r].y * own[r].y;
  }
  wave_sum(n2);
  if (V.lane0) s_red[2 * kMaxOverlapRefs][V.wv] = n2;

#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const gd2* gref = gptr(P.ovl_refs[k] + V.base);
    double2 f[R];
#pragma unroll
    for (int r = 0; r < R; ++r) f[r] = V.live ? gld(gref, r * NT + tid) : make_double2(0.0, 0.0);
    double re = 0.0, im = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {  // conj(phi) psi
      re += f[r].x * own[r].x + f[r].y * own[r].y;
      im += f[r].x * own[r].y - f[r].y * own[r].x;
    }
    wave_sum(re, im);
    if (V.lane0) {
      s_red[2 * k][V.wv] = re;
      s_red[2 * k + 1][V.wv] = im;
    }
  }
  __syncthreads();
  for (int i = tid; i < S; i += NT) {
    const int src = i < 2 * K ? i : (i == S - 2 ? 2 * kMaxOverlapRefs : -1);
    double v = 0.0;
    if (src >= 0)
      for (int w = 0; w < NW; ++w) v += s_red[src][w];
    V.partial[i] = v;
  }
}

}  // namespace

hipError_t launch_obs_overlap(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                              double* partial, int S, hipStream_t st, int n_out, size_t out_stride, int xq) {
  if (n_items <= 0 || n_out <= 0) return hipSuccess;
  if ((n_out > 1 && bsel >= 3) || S < 4 || S > overlap_stride(kMaxOverlapRefs)) return hipErrorInvalidValue;
  return for_tile_bits(L, [&](auto l) {
    hipLaunchKernelGGL((k_obs_overlap<l()>), dim3(n_items, n_out), dim3(Geo<l()>::NT), 0, st, probs, items, bsel,
                       partial, out_stride, xq, S);
    return hipGetLastError();
  });
}

}  // namespace dse
