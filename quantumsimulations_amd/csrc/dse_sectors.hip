// dse_sectors.hip -- populations of the sectors of a total spin projection (dse_set_sectors,
// dse_sector_values, dse_get_sectors).
//
// A sector set is three masks over register bits (SectorEntry): m the counted bits, cm the selecting
// bits, cv their required values.  Its raw sums on a state psi are the B = popcount(m) + 1 bins
//   bin_j = sum_{x : (x & cm) == cv, popcount(x & m) == j} |psi_x|^2.
// The record of a state: the bins of set k at [off_k + j], U = sum_k B_k in all, ||psi||^2 at
// [S - 2], zero elsewhere up to S = sector_stride(U_max) of the context.
//
//   k_obs_sectors<L>      tiled registers: arguments and addressing are ObsTile's (dse_device.h)
//   k_dense_obs_sectors   the dense engine's columns, the non-uniform FFT's blocks, matrix mode's states
// (the small engine: small_sector_sums, dse_small.hip)
#include "dse_dense.h"
#include "dse_device.h"

namespace dse {
namespace {

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

// Thread t of the tile's NT loads its R amplitudes idx = r * NT + t once and keeps only |psi|^2: a bin
// needs no partner, so the tile is not staged in LDS.  Per set (the table is read at run time, uniform
// loads) the selection's in-tile part zeroes the amplitudes that fail it and sector_wave_bins merges
// the rest over the row bits and the lane bits into the wave's LR + 7 partial bins, indexed by the
// number of counted row and lane bits set; lane 0 leaves them in s_bin[set][wave].  After one barrier
// thread i forms unit i: the waves in order, wave w's vector shifted by popcount(w & m's wave bits),
// everything shifted by the tile's own counted bits popcount(hg & (m >> L)), so the elementwise sum
// over tiles (flush_partials) gives the register's bins.  Selecting bits at or above L are the tile's
// own: a tile that fails them skips the set and writes zeros.  No atomics, every sum in a fixed
// order: bitwise reproducible.  A register without sets returns at once (uniform: K is the problem's).
template <int L>
__global__ void __launch_bounds__(Geo<L>::NT)
k_obs_sectors(const DevProb* __restrict__ probs, const int2* __restrict__ items, int bsel_last,
              double* __restrict__ partial, size_t out_stride, int xq, int S) {
  using G = Geo<L>;
  constexpr int T = G::T, NT = G::NT, R = G::R, NW = NT / 64, LR = ilog2(R), VL = LR + 7;
  constexpr int LGNT = G::LGNT;
  constexpr uint32_t TM = (uint32_t)T - 1u;
  __shared__ double s_bin[kMaxSectorSets][NW][VL];
  __shared__ double s_nrm[NW];

  const ObsTile<L> V = obs_tile<L>(probs, items, bsel_last, partial, out_stride, xq, S);
  const DevProb& P = V.P;
  const int K = P.sec_k;
  if (K <= 0) return;
  const int tid = V.tid;
  const SectorEntry* __restrict__ tab = P.sec_tab;

  double p2[R];
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    p2[r] = 0.0;
    if (V.live) {
      const double2 a = V.psi[V.base + r * NT + tid];
      p2[r] = a.x * a.x + a.y * a.y;
    }
    n2 += p2[r];
  }
  wave_sum(n2);
  if (V.lane0) s_nrm[V.wv] = n2;

#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const uint64_t m = tab[k].m, cm = tab[k].cm, cv = tab[k].cv;
    if ((V.hg & (uint32_t)(cm >> L)) != (uint32_t)(cv >> L)) continue;  // (uniform: the tile's selecting bits)
    const uint32_t m_lo = (uint32_t)m & TM, cm_lo = (uint32_t)cm & TM, cv_lo = (uint32_t)cv & TM;
    double q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) q[r] = (((uint32_t)(r * NT + tid)) & cm_lo) == cv_lo ? p2[r] : 0.0;
    double v[VL];
    sector_wave_bins<LR>(q, m_lo >> LGNT, m_lo & 63u, v);
    if (V.lane0) {
#pragma unroll
      for (int c = 0; c < VL; ++c) s_bin[k][V.wv][c] = v[c];
    }
  }
  __syncthreads();
  const int U = tab[K - 1].off + tab[K - 1].bins;
  for (int i = tid; i < S; i += NT) {
    double v = 0.0;
    if (i < U) {
      int k = 0;
      while (k + 1 < K && i >= tab[k + 1].off) ++k;
      const uint64_t m = tab[k].m, cm = tab[k].cm, cv = tab[k].cv;
      if ((V.hg & (uint32_t)(cm >> L)) == (uint32_t)(cv >> L)) {
        const uint32_t m_wv = ((uint32_t)m & TM) >> 6;
        const int c0 = i - tab[k].off - __popc(V.hg & (uint32_t)(m >> L));
        for (int w = 0; w < NW; ++w) {
          const int c = c0 - __popc((uint32_t)w & m_wv);
          if (c >= 0 && c < VL) v += s_bin[k][w][c];
        }
      }
    } else if (i == S - 2) {
      for (int w = 0; w < NW; ++w) v += s_nrm[w];
    }
    V.partial[i] = v;
  }
}

// Sector populations of the dense engine's columns (the columns' layout: DenseCols, dse_dense.h; one
// workgroup per column): P.secs row t0 + j holds the record above, S doubles per row.  The rotated
// frame (P.rot: psi' = i^|x| psi) needs nothing here: |psi'_x| = |psi_x|, and the psi0 phase and the
// shift's phase have modulus 1.  One pass over the column per set (the column stays in L2) and one
// for the norm: a thread adds its |psi_x|^2 to every bin of a register vector under a compile-time
// index (to the bin popcount(x & m) the value, to the others zero), the bins are reduced over the
// wave, then the four waves in order: no atomics.
constexpr int kDenseBins = kDenseMaxQubits + 1;
__global__ void __launch_bounds__(256)
k_dense_obs_sectors(const DenseProb* __restrict__ probs, int dim, const double* __restrict__ Psi, size_t pstride,
                    size_t colstride, size_t imoff, int es, int t0, int S) {
  __shared__ double red[4][kDenseBins];
  const DenseProb& P = probs[blockIdx.y];
  const int K = P.sec_k;
  if (K <= 0 || !P.secs) return;
  const int j = blockIdx.x;
  const auto [re, im] = dense_col(Psi, pstride, colstride, imoff, blockIdx.y, j);
  double* o = P.secs + (size_t)(t0 + j) * S;
  const int w = threadIdx.x >> 6;
  const int U = P.sec_tab[K - 1].off + P.sec_tab[K - 1].bins;
  for (int k = 0; k <= K; ++k) {  // k == K: the norm alone (one bin, nothing selected or counted)
    const bool set = k < K;
    const uint32_t m = set ? (uint32_t)P.sec_tab[k].m : 0u;
    const uint32_t cm = set ? (uint32_t)P.sec_tab[k].cm : 0u, cv = set ? (uint32_t)P.sec_tab[k].cv : 0u;
    double v[kDenseBins];
#pragma unroll
    for (int c = 0; c < kDenseBins; ++c) v[c] = 0.0;
    for (uint32_t x = threadIdx.x; x < (uint32_t)dim; x += 256u) {
      if ((x & cm) != cv) continue;
      const double ar = re[(size_t)x * es], ai = im[(size_t)x * es];
      const double p = ar * ar + ai * ai;
      const int b = __popc(x & m);
#pragma unroll
      for (int c = 0; c < kDenseBins; ++c) v[c] += b == c ? p : 0.0;
    }
#pragma unroll
    for (int c = 0; c < kDenseBins; ++c) {
      wave_sum(v[c]);
      if ((threadIdx.x & 63) == 0) red[w][c] = v[c];
    }
    __syncthreads();
    const int bins = set ? P.sec_tab[k].bins : 1;
    if ((int)threadIdx.x < bins)
      o[set ? P.sec_tab[k].off + threadIdx.x : S - 2] =
          red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    __syncthreads();
  }
  for (int i = U + threadIdx.x; i < S; i += 256)
    if (i != S - 2) o[i] = 0.0;
}

}  // namespace

hipError_t launch_obs_sectors(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                              double* partial, int S, hipStream_t st, int n_out, size_t out_stride, int xq) {
  if (n_items <= 0 || n_out <= 0) return hipSuccess;
  if ((n_out > 1 && bsel >= 3) || S < 3 || S > sector_stride(kMaxSectorSets * (kMaxQubits + 1)))
    return hipErrorInvalidValue;
  return for_tile_bits(L, [&](auto l) {
    hipLaunchKernelGGL((k_obs_sectors<l()>), dim3(n_items, n_out), dim3(Geo<l()>::NT), 0, st, probs, items, bsel,
                       partial, out_stride, xq, S);
    return hipGetLastError();
  });
}

hipError_t launch_dense_obs_sectors(const DenseProb* d, int count, int dim, const DenseCols& cols, int tb, int t0,
                                    int S, hipStream_t st) {
  if (dim > (1 << kDenseMaxQubits)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dense_obs_sectors, dim3(tb, count), dim3(256), 0, st, d, dim, cols.Psi, cols.pstride,
                     cols.colstride, cols.imoff, cols.es, t0, S);
  return hipGetLastError();
}

}  // namespace dse
