// dse_pairs.hip -- two-spin correlators of every pair of register bits (option pair_obs,
// dse_pair_observables).
//
// For register bits i < j and y = x ^ e_i ^ e_j, the raw sums of pair p = pair_index(i, j) are
//   [5 p + 0]     ZZ = sum_x |psi_x|^2 s_i(x) s_j(x)                       (s_b = 1/2 - bit_b)
//   [5 p + 1, 2]  ZQ = sum_{bit_i(x)=0, bit_j(x)=1} conj(psi_x) psi_y      <I+_i I-_j>
//   [5 p + 3, 4]  DQ = sum_{bit_i(x)=0, bit_j(x)=0} conj(psi_x) psi_y      <I+_i I+_j>
// and [5 NP] holds ||psi||^2 (NP = n (n - 1) / 2; zero up to the record's stride).  Each unordered
// amplitude pair {x, y} is visited once, from the side with bit_i(x) = 0; bit_j(x) then says
// whether the product belongs to ZQ or DQ, so one partner read serves both.
//
//   k_obs_pairs<L>      tiled registers: arguments and addressing are ObsTile's (dse_device.h)
//   k_dense_obs_pairs   the dense engine's columns, the non-uniform FFT's blocks, matrix mode's states
#include "dse_dense.h"
#include "dse_device.h"

namespace dse {
namespace {

// pairs whose per-wave sums wait in LDS for one reduction over the waves
constexpr int kPairBatch = 32;

// Per tile the S >= pair_stride(n_max) partial sums of the layout above.  The three routes to the
// partner amplitude are k_obs_sites' (register bit: another row of this thread; thread bit: LDS;
// bit >= L: the partner tile, obs_partner_tile):
//   i, j register bits   row r ^ e_i ^ e_j, chosen at compile time (the j and i loops unroll)
//   i or j a thread bit  LDS at idx ^ e_i ^ e_j
//   j >= L > i           tile hg ^ e_j, element idx ^ e_i
//   i, j >= L            tile hg ^ e_i ^ e_j, same element; tiles with bit_i = 1 skip the reads
// ZZ needs no partner: |psi|^2 with the two signs (a bit >= L gives the whole tile one sign).
// No thread holds more than one pair's five sums: they are reduced over the wave when formed, lane 0
// leaves them in s_red[slot][wave] (the pair's index in s_pair[slot]), and every kPairBatch pairs
// (and at the end) thread i adds entry i over the waves in order between two barriers.  Fixed
// order, no atomics: bitwise reproducible.
template <int L>
__global__ void __launch_bounds__(Geo<L>::NT)
k_obs_pairs(const DevProb* __restrict__ probs, const int2* __restrict__ items, int bsel_last,
            double* __restrict__ partial, size_t out_stride, int xq, int S) {
  using G = Geo<L>;
  constexpr int T = G::T, NT = G::NT, R = G::R, NW = NT / 64, TB = G::TB;
  __shared__ double2 s_w[T];
  __shared__ double s_red[kPairBatch][NW][5];
  __shared__ double s_n2[NW];
  __shared__ int s_pair[kPairBatch];

  const ObsTile<L> V = obs_tile<L>(probs, items, bsel_last, partial, out_stride, xq, S);
  const DevProb& P = V.P;
  const int tid = V.tid;
  const int n = P.n;
  const int np = n * (n - 1) / 2;

  double2 own[R];
  double p2[R];
  double p2sum = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    own[r] = make_double2(0.0, 0.0);
    if (V.live) {
      own[r] = V.psi[V.base + r * NT + tid];
      s_w[r * NT + tid] = own[r];
    }
    p2[r] = own[r].x * own[r].x + own[r].y * own[r].y;
    p2sum += p2[r];
  }
  __syncthreads();
  {
    double v = p2sum;
    wave_sum(v);
    if (V.lane0) s_n2[V.wv] = v;
  }

  int slot = 0;  // pairs waiting in s_red (uniform)
  auto flush = [&]() {
    __syncthreads();
    for (int i = tid; i < 5 * slot; i += NT) {
      const int s = i / 5, c = i - 5 * s;
      double v = 0.0;
      for (int w = 0; w < NW; ++w) v += s_red[s][w][c];
      V.partial[5 * s_pair[s] + c] = v;
    }
    __syncthreads();
    slot = 0;
  };
  // wave butterfly of the five sums of pair p (every lane takes part), lane 0 stores them
  auto wave_put = [&](int p, double zz, double qr, double qi, double dr, double di) {
    double v[5] = {zz, qr, qi, dr, di};
#pragma unroll
    for (int k = 0; k < 5; ++k) wave_sum(v[k]);
    if (V.lane0)
#pragma unroll
      for (int k = 0; k < 5; ++k) s_red[slot][V.wv][k] = v[k];
    if (tid == 0) s_pair[slot] = p;
    if (++slot == kPairBatch) flush();
  };

  // both bits register bits: the partner is another of this thread's rows
#pragma unroll
  for (int j = TB + 1; j < L; ++j) {
#pragma unroll
    for (int i = TB; i < j; ++i) {
      if (j >= n) continue;  // (uniform; no early exit, so the loops unroll around the wave shuffles)
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool i1 = (r >> (i - TB)) & 1, j1 = (r >> (j - TB)) & 1;
        v[0] += (i1 != j1 ? -0.25 : 0.25) * p2[r];
        if (i1) continue;
        const double2 s = own[r ^ (1 << (i - TB)) ^ (1 << (j - TB))];
        const double re = own[r].x * s.x + own[r].y * s.y, im = own[r].x * s.y - own[r].y * s.x;
        if (j1)
          v[1] += re, v[2] += im;
        else
          v[3] += re, v[4] += im;
      }
      wave_put(pair_index(i, j), v[0], v[1], v[2], v[3], v[4]);
    }
  }
  // i a thread bit, j any tile bit: LDS partner; the amplitudes with bit_j = 1 feed ZQ, the others DQ
  for (int j = 1; j < (L < n ? L : n); ++j) {
    for (int i = 0; i < (j < TB ? j : TB); ++i) {
      const bool i1 = (tid >> i) & 1;
      const uint32_t m = (1u << i) | (1u << j);
      double zz = 0.0, qr = 0.0, qi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t idx = (uint32_t)(r * NT + tid);
        const bool j1 = (idx >> j) & 1u;
        zz += (i1 != j1 ? -0.25 : 0.25) * p2[r];
        if (i1 || !V.live) continue;
        const double2 s = s_w[idx ^ m];
        const double re = own[r].x * s.x + own[r].y * s.y, im = own[r].x * s.y - own[r].y * s.x;
        qr += j1 ? re : 0.0;
        qi += j1 ? im : 0.0;
        dr += j1 ? 0.0 : re;
        di += j1 ? 0.0 : im;
      }
      wave_put(pair_index(i, j), zz, qr, qi, dr, di);
    }
  }
  // j above the tile: bit_j is the tile's
  for (int j = L; j < n; ++j) {
    const bool j1 = (V.hg >> (j - L)) & 1u;
    const uint32_t hj = V.hg ^ (1u << (j - L));
    for (int i = 0; i < j; ++i) {
      double zz = 0.0, ar = 0.0, ai = 0.0;
      if (i < L) {  // element idx ^ e_i of the tile hg ^ e_j
        const double2* src = obs_partner_tile(V, hj);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t idx = (uint32_t)(r * NT + tid);
          const bool i1 = (idx >> i) & 1u;
          zz += (i1 != j1 ? -0.25 : 0.25) * p2[r];
          if (i1 || !V.live) continue;
          const double2 s = src[idx ^ (1u << i)];
          ar += own[r].x * s.x + own[r].y * s.y;
          ai += own[r].x * s.y - own[r].y * s.x;
        }
      } else {  // the same element of the tile hg ^ e_i ^ e_j
        const bool i1 = (V.hg >> (i - L)) & 1u;
        zz = (i1 != j1 ? -0.25 : 0.25) * p2sum;
        if (!i1 && V.live) {  // (i1 uniform: the tiles holding bit_i = 1 read nothing)
          const double2* src = obs_partner_tile(V, hj ^ (1u << (i - L)));
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const double2 s = src[r * NT + tid];
            ar += own[r].x * s.x + own[r].y * s.y;
            ai += own[r].x * s.y - own[r].y * s.x;
          }
        }
      }
      wave_put(pair_index(i, j), zz, j1 ? ar : 0.0, j1 ? ai : 0.0, j1 ? 0.0 : ar, j1 ? 0.0 : ai);
    }
  }
  flush();  // (its first barrier also orders s_n2)
  for (int i = 5 * np + tid; i < S; i += NT) {
    double v = 0.0;
    if (i == 5 * np)
      for (int w = 0; w < NW; ++w) v += s_n2[w];
    V.partial[i] = v;
  }
}

// Pair sums of the dense engine's columns (option pair_obs; the columns' layout: DenseCols,
// dse_dense.h): P.pairs row t0 + j holds the record above, S doubles per row.  In the rotated
// frame (psi' = i^|x| psi) ZZ and ZQ are unchanged and DQ takes the factor -1: flipping two equal
// bits changes the popcount by 2.  One pass over the column per pair (the column stays in L2), its
// five sums reduced over the wave, then the four waves in order: no atomics.
__global__ void __launch_bounds__(256)
k_dense_obs_pairs(const DenseProb* __restrict__ probs, int dim, const double* __restrict__ Psi, size_t pstride,
                  size_t colstride, size_t imoff, int es, int t0, int S) {
  __shared__ double red[4][5];
  const DenseProb& P = probs[blockIdx.y];
  const int jcol = blockIdx.x;
  const auto [re, im] = dense_col(Psi, pstride, colstride, imoff, blockIdx.y, jcol);
  const int n = P.n;
  const int np = n * (n - 1) / 2;
  double* o = P.pairs + (size_t)(t0 + jcol) * S;
  const int w = threadIdx.x >> 6;
  const double dq_sign = P.rot ? -1.0 : 1.0;
  int bi = 0, bj = 1;  // pair p = (bi, bj); p == np: the norm alone
  for (int p = 0; p <= np; ++p) {
    double v[5] = {0, 0, 0, 0, 0};
    const uint32_t m = p < np ? (1u << bi) | (1u << bj) : 0u;
    for (uint32_t x = threadIdx.x; x < (uint32_t)dim; x += 256u) {
      const double ar = re[(size_t)x * es], ai = im[(size_t)x * es];
      const double q2 = ar * ar + ai * ai;
      if (p == np) {
        v[0] += q2;
        continue;
      }
      const bool i1 = (x >> bi) & 1u, j1 = (x >> bj) & 1u;
      v[0] += (i1 != j1 ? -0.25 : 0.25) * q2;
      if (i1) continue;
      const uint32_t y = x ^ m;
      const double br = re[(size_t)y * es], bim = im[(size_t)y * es];
      const double zr = ar * br + ai * bim, zi = ar * bim - ai * br;  // conj(a) b
      if (j1)
        v[1] += zr, v[2] += zi;
      else
        v[3] += dq_sign * zr, v[4] += dq_sign * zi;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int k = 0; k < 5; ++k) red[w][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 5) {
      const double t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
      if (p < np)
        o[5 * p + threadIdx.x] = t;
      else if (threadIdx.x == 0)
        o[5 * np] = t;
    }
    __syncthreads();
    if (++bi == bj) bi = 0, ++bj;
  }
  for (int i = 5 * np + 1 + threadIdx.x; i < S; i += 256) o[i] = 0.0;
}

}  // namespace

hipError_t launch_obs_pairs(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                            double* partial, int S, hipStream_t st, int n_out, size_t out_stride, int xq) {
  if (n_items <= 0 || n_out <= 0) return hipSuccess;
  if ((n_out > 1 && bsel >= 3) || S < 2) return hipErrorInvalidValue;
  return for_tile_bits(L, [&](auto l) {
    hipLaunchKernelGGL((k_obs_pairs<l()>), dim3(n_items, n_out), dim3(Geo<l()>::NT), 0, st, probs, items, bsel,
                       partial, out_stride, xq, S);
    return hipGetLastError();
  });
}

hipError_t launch_dense_obs_pairs(const DenseProb* d, int count, int dim, const DenseCols& cols, int tb, int t0,
                                  int S, hipStream_t st) {
  hipLaunchKernelGGL(k_dense_obs_pairs, dim3(tb, count), dim3(256), 0, st, d, dim, cols.Psi, cols.pstride,
                     cols.colstride, cols.imoff, cols.es, t0, S);
  return hipGetLastError();
}

}  // namespace dse
