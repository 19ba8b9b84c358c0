// dse_strings.hip -- expectation values of operator strings: products of one-spin operators, one
// factor per register bit (dse_set_op_strings, dse_op_string_values, dse_get_op_strings).
//
// The host compiles a string into four masks and a prefactor (dse_op_string_masks; StringEntry):
//   xm  bits that flip (Ix, Iy, I+, I-)          zm  bits that sign (Iz, Iy)
//   cm  bits that select (I+, I-, Ea, Eb)        cv  their value in the row x (I-, Eb: 1)
// and the raw sum of string k on a state psi is
//   S_k = pre_k sum_{x : (x & cm) == cv} (-1)^popcount(x & zm) conj(psi_x) psi_{x ^ xm}.
// The record of a state: Re, Im of S_k at [2 k], [2 k + 1] for k < K, ||psi||^2 at [S - 2], zero
// elsewhere up to S = string_stride(K_max) of the context.
//
//   k_obs_strings<L>      tiled registers: arguments and addressing are ObsTile's (dse_device.h)
//   k_dense_obs_strings   the dense engine's columns, the non-uniform FFT's blocks, matrix mode's states
// (the small engine: small_string_sums, dse_small.hip)
#include "dse_dense.h"
#include "dse_device.h"

namespace dse {
namespace {

// Thread t of the tile's NT loads its R amplitudes idx = r * NT + t once, keeps them and |psi|^2 in
// registers and stages the tile in LDS.  The table is read at run time (uniform loads), so the
// route to the partner is chosen per string from its flip mask, split at the tile size:
//   xm == 0           no partner: signed, selected |psi|^2
//   xm >> L == 0      LDS at idx ^ xm_lo (thread and row bits alike: nothing indexed by the string
//                     sits in a per-thread array)
//   xm >> L != 0      tile hg ^ xm_hi (obs_partner_tile), element idx ^ xm_lo: a xor of lane indices
//                     permutes within aligned runs, so the loads stay coalesced
// Selected and signing bits at or above L are the tile's own: a tile that fails the selection reads
// nothing and contributes zeros; the tile's sign multiplies the finished sums.  Each string's two
// sums are reduced over the wave when formed (xor butterfly), lane 0 leaves them in s_red[.][wave];
// after one barrier thread i adds entry i over the waves in order and applies the prefactor.  No
// atomics: bitwise reproducible.  A register without strings returns at once (uniform: K is the
// problem's).
template <int L>
__global__ void __launch_bounds__(Geo<L>::NT)
k_obs_strings(const DevProb* __restrict__ probs, const int2* __restrict__ items, int bsel_last,
              double* __restrict__ partial, size_t out_stride, int xq, int S) {
  using G = Geo<L>;
  constexpr int T = G::T, NT = G::NT, R = G::R, NW = NT / 64;
  constexpr uint32_t TM = (uint32_t)T - 1u;
  __shared__ double2 s_w[T];
  __shared__ double s_red[2 * kMaxOpStrings + 1][NW];

  const ObsTile<L> V = obs_tile<L>(probs, items, bsel_last, partial, out_stride, xq, S);
  const DevProb& P = V.P;
  const int K = P.str_k;
  if (K <= 0) return;
  const int tid = V.tid;
  const StringEntry* __restrict__ tab = P.str_tab;

  double2 own[R];
  double p2[R];
  double n2 = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    own[r] = make_double2(0.0, 0.0);
    if (V.live) {
      own[r] = V.psi[V.base + r * NT + tid];
      s_w[r * NT + tid] = own[r];
    }
    p2[r] = own[r].x * own[r].x + own[r].y * own[r].y;
    n2 += p2[r];
  }
  __syncthreads();
  wave_sum(n2);
  if (V.lane0) s_red[2 * kMaxOpStrings][V.wv] = n2;

#pragma unroll 1
  for (int k = 0; k < K; ++k) {
    const uint64_t xm = tab[k].xm, zm = tab[k].zm, cm = tab[k].cm, cv = tab[k].cv;
    const uint32_t xm_lo = (uint32_t)xm & TM, xm_hi = (uint32_t)(xm >> L);
    const uint32_t zm_lo = (uint32_t)zm & TM, cm_lo = (uint32_t)cm & TM, cv_lo = (uint32_t)cv & TM;
    double re = 0.0, im = 0.0;
    if ((V.hg & (uint32_t)(cm >> L)) == (uint32_t)(cv >> L)) {  // (uniform: the tile's selected bits)
      if (xm == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t idx = (uint32_t)(r * NT + tid);
          const double q = (idx & cm_lo) == cv_lo ? p2[r] : 0.0;
          re += par32(idx & zm_lo) ? -q : q;
        }
      } else if (V.live) {
        const double2* src = xm_hi ? obs_partner_tile(V, V.hg ^ xm_hi) : s_w;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t idx = (uint32_t)(r * NT + tid);
          if ((idx & cm_lo) != cv_lo) continue;
          const double2 s = src[idx ^ xm_lo];
          const double zr = own[r].x * s.x + own[r].y * s.y, zi = own[r].x * s.y - own[r].y * s.x;  // conj(own) s
          const bool neg = par32(idx & zm_lo);
          re += neg ? -zr : zr;
          im += neg ? -zi : zi;
        }
      }
      if (par32(V.hg & (uint32_t)(zm >> L))) re = -re, im = -im;
    }
    wave_sum(re, im);
    if (V.lane0) {
      s_red[2 * k][V.wv] = re;
      s_red[2 * k + 1][V.wv] = im;
    }
  }
  __syncthreads();
  for (int i = tid; i < S; i += NT) {
    double v = 0.0;
    if (i < 2 * K) {
      const int k = i >> 1;
      double sr = 0.0, si = 0.0;
      for (int w = 0; w < NW; ++w) sr += s_red[2 * k][w], si += s_red[2 * k + 1][w];
      const double pr = tab[k].pre_re, pi = tab[k].pre_im;
      v = (i & 1) ? pr * si + pi * sr : pr * sr - pi * si;
    } else if (i == S - 2) {
      for (int w = 0; w < NW; ++w) v += s_red[2 * kMaxOpStrings][w];
    }
    V.partial[i] = v;
  }
}

// Operator strings of the dense engine's columns (the columns' layout: DenseCols, dse_dense.h; one
// workgroup per column): P.strs row t0 + j holds the record above, S doubles per row.  In the rotated
// frame (P.rot: psi' = i^|x| psi) conj(psi_x) psi_{x ^ xm} = (-i)^|xm| (-1)^|x & xm| conj(psi'_x)
// psi'_{x ^ xm}, so the same sum holds with zm' = zm ^ xm and pre' = pre (-i)^popcount(xm) (I+ I+:
// the pair kernel's factor -1; I+ I-: none); the psi0 phase and the shift's phase are the same for
// every x and cancel.  One pass over the column per string (the column stays in L2) and one for the
// norm, the sums reduced over the wave, then the four waves in order: no atomics.
__global__ void __launch_bounds__(256)
k_dense_obs_strings(const DenseProb* __restrict__ probs, int dim, const double* __restrict__ Psi, size_t pstride,
                    size_t colstride, size_t imoff, int es, int t0, int S) {
  __shared__ double red[4][2];
  const DenseProb& P = probs[blockIdx.y];
  const int K = P.str_k;
  if (K <= 0 || !P.strs) return;
  const int j = blockIdx.x;
  const auto [re, im] = dense_col(Psi, pstride, colstride, imoff, blockIdx.y, j);
  double* o = P.strs + (size_t)(t0 + j) * S;
  const int w = threadIdx.x >> 6;
  for (int k = 0; k <= K; ++k) {  // k == K: the norm alone
    const bool str = k < K;
    const uint32_t xm = str ? (uint32_t)P.str_tab[k].xm : 0u;
    const uint32_t cm = str ? (uint32_t)P.str_tab[k].cm : 0u, cv = str ? (uint32_t)P.str_tab[k].cv : 0u;
    const uint32_t zm = str ? (uint32_t)P.str_tab[k].zm ^ (P.rot ? xm : 0u) : 0u;
    double v[2] = {0, 0};
    for (uint32_t x = threadIdx.x; x < (uint32_t)dim; x += 256u) {
      if ((x & cm) != cv) continue;
      const double ar = re[(size_t)x * es], ai = im[(size_t)x * es];
      double zr = ar * ar + ai * ai, zi = 0.0;
      if (xm) {
        const uint32_t y = x ^ xm;
        const double br = re[(size_t)y * es], bi = im[(size_t)y * es];
        zr = ar * br + ai * bi, zi = ar * bi - ai * br;  // conj(a) b
      }
      const bool neg = __popc(x & zm) & 1;
      v[0] += neg ? -zr : zr;
      v[1] += neg ? -zi : zi;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) wave_sum(v[c]);
    if ((threadIdx.x & 63) == 0) red[w][0] = v[0], red[w][1] = v[1];
    __syncthreads();
    if (threadIdx.x == 0) {
      const double sr = red[0][0] + red[1][0] + red[2][0] + red[3][0];
      const double si = red[0][1] + red[1][1] + red[2][1] + red[3][1];
      if (str) {
        double pr = P.str_tab[k].pre_re, pi = P.str_tab[k].pre_im;
        if (P.rot)  // times (-i)^popcount(xm)
          for (int q = __popc(xm) & 3; q > 0; --q) {
            const double t = pr;
            pr = pi, pi = -t;
          }
        o[2 * k] = pr * sr - pi * si;
        o[2 * k + 1] = pr * si + pi * sr;
      } else {
        o[S - 2] = sr;
      }
    }
    __syncthreads();
  }
  for (int i = 2 * K + threadIdx.x; i < S; i += 256)
    if (i != S - 2) o[i] = 0.0;
}

}  // namespace

hipError_t launch_obs_strings(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                              double* partial, int S, hipStream_t st, int n_out, size_t out_stride, int xq) {
  if (n_items <= 0 || n_out <= 0) return hipSuccess;
  if ((n_out > 1 && bsel >= 3) || S < 4 || S > string_stride(kMaxOpStrings)) return hipErrorInvalidValue;
  return for_tile_bits(L, [&](auto l) {
    hipLaunchKernelGGL((k_obs_strings<l()>), dim3(n_items, n_out), dim3(Geo<l()>::NT), 0, st, probs, items, bsel,
                       partial, out_stride, xq, S);
    return hipGetLastError();
  });
}

hipError_t launch_dense_obs_strings(const DenseProb* d, int count, int dim, const DenseCols& cols, int tb, int t0,
                                    int S, hipStream_t st) {
  hipLaunchKernelGGL(k_dense_obs_strings, dim3(tb, count), dim3(256), 0, st, d, dim, cols.Psi, cols.pstride,
                     cols.colstride, cols.imoff, cols.es, t0, S);
  return hipGetLastError();
}

}  // namespace dse
