// dse_small_kernels.inc -- the two kernels of the small-register engine, included by dse_small.hip
// once per form: DSE_SMALL_OVL 0, k_small / k_small_obs0 (the text below is then exactly what it was
// before the overlaps existed, so those instances keep their code), DSE_SMALL_OVL 1, k_small_ovl /
// k_small_obs0_ovl with one more output pointer, and DSE_SMALL_OVL 2, k_small_str / k_small_obs0_str
// with two more, the overlaps' and the operator strings', each optional at run time (null: skipped),
// and DSE_SMALL_OVL 3, k_small_sec / k_small_obs0_sec with a third, the sector populations', optional
// in the same way.
// A device function holding the body, called from two kernels, is not equivalent: inlined, the
// existing instances came out with other register counts.
#if DSE_SMALL_OVL == 3
#define DSE_SMALL_NAME(k) k##_sec
#define DSE_SMALL_OVL_PARAM , double* __restrict__ ovl, double* __restrict__ strs, double* __restrict__ secs
#elif DSE_SMALL_OVL == 2
#define DSE_SMALL_NAME(k) k##_str
#define DSE_SMALL_OVL_PARAM , double* __restrict__ ovl, double* __restrict__ strs
#elif DSE_SMALL_OVL
#define DSE_SMALL_NAME(k) k##_ovl
#define DSE_SMALL_OVL_PARAM , double* __restrict__ ovl
#else
#define DSE_SMALL_NAME(k) k
#define DSE_SMALL_OVL_PARAM
#endif

// SITES: also the site-resolved sums of every output into sites[problem][m][kSmallSiteStride]
// (the 7 aggregate sums keep their code and order); PAIRS: after them the two-spin sums into
// pairs[problem][m][kSmallPairStride]; DSE_SMALL_OVL: after those the overlaps with the problem's
// reference states into ovl[problem][m][kSmallOverlapStride] (those instances take the PAIRS form of
// the prologue)
template <int N, bool SITES, bool PAIRS>
__global__ void __launch_bounds__(64)
DSE_SMALL_NAME(k_small)(const SmallProb* __restrict__ probs, const int* __restrict__ sel, int m0, int n_int,
                        const int* __restrict__ iv_set, double* __restrict__ out, double* __restrict__ sites,
                        double* __restrict__ pairs DSE_SMALL_OVL_PARAM) {
  using G = SmallGeo<N>;
  constexpr int R = G::R, DIM = G::DIM, NP = G::NP;
  __shared__ double2 w[DIM];
  __shared__ double2 fl[N][2];  // drive coefficient of bit b for output bit value v
  __shared__ double pg[NP > 0 ? NP : 1];
  __shared__ int pm[NP > 0 ? NP : 1];   // pair masks e_i | e_j
  __shared__ double red[8];

  const SmallProb& P = probs[sel[blockIdx.x]];
  const int lane = threadIdx.x;
  const bool live = lane < DIM;
  const gd2* gst_ = gptr((const double2*)P.state);

  // tables -> LDS; the diagonal D(x) - beta of the owned amplitudes -> registers
  if (lane < N) {
    fl[lane][0] = make_double2(P.flip[4 * lane + 0], P.flip[4 * lane + 1]);
    fl[lane][1] = make_double2(P.flip[4 * lane + 2], P.flip[4 * lane + 3]);
  }
  for (int e = lane; e < NP; e += 64) {
    int i = 0, rem = e;
    while (rem >= N - 1 - i) rem -= N - 1 - i, ++i;
    pg[e] = P.pair[i * N + i + 1 + rem];
    pm[e] = (1 << i) | (1 << (i + 1 + rem));
  }
  double dmb[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int x = r * 64 + lane;
    double d = P.shift - P.beta;
    for (int b = 0; b < N; ++b) {
      const double sb = 0.5 - (double)((x >> b) & 1);
      d += P.field[b] * sb;
      for (int c = b + 1; c < N; ++c) d += P.zz[b * N + c] * (sb * (0.5 - (double)((x >> c) & 1)));
    }
    dmb[r] = d;
    if (!PAIRS && !DSE_SMALL_OVL && live) w[x] = gld(gst_, x);  // (the instances without pair sums: their code as it was)
  }
  if (PAIRS || DSE_SMALL_OVL) {
    // The state in a loop of its own.  Stored to LDS inside the loop above, each store might alias the
    // coefficient tables read through generic pointers, so all R x N (N + 1) / 2 loads are issued again
    // per row: at N = 9 that prologue spilled (246 VGPRs, 988 B of scratch per lane).
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live) w[r * 64 + lane] = gld(gst_, r * 64 + lane);
  }
  __syncthreads();

  const double s1 = P.s1, inv2s1 = 0.5 / s1;
  for (int mi = 0; mi < n_int; ++mi) {
    const int m = m0 + mi;  // interval [t_m, t_{m+1}]
    const int set = iv_set[m];
    const cptr<double> a = (cptr<double>)(P.coef + (size_t)set * P.kcap1);  // a_k = (a[2k], a[2k+1])
    const int K = P.deg[set];
    double2 o[R], acc[R];
    {
      const double2 a0 = make_double2(a[0], a[1]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const double2 v = live ? w[r * 64 + lane] : make_double2(0.0, 0.0);
        acc[r] = cmad(make_double2(0.0, 0.0), a0.x, a0.y, v);
        o[r] = make_double2(0.0, 0.0);
      }
    }
    for (int k = 1; k <= K; ++k) {
      double2 own[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int x = r * 64 + lane;
        own[r] = live ? w[x] : make_double2(0.0, 0.0);
        o[r].x = fma(dmb[r], own[r].x, o[r].x);
        o[r].y = fma(dmb[r], own[r].y, o[r].y);
      }
#pragma unroll
      for (int b = 0; b < N; ++b) {
        const double2 c0 = fl[b][0], c1 = fl[b][1];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int x = r * 64 + lane;
          if (!live) continue;
          const double2 c = ((x >> b) & 1) ? c1 : c0;
          o[r] = cmad(o[r], c.x, c.y, w[x ^ (1 << b)]);
        }
      }
      if (N <= 7) {  // every pair's mask at compile time
        int e = 0;
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
          for (int j = i + 1; j < N; ++j, ++e) {
            const double g = pg[e];
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const int x = r * 64 + lane;
              if (!live || (((x >> i) ^ (x >> j)) & 1)) continue;
              const double2 v = w[x ^ ((1 << i) | (1 << j))];
              o[r].x = fma(g, v.x, o[r].x);
              o[r].y = fma(g, v.y, o[r].y);
            }
          }
      } else {  // 28 / 36 pairs: a loop (an unrolled one hoists every coefficient into registers)
#pragma unroll 1
        for (int e = 0; e < NP; ++e) {
          const double g = pg[e];
          const int m = pm[e];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int x = r * 64 + lane;
            if (!live || (__popc(x & m) & 1)) continue;
            const double2 v = w[x ^ m];
            o[r].x = fma(g, v.x, o[r].x);
            o[r].y = fma(g, v.y, o[r].y);
          }
        }
      }
      const double sc = (k == 1) ? s1 : 2.0 * s1;
      const double2 ak = make_double2(a[2 * k], a[2 * k + 1]);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        o[r].x *= sc;
        o[r].y *= sc;
        acc[r] = cmad(acc[r], ak.x, ak.y, o[r]);
      }
      __syncthreads();  // all reads of w_{k-1} done
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int x = r * 64 + lane;
        if (live) w[x] = o[r];
        o[r] = make_double2(-inv2s1 * own[r].x, -inv2s1 * own[r].y);  // the next term's -w_{k-2}/(2 s1)
      }
      __syncthreads();
    }
    // psi(t_{m+1}) = acc -> LDS (w_0 of the next interval), then its observables
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live) w[r * 64 + lane] = acc[r];
    __syncthreads();
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    if (live) {
      const double half_sea = 0.5 * (double)__popcll(P.sea_mask);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int x = r * 64 + lane;
        const double2 p = acc[r];
        const double p2 = p.x * p.x + p.y * p.y;
        v[6] += p2;
        v[2] += p2 * (half_sea - (double)__popcll((uint64_t)x & P.sea_mask));
        if (P.rare_bit >= 0) v[3] += p2 * (0.5 - (double)((x >> P.rare_bit) & 1));
#pragma unroll
        for (int b = 0; b < N; ++b) {
          const bool sea = (P.sea_mask >> b) & 1ull, rr = (b == P.rare_bit);
          if ((!sea && !rr) || ((x >> b) & 1)) continue;
          const double2 s = w[x ^ (1 << b)];
          const double re = p.x * s.x + p.y * s.y, im = p.x * s.y - p.y * s.x;
          if (sea) v[0] += re, v[1] += im;
          if (rr) v[4] += re, v[5] += im;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      double t = v[j];
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
      if (lane == 0) red[j] = t;
    }
    __syncthreads();
    if (lane < 8) out[((size_t)sel[blockIdx.x] * P.n_t + (m + 1)) * 8 + lane] = lane < 7 ? red[lane] : 0.0;
    if (SITES)
      small_site_sums<N>(w, lane, live, sites + ((size_t)sel[blockIdx.x] * P.n_t + (m + 1)) * kSmallSiteStride);
    if (PAIRS)
      small_pair_sums<N>(w, lane, live, pairs + ((size_t)sel[blockIdx.x] * P.n_t + (m + 1)) * kSmallPairStride);
#if DSE_SMALL_OVL >= 2
    if (ovl)
      small_overlap_sums<N>(w, lane, live, P.ovl_refs, P.ovl_k,
                            ovl + ((size_t)sel[blockIdx.x] * P.n_t + (m + 1)) * kSmallOverlapStride);
    if (strs)
      small_string_sums<N>(w, lane, live, P.str_tab, P.str_k,
                           strs + ((size_t)sel[blockIdx.x] * P.n_t + (m + 1)) * kSmallStringStride);
#if DSE_SMALL_OVL == 3
    if (secs)
      small_sector_sums<N>(w, lane, live, P.sec_tab, P.sec_k,
                           secs + ((size_t)sel[blockIdx.x] * P.n_t + (m + 1)) * kSmallSectorStride);
#endif
#elif DSE_SMALL_OVL
    small_overlap_sums<N>(w, lane, live, P.ovl_refs, P.ovl_k,
                          ovl + ((size_t)sel[blockIdx.x] * P.n_t + (m + 1)) * kSmallOverlapStride);
#endif
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (live) gst(gptr((double2*)P.state), r * 64 + lane, w[r * 64 + lane]);
}

// observables of the initial state (output 0)
template <int N, bool SITES, bool PAIRS>
__global__ void __launch_bounds__(64)
DSE_SMALL_NAME(k_small_obs0)(const SmallProb* __restrict__ probs, const int* __restrict__ sel,
                             double* __restrict__ out, double* __restrict__ sites,
                             double* __restrict__ pairs DSE_SMALL_OVL_PARAM) {
  using G = SmallGeo<N>;
  constexpr int R = G::R, DIM = G::DIM;
  __shared__ double2 w[DIM];
  const SmallProb& P = probs[sel[blockIdx.x]];
  const int lane = threadIdx.x;
  const bool live = lane < DIM;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (live) w[r * 64 + lane] = gld(gptr((const double2*)P.state), r * 64 + lane);
  __syncthreads();
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const double half_sea = 0.5 * (double)__popcll(P.sea_mask);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int x = r * 64 + lane;
      const double2 p = w[x];
      const double p2 = p.x * p.x + p.y * p.y;
      v[6] += p2;
      v[2] += p2 * (half_sea - (double)__popcll((uint64_t)x & P.sea_mask));
      if (P.rare_bit >= 0) v[3] += p2 * (0.5 - (double)((x >> P.rare_bit) & 1));
      for (int b = 0; b < N; ++b) {
        const bool sea = (P.sea_mask >> b) & 1ull, rr = (b == P.rare_bit);
        if ((!sea && !rr) || ((x >> b) & 1)) continue;
        const double2 s = w[x ^ (1 << b)];
        const double re = p.x * s.x + p.y * s.y, im = p.x * s.y - p.y * s.x;
        if (sea) v[0] += re, v[1] += im;
        if (rr) v[4] += re, v[5] += im;
      }
    }
  }
  for (int j = 0; j < 7; ++j) {
    double t = v[j];
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
    v[j] = t;
  }
  if (lane == 0) {
    double* o = out + (size_t)sel[blockIdx.x] * P.n_t * 8;
    for (int j = 0; j < 7; ++j) o[j] = v[j];
    o[7] = 0.0;
  }
  if (SITES) small_site_sums<N>(w, lane, live, sites + (size_t)sel[blockIdx.x] * P.n_t * kSmallSiteStride);
  if (PAIRS) small_pair_sums<N>(w, lane, live, pairs + (size_t)sel[blockIdx.x] * P.n_t * kSmallPairStride);
#if DSE_SMALL_OVL >= 2
  if (ovl)
    small_overlap_sums<N>(w, lane, live, P.ovl_refs, P.ovl_k, ovl + (size_t)sel[blockIdx.x] * P.n_t * kSmallOverlapStride);
  if (strs)
    small_string_sums<N>(w, lane, live, P.str_tab, P.str_k, strs + (size_t)sel[blockIdx.x] * P.n_t * kSmallStringStride);
#if DSE_SMALL_OVL == 3
  if (secs)
    small_sector_sums<N>(w, lane, live, P.sec_tab, P.sec_k, secs + (size_t)sel[blockIdx.x] * P.n_t * kSmallSectorStride);
#endif
#elif DSE_SMALL_OVL
  small_overlap_sums<N>(w, lane, live, P.ovl_refs, P.ovl_k, ovl + (size_t)sel[blockIdx.x] * P.n_t * kSmallOverlapStride);
#endif
}

#undef DSE_SMALL_NAME
#undef DSE_SMALL_OVL_PARAM
