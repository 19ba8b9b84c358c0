// dse_rt_small.hip -- host side of the small-register engine (dse_small.hip).
#include "dse_ctx.h"

namespace dse::rt {

// ---- small-register engine (dse_small.hip) ------------------------------------------------
// Problems with P.sm: Chebyshev coefficients per distinct interval length (one output per series),
// descriptors, then every launch of the whole evolve is enqueued on the engine's own stream
// (ceil((n_t - 1) / small_chunk) per register size); small_gather waits for them and fills obs_out.
int small_launch(dse_ctx* ctx, const double* t, int n_t, double tol, double* h_applications,
                 double* launches) {
  std::vector<int> sm;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi)
    if (ctx->probs[pi].sm) sm.push_back((int)pi);
  *h_applications = 0.0;
  *launches = 0.0;
  if (sm.empty()) return DSE_OK;
  if (!ctx->small_stream) HIPC(hipStreamCreateWithFlags(&ctx->small_stream, hipStreamNonBlocking));
  // distinct interval lengths -> sets
  std::vector<double> taus;
  std::vector<int> iv_set(std::max(n_t - 1, 1), 0);
  std::map<double, int> tau_id;
  for (int m = 0; m + 1 < n_t; ++m) {
    const double tau = t[m + 1] - t[m];
    auto it = tau_id.find(tau);
    if (it == tau_id.end()) {
      if (taus.size() >= 4096) return fail(ctx, DSE_ERR_ARG, "more than 4096 distinct output intervals");
      it = tau_id.emplace(tau, (int)taus.size()).first;
      taus.push_back(tau);
    }
    iv_set[m] = it->second;
  }
  if (taus.empty()) taus.push_back(0.0);
  const int n_sets = (int)taus.size();
  std::vector<SmallProb> desc(ctx->probs.size());
  std::memset(desc.data(), 0, desc.size() * sizeof(SmallProb));
  Arena arena;  // every problem's coefficients and degrees, one upload
  std::vector<std::pair<size_t, size_t>> aoff(ctx->probs.size());
  for (int pi : sm) {
    HostProblem& P = ctx->probs[pi];
    const double alpha = std::max(0.5 * (P.e_max - P.e_min), 1e-300);
    const double beta = 0.5 * (P.e_max + P.e_min);
    std::vector<std::vector<std::pair<double, double>>> series(n_sets);
    std::vector<int> deg(n_sets, 1);
    int kcap = 1;
    for (int sidx = 0; sidx < n_sets; ++sidx) {
      int kmax = 0;
      const int rc = cheb_series(alpha, beta, taus[sidx], tol, ctx->max_degree, &deg[sidx], &series[sidx], &kmax);
      if (rc == DSE_ERR_CONVERGENCE)
        return fail(ctx, DSE_ERR_CONVERGENCE, "Chebyshev degree " + std::to_string(kmax) +
                                                  " exceeds max_degree; use a finer output grid");
      if (rc != DSE_OK) return fail(ctx, DSE_ERR_ARG, "bessel failed");
      kcap = std::max(kcap, deg[sidx]);
    }
    for (int m = 0; m + 1 < n_t; ++m) *h_applications += deg[iv_set[m]];
    const int kcap1 = kcap + 1;
    std::vector<double2> a((size_t)n_sets * kcap1, make_double2(0.0, 0.0));
    for (int sidx = 0; sidx < n_sets; ++sidx)
      for (int k = 0; k <= deg[sidx]; ++k)
        a[(size_t)sidx * kcap1 + k] = make_double2(series[sidx][k].first, series[sidx][k].second);
    aoff[pi].first = arena.add(a.data(), a.size() * sizeof(double2));
    aoff[pi].second = arena.add(deg.data(), deg.size() * sizeof(int));
    P.degree = kcap;
    const DevProb& d = ctx->h_desc[pi];
    SmallProb& q = desc[pi];
    q.state = P.buf[0];
    q.field = d.field;
    q.zz = d.zz;
    q.pair = nullptr;
    q.flip = nullptr;
    q.sea_mask = P.sea_mask;
    q.shift = P.shift;
    q.beta = beta;
    q.s1 = 1.0 / alpha;
    q.n = P.n;
    q.rare_bit = P.rare_bit;
    q.kcap1 = kcap1;
    q.n_t = n_t;
    q.ovl_refs = P.d_ovl_tab;
    q.ovl_k = P.ovl_k();
    q.str_tab = P.d_str_tab;
    q.str_k = P.str_k();
    q.sec_tab = P.d_sec_tab;
    q.sec_k = P.sec_k();
    P.final_bsel = 0;
  }
  {
    int rc = upload_arena(ctx, arena, ctx->d_sm_coef, ctx->small_stream);
    if (rc) return rc;
  }
  for (int pi : sm) {
    HostProblem& P = ctx->probs[pi];
    P.sm_coef = reinterpret_cast<double2*>(ctx->d_sm_coef.p + aoff[pi].first);
    P.sm_deg = reinterpret_cast<int*>(ctx->d_sm_coef.p + aoff[pi].second);
    desc[pi].coef = P.sm_coef;
    desc[pi].deg = P.sm_deg;
  }
  // pair / flip tables: the problem's full n x n and 4n arrays (the device tables hold field, zz)
  size_t extra = 0;
  for (int pi : sm) extra += (size_t)ctx->probs[pi].n * ctx->probs[pi].n + 4 * (size_t)ctx->probs[pi].n;
  // aux ints: per register size the selection of problems, then the interval -> set map
  const size_t aux = ctx->probs.size() + (size_t)std::max(n_t - 1, 1) + 2 * extra + 64;
  if (int rc = ctx->d_small_aux.reserve(ctx, aux, "small-engine allocation failed")) return rc;
  // tables after the ints (8-byte aligned)
  double* tab = reinterpret_cast<double*>(ctx->d_small_aux.p + ((ctx->probs.size() + std::max(n_t - 1, 1) + 1) & ~size_t(1)));
  {
    std::vector<double> ht;
    ht.reserve(extra);
    std::vector<size_t> off(ctx->probs.size(), 0);
    for (int pi : sm) {
      const HostProblem& P = ctx->probs[pi];
      off[pi] = ht.size();
      ht.insert(ht.end(), P.pair.begin(), P.pair.end());
      // drives as the engine's kernels see them (cos(pi/2) residue dropped, build_tables)
      for (int b = 0; b < P.n; ++b)
        for (int c = 0; c < 4; c += 2) {
          double re = P.flip[4 * b + c], im = P.flip[4 * b + c + 1];
          if (std::fabs(re) <= 1e-15 * std::hypot(re, im)) re = 0.0;
          ht.push_back(re);
          ht.push_back(im);
        }
    }
    if (!ht.empty()) HIPC(hipMemcpy(tab, ht.data(), ht.size() * sizeof(double), hipMemcpyHostToDevice));
    for (int pi : sm) {
      desc[pi].pair = tab + off[pi];
      desc[pi].flip = tab + off[pi] + (size_t)ctx->probs[pi].n * ctx->probs[pi].n;
    }
  }
  if (int rc = ctx->d_small.reserve(ctx, desc.size(), "small-engine allocation failed")) return rc;
  HIPC(hipMemcpy(ctx->d_small.p, desc.data(), desc.size() * sizeof(SmallProb), hipMemcpyHostToDevice));
  double* d_fam[kNumObsFamilies] = {};  // the enabled families' outputs
  for (ObsFamily f : kObsLaunchOrder) {
    if (!ctx->fam[f].on) continue;
    const size_t sn = ctx->probs.size() * (size_t)n_t * kObsFamilies[f].small_stride;
    const std::string what = std::string("small-engine ") + kObsFamilies[f].noun + " output allocation failed";
    if (int rc = ctx->fam[f].d_small.reserve(ctx, sn, what.c_str())) return rc;
    d_fam[f] = ctx->fam[f].d_small.p;
  }
  // the string kernels (k_small_str, k_small_obs0_str) only when a small register of this call holds strings
  bool sm_strings = false;
  for (int pi : sm) sm_strings = sm_strings || ctx->probs[pi].str_k() > 0;
  double* d_str = sm_strings ? d_fam[kString] : nullptr;
  // the sector kernels (k_small_sec, k_small_obs0_sec) only when a small register of this call holds sets
  bool sm_sectors = false;
  for (int pi : sm) sm_sectors = sm_sectors || ctx->probs[pi].sec_k() > 0;
  double* d_sec = sm_sectors ? d_fam[kSector] : nullptr;
  const size_t outn = ctx->probs.size() * (size_t)n_t * 8;
  if (int rc = ctx->d_small_out.reserve(ctx, outn, "small-engine output allocation failed")) return rc;
  // selections per register size, then the interval -> set map
  std::vector<int> ints;
  std::vector<std::pair<int, std::pair<int, int>>> groups;  // n -> (offset, count)
  for (int n = 1; n <= kSmallMaxQubits; ++n) {
    const int o = (int)ints.size();
    for (int pi : sm)
      if (ctx->probs[pi].n == n) ints.push_back(pi);
    if ((int)ints.size() > o) groups.push_back({n, {o, (int)ints.size() - o}});
  }
  const int iv_off = (int)ints.size();
  ints.insert(ints.end(), iv_set.begin(), iv_set.end());
  HIPC(hipMemcpy(ctx->d_small_aux.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
  hipStream_t st = ctx->small_stream;
  for (const auto& g : groups)
    HIPC(launch_small_obs0(g.first, ctx->d_small.p, ctx->d_small_aux.p + g.second.first, g.second.second,
                           ctx->d_small_out.p, st, d_fam[kSite], d_fam[kPair], d_fam[kOverlap], d_str, d_sec));
  const int chunk = std::max(1, ctx->small_chunk);
  for (int m0 = 0; m0 + 1 < n_t; m0 += chunk) {
    const int cnt = std::min(chunk, n_t - 1 - m0);
    for (const auto& g : groups) {
      HIPC(launch_small(g.first, ctx->d_small.p, ctx->d_small_aux.p + g.second.first, g.second.second, m0,
                        cnt, ctx->d_small_aux.p + iv_off, ctx->d_small_out.p, st, d_fam[kSite], d_fam[kPair],
                        d_fam[kOverlap], d_str, d_sec));
      *launches += 1.0;
    }
  }
  return DSE_OK;
}

int small_gather(dse_ctx* ctx, int n_t, double* obs_out) {
  bool any = false;
  for (auto& P : ctx->probs) any = any || P.sm;
  if (!any) return DSE_OK;
  HIPC(hipStreamSynchronize(ctx->small_stream));
  std::vector<double> h(ctx->probs.size() * (size_t)n_t * 8);
  HIPC(hipMemcpy(h.data(), ctx->d_small_out.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    if (!P.sm) continue;
    for (int ti = 0; ti < n_t; ++ti)
      finish_obs(P, h.data() + (pi * (size_t)n_t + ti) * 8, obs_out + pi * DSE_N_OBS * (size_t)n_t + ti,
                 (size_t)n_t);
  }
  for (ObsFamily f : kObsReadbackOrder) {
    if (!ctx->fam[f].on) continue;
    const size_t S = (size_t)kObsFamilies[f].small_stride;
    std::vector<double> hf(ctx->probs.size() * (size_t)n_t * S);
    HIPC(hipMemcpy(hf.data(), ctx->fam[f].d_small.p, hf.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t pi = 0; pi < ctx->probs.size(); ++pi)
      if (ctx->probs[pi].sm) finish_family_outputs(ctx, f, pi, hf.data() + pi * (size_t)n_t * S, S, n_t);
  }
  return DSE_OK;
}

}  // namespace dse::rt
