// dse_runtime.hip -- host runtime behind the C ABI of include/dse.h.
//
// Replaces qt.sesolve (dipolar_ensemble_with_rare.py:653-666) for many independent evolutions
// per device.  Per output interval [t_m, t_{m+1}] every problem runs
//     k = 1 (MODE_FIRST), k = 2..K_p (MODE_GEN), observables of the new state
// on one of several HIP streams ("lanes").  Problems are independent, so lanes never
// synchronise with each other until observable partials are copied back; the GPU overlaps
// the tail of one lane's launch with the next launches of the others.  Within a lane,
// items (problem, tile) are sorted by Chebyshev degree so the items still active at term k are
// a prefix of the lane's item list.
//
// HBM layout per problem: three 2^n double2 state buffers B0, B1, B2.  In interval m (parity q):
//   psi = B[q ? 2 : 0], acc = B[q ? 0 : 2], scratch = B1;  w_j lives in (j odd ? scratch : psi)
// and MODE_GEN overwrites w_{k-2} in place with w_k.  At the end of the interval acc holds
// psi(t_{m+1}) and becomes psi of the next interval.
//
// The small-register engine has a source of its own (dse_rt_small.hip); dse_ctx.h is what the runtime's
// sources share.
#include <unistd.h>

#include <rocsolver/rocsolver.h>

#include "dse_ctx.h"

using namespace dse;
using namespace dse::rt;

namespace {

thread_local std::string g_create_err;

// Host worker threads kept for the process (created on first use, never joined: they only wait
// on a condition variable between jobs), so a dse_evolve does not pay ~16 thread creations per
// parallel section.  One job at a time; a caller that finds the pool busy (another context on
// another host thread) runs its job on threads of its own instead.
class HostPool {
 public:
  static HostPool& get() {
    static HostPool* p = new HostPool();  // intentionally never destroyed (detached workers)
    return *p;
  }
  size_t size() const { return workers_; }
  // body(w) for w < nb, on the pool and the calling thread; false if the pool was busy
  bool run(size_t nb, const std::function<void(size_t)>& body) {
    if (getpid() != pid_) return false;  // a forked child has none of the workers
    std::unique_lock<std::mutex> busy(busy_, std::try_to_lock);
    if (!busy.owns_lock()) return false;
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = &body;
      nb_ = nb;
      next_.store(0);
      active_ = workers_;
      ++gen_;
    }
    cv_.notify_all();
    drain();
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [&] { return active_ == 0; });
    job_ = nullptr;
    return true;
  }

 private:
  HostPool() : workers_(std::min<size_t>(15, std::max(1u, std::thread::hardware_concurrency()) - 1)), pid_(getpid()) {
    for (size_t w = 0; w < workers_; ++w) std::thread([this] { loop(); }).detach();
  }
  void drain() {
    for (size_t b = next_++; b < nb_; b = next_++) (*job_)(b);
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
      }
      drain();
      std::lock_guard<std::mutex> lk(m_);
      if (--active_ == 0) done_.notify_all();
    }
  }
  const size_t workers_;
  const pid_t pid_;
  std::mutex busy_, m_;
  std::condition_variable cv_, done_;
  const std::function<void(size_t)>* job_ = nullptr;
  size_t nb_ = 0, active_ = 0;
  uint64_t gen_ = 0;
  std::atomic<size_t> next_{0};
};

// f(i) for i < n on up to 16 host threads (contiguous blocks; f must touch only item i's data).
template <class F>
void parallel_for(size_t n, F&& f) {
  const size_t nth = std::min<size_t>({(size_t)std::max(1u, std::thread::hardware_concurrency()), 16, (n + 7) / 8});
  if (nth <= 1) {
    for (size_t i = 0; i < n; ++i) f(i);
    return;
  }
  const std::function<void(size_t)> block = [&](size_t w) {
    for (size_t i = n * w / nth; i < n * (w + 1) / nth; ++i) f(i);
  };
  if (HostPool::get().run(nth, block)) return;
  std::vector<std::thread> th;
  th.reserve(nth);
  for (size_t w = 0; w < nth; ++w) th.emplace_back(block, w);
  for (auto& x : th) x.join();
}

}  // namespace

namespace dse::rt {
// The arena's device copy: grows dev to fit, then one copy on stream st (stream-ordered before
// every later launch on st; the caller synchronises st before other streams use it).
int upload_arena(dse_ctx* ctx, const Arena& a, DevBuf<unsigned char>& dev, hipStream_t st) {
  if (a.host.empty()) return DSE_OK;
  if (int rc = dev.reserve(ctx, a.host.size(), "coefficient allocation failed", true)) return rc;
  HIPC(hipMemcpyAsync(dev.p, a.host.data(), a.host.size(), hipMemcpyHostToDevice, st));
  HIPC(hipStreamSynchronize(st));  // the host bytes may be released after return
  return DSE_OK;
}
}  // namespace dse::rt

namespace {

void free_wht(HostProblem& p) {
  for (auto& b : p.wvec)
    if (b) (void)hipFree(b), b = nullptr;
  if (p.d_cquad) (void)hipFree(p.d_cquad), p.d_cquad = nullptr;
  if (p.d_wtab) (void)hipFree(p.d_wtab), p.d_wtab = nullptr;
  p.wht_groups = 0;
}

void free_initial(HostProblem& p) {
  if (p.init_state) (void)hipFree(p.init_state), p.init_state = nullptr;
  if (p.d_init_amp) (void)hipFree(p.d_init_amp), p.d_init_amp = nullptr;
  p.init_amp.clear();
  p.init_kind = 0;
}

void free_overlap_refs(HostProblem& p) {
  for (double2* r : p.ovl_refs) (void)hipFree(r);
  p.ovl_refs.clear();
  if (p.d_ovl_tab) (void)hipFree(p.d_ovl_tab), p.d_ovl_tab = nullptr;
}

void free_op_strings(HostProblem& p) {
  p.str_tab.clear();
  if (p.d_str_tab) (void)hipFree(p.d_str_tab), p.d_str_tab = nullptr;
}

void free_sectors(HostProblem& p) {
  p.sec_tab.clear();
  if (p.d_sec_tab) (void)hipFree(p.d_sec_tab), p.d_sec_tab = nullptr;
}

void free_device(dse_ctx* ctx) {
  for (auto& p : ctx->probs) {
    for (auto& b : p.buf)
      if (b) (void)hipFree(b), b = nullptr;
    if (p.tables) (void)hipFree(p.tables), p.tables = nullptr;
    p.coef = nullptr;
    if (p.d_items) (void)hipFree(p.d_items), p.d_items = nullptr;
    for (auto& b : p.rbuf_own)
      if (b) (void)hipFree(b), b = nullptr;
    p.sm_coef = nullptr;
    p.sm_deg = nullptr;
    free_wht(p);
  }
  if (ctx->d_wht) (void)hipFree(ctx->d_wht), ctx->d_wht = nullptr;
  ctx->wht_ready = false;
  if (ctx->d_probs) (void)hipFree(ctx->d_probs), ctx->d_probs = nullptr;
  if (ctx->d_items) (void)hipFree(ctx->d_items), ctx->d_items = nullptr;
  if (ctx->d_items_iv) (void)hipFree(ctx->d_items_iv), ctx->d_items_iv = nullptr;
  for (auto& A : ctx->fam) A.release();
  release_all(ctx->d_partial, ctx->d_flags, ctx->d_xslots, ctx->d_xacc, ctx->d_real,
              ctx->d_real_tab, ctx->d_real_items, ctx->d_span, ctx->d_span_tab, ctx->d_span_slots, ctx->d_span_flags,
              ctx->d_span_items, ctx->d_coef, ctx->d_sm_coef, ctx->d_init, ctx->d_small, ctx->d_small_out,
              ctx->d_small_aux, ctx->d_allreduce);
  for (auto& kv : ctx->zzlo_tables) (void)hipFree(kv.second);
  ctx->zzlo_tables.clear();
  ctx->partial_slots = 0;
  ctx->total_items = 0;
  ctx->prepared = false;
  ctx->evolved = false;
}

void destroy_lanes(dse_ctx* ctx) {
  if (ctx->swap_stream) {
    (void)hipStreamSynchronize(ctx->swap_stream);
    for (auto& e : ctx->swap_ev)
      if (e) (void)hipEventDestroy(e), e = nullptr;
    (void)hipStreamDestroy(ctx->swap_stream);
    ctx->swap_stream = nullptr;
  }
  if (ctx->small_stream) {
    (void)hipStreamSynchronize(ctx->small_stream);
    (void)hipStreamDestroy(ctx->small_stream);
    ctx->small_stream = nullptr;
  }
  if (ctx->blas) (void)rocblas_destroy_handle(ctx->blas), ctx->blas = nullptr;
  for (auto& h : ctx->eig_h) (void)rocblas_destroy_handle(h);
  ctx->eig_h.clear();
  for (auto& e : ctx->eig_st) (void)hipStreamSynchronize(e), (void)hipStreamDestroy(e);
  ctx->eig_st.clear();
  for (auto e : ctx->xev) (void)hipEventDestroy(e);
  ctx->xev.clear();
  ctx->xev_used = 0;
  if (ctx->dense_stream) {
    (void)hipStreamSynchronize(ctx->dense_stream);
    (void)hipStreamDestroy(ctx->dense_stream);
    ctx->dense_stream = nullptr;
  }
  nufft_release(ctx->nufft);
  ctx->nufft = nullptr;
  for (auto& ln : ctx->lanes) {
    if (ln.stream) (void)hipStreamSynchronize(ln.stream);
    if (ln.obs_stream) (void)hipStreamSynchronize(ln.obs_stream);
    for (auto& pool : ln.ev)
      for (auto e : pool) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
      if (ln.ev_iv[i]) (void)hipEventDestroy(ln.ev_iv[i]);
      if (ln.ev_obs[i]) (void)hipEventDestroy(ln.ev_obs[i]);
    }
    if (ln.obs_stream) (void)hipStreamDestroy(ln.obs_stream);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
  }
  ctx->lanes.clear();
}

int ensure_lanes(dse_ctx* ctx) {
  if ((int)ctx->lanes.size() == ctx->n_streams) return DSE_OK;
  destroy_lanes(ctx);
  ctx->lanes.resize(ctx->n_streams);
  for (auto& ln : ctx->lanes) {
    HIPC(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
    // lowest priority: the observables take the CUs the next interval launch leaves, not the
    // other way round
    int least = 0, greatest = 0;
    HIPC(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPC(hipStreamCreateWithPriority(&ln.obs_stream, hipStreamNonBlocking, least));
    for (int i = 0; i < 2; ++i) {
      HIPC(hipEventCreateWithFlags(&ln.ev_iv[i], hipEventDisableTiming));
      HIPC(hipEventCreateWithFlags(&ln.ev_obs[i], hipEventDisableTiming));
    }
  }
  return DSE_OK;
}

// the interval / step / observable streams (not the small-register engine's, which small_gather
// waits for): what flush_partials needs before it reads the observable partials
int sync_lanes(dse_ctx* ctx) {
  if (ctx->swap_stream) HIPC(hipStreamSynchronize(ctx->swap_stream));
  for (auto& ln : ctx->lanes) {
    HIPC(hipStreamSynchronize(ln.stream));
    if (ln.obs_stream) HIPC(hipStreamSynchronize(ln.obs_stream));
  }
  return DSE_OK;
}

int sync_all(dse_ctx* ctx) {
  if (ctx->swap_stream) HIPC(hipStreamSynchronize(ctx->swap_stream));
  for (auto& ln : ctx->lanes) {
    HIPC(hipStreamSynchronize(ln.stream));
    if (ln.obs_stream) HIPC(hipStreamSynchronize(ln.obs_stream));
  }
  if (ctx->small_stream) HIPC(hipStreamSynchronize(ctx->small_stream));
  return DSE_OK;
}

// ---- per-problem device tables ------------------------------------------------------------
int build_tables(dse_ctx* ctx, HostProblem& p, DevProb& d) {
  const int n = p.n;
  const int nl = p.n_local;   // qubits held in this context (n unless partitioned)
  int L = std::max(std::min(nl, ctx->tile_bits), std::max(kMinTile, nl - 32));
  // registers for the Walsh-Hadamard engine (whole, more than two 2^13 tiles) take its tile size
  if (ctx->wht && ctx->tile_bits == kMaxTile && nl > kMaxTile + 1)
    L = ctx->wht_tile_bits ? ctx->wht_tile_bits : 13;
  if (L > kMaxTile) return fail(ctx, DSE_ERR_ARG, "problem too large for the tile range");
  p.L = L;
  p.n_tiles = int64_t(1) << (nl - L);
  const size_t T = size_t(1) << L;
  const uint64_t lo_mask = (uint64_t(1) << L) - 1;
  const bool rb = L >= kRegBlockMinTile;
  const int TB = L - kRegBits;

  std::vector<double> zzlo(T, 0.0);
  for (size_t x = 0; x < T; ++x) {
    double acc = 0.0;
    for (int i = 0; i < L; ++i) {
      const double si = 0.5 - (double)((x >> i) & 1);
      for (int j = i + 1; j < L; ++j) acc += p.zz[i * n + j] * (si * (0.5 - (double)((x >> j) & 1)));
    }
    zzlo[x] = acc;
  }
  std::memset(&d, 0, sizeof(d));
  std::vector<DPair> plo, phi, ptt;
  std::vector<DFlip> flo, fhi;
  std::vector<DSweep> sweeps(rb ? TB : 0);
  for (auto& s : sweeps) std::memset(&s, 0, sizeof(s));
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const double g = p.pair[i * n + j];
      if (g == 0.0) continue;
      const uint64_t m = (uint64_t(1) << i) | (uint64_t(1) << j);
      DPair q;
      q.mask_lo = (uint32_t)(m & lo_mask);
      q.tile_xor = (uint32_t)(m >> L);
      q.g = g;
      if (q.tile_xor) {
        phi.push_back(q);
      } else if (!rb) {
        plo.push_back(q);
      } else if (j < TB) {
        ptt.push_back(q);  // both thread bits
      } else if (i >= TB) {
        d.rr_g[rr_index(i - TB, j - TB)] = g;  // both register bits
      } else {
        sweeps[i].g[j - TB] = g;  // thread bit i, register bit j - TB
        sweeps[i].has_pair = 1;
      }
    }
  p.imag = true;
  for (int b = 0; b < n; ++b) {
    // A real part below 1e-15 of the coefficient's modulus is the rounding residue of cos(pi/2)
    // (the reference's drive phase, dipolar_ensemble_with_rare.py:516-530): it is dropped, so
    // drives at phase pi/2 take the imaginary-coefficient kernels (2 FMAs per amplitude, not 4).
    // The dropped entry is 1e-16 of its row's drive term, below the rounding of H itself.
    double f[4];
    for (int c = 0; c < 4; c += 2) {
      f[c] = p.flip[4 * b + c];
      f[c + 1] = p.flip[4 * b + c + 1];
      if (std::fabs(f[c]) <= 1e-15 * std::hypot(f[c], f[c + 1])) f[c] = 0.0;
    }
    if (f[0] == 0.0 && f[1] == 0.0 && f[2] == 0.0 && f[3] == 0.0) continue;
    if (f[0] != 0.0 || f[2] != 0.0) p.imag = false;
    const uint64_t m = uint64_t(1) << b;
    DFlip q;
    q.mask_lo = (uint32_t)(m & lo_mask);
    q.tile_xor = (uint32_t)(m >> L);
    q.re0 = f[0];
    q.im0 = f[1];
    q.re1 = f[2];
    q.im1 = f[3];
    q.pad = 0.0;
    if (q.tile_xor) {
      fhi.push_back(q);
    } else if (!rb) {
      flo.push_back(q);
    } else if (b < TB) {
      DSweep& s = sweeps[b];
      s.re0 = f[0];
      s.im0 = f[1];
      s.re1 = f[2];
      s.im1 = f[3];
      s.has_flip = 1;
    } else {
      const int i = b - TB;
      for (int c = 0; c < 4; ++c) d.rflip[i][c] = f[c];
      d.rflip_mask |= 1 << i;
    }
  }
  const size_t o_field = 0;
  const size_t o_zz = align_up(o_field + n * sizeof(double), 256);
  const size_t o_plo = align_up(o_zz + size_t(n) * n * sizeof(double), 256);
  const size_t o_phi = align_up(o_plo + plo.size() * sizeof(DPair), 256);
  const size_t o_ptt = align_up(o_phi + phi.size() * sizeof(DPair), 256);
  const size_t o_flo = align_up(o_ptt + ptt.size() * sizeof(DPair), 256);
  const size_t o_fhi = align_up(o_flo + flo.size() * sizeof(DFlip), 256);
  const size_t o_sw = align_up(o_fhi + fhi.size() * sizeof(DFlip), 256);
  const size_t total = align_up(o_sw + sweeps.size() * sizeof(DSweep) + 16, 256);
  std::vector<char> blob(total, 0);
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) std::memcpy(blob.data() + off, src, bytes);
  };
  put(o_field, p.field.data(), n * sizeof(double));
  put(o_zz, p.zz.data(), size_t(n) * n * sizeof(double));
  put(o_plo, plo.data(), plo.size() * sizeof(DPair));
  put(o_phi, phi.data(), phi.size() * sizeof(DPair));
  put(o_ptt, ptt.data(), ptt.size() * sizeof(DPair));
  put(o_flo, flo.data(), flo.size() * sizeof(DFlip));
  put(o_fhi, fhi.data(), fhi.size() * sizeof(DFlip));
  put(o_sw, sweeps.data(), sweeps.size() * sizeof(DSweep));
  if (hipMalloc(&p.tables, total) != hipSuccess)
    return fail(ctx, DSE_ERR_OOM, "device allocation of coefficient tables failed");
  HIPC(hipMemcpy(p.tables, blob.data(), total, hipMemcpyHostToDevice));
  const size_t vbytes = (size_t(1) << nl) * sizeof(double2);
  for (auto& b : p.buf) {
    if (hipMalloc(&b, vbytes) != hipSuccess)
      return fail(ctx, DSE_ERR_OOM, "device allocation of state buffers failed (" +
                                        std::to_string(3 * vbytes) + " bytes per problem)");
    HIPC(hipMemset(b, 0, vbytes));
  }
  char* tb = static_cast<char*>(p.tables);
  for (int i = 0; i < 3; ++i) d.buf[i] = p.buf[i];
  auto zt = ctx->zzlo_tables.find(zzlo);
  if (zt == ctx->zzlo_tables.end()) {
    double* dz = nullptr;
    if (hipMalloc(&dz, T * sizeof(double)) != hipSuccess)
      return fail(ctx, DSE_ERR_OOM, "device allocation of the ZZ table failed");
    HIPC(hipMemcpy(dz, zzlo.data(), T * sizeof(double), hipMemcpyHostToDevice));
    zt = ctx->zzlo_tables.emplace(zzlo, dz).first;
  }
  d.zzlo = zt->second;
  d.field = reinterpret_cast<const double*>(tb + o_field);
  d.zz = reinterpret_cast<const double*>(tb + o_zz);
  d.pairs_lo = reinterpret_cast<const DPair*>(tb + o_plo);
  d.pairs_hi = reinterpret_cast<const DPair*>(tb + o_phi);
  d.pairs_tt = reinterpret_cast<const DPair*>(tb + o_ptt);
  d.flips_lo = reinterpret_cast<const DFlip*>(tb + o_flo);
  d.flips_hi = reinterpret_cast<const DFlip*>(tb + o_fhi);
  d.sweeps = reinterpret_cast<const DSweep*>(tb + o_sw);
  d.coef = nullptr;
  d.sea_mask = p.sea_mask;
  d.shift = p.shift;
  d.beta = 0.0;
  d.s1 = 1.0;
  d.n = n;
  d.L = L;
  d.n_pairs_lo = (int)plo.size();
  d.n_pairs_hi = (int)phi.size();
  d.n_pairs_tt = (int)ptt.size();
  d.n_flips_lo = (int)flo.size();
  d.n_flips_hi = (int)fhi.size();
  d.kcap1 = 0;
  d.rare_bit = p.rare_bit;
  d.n_sea = __builtin_popcountll(p.sea_mask);
  // partitioned register: global tile index = rank << tbl | local tile; partner masks
  d.tbl = nl - L;
  d.h_base = (uint32_t)p.shard_rank << d.tbl;
  p.xmasks = 0;
  if (p.shard_bits > 0) {
    for (const auto& q : phi)
      if (q.tile_xor >> d.tbl) p.xmasks |= 1u << (q.tile_xor >> d.tbl);
    for (const auto& q : fhi)
      if (q.tile_xor >> d.tbl) p.xmasks |= 1u << (q.tile_xor >> d.tbl);
    for (int b = nl; b < n; ++b)  // <Ix>, <Iy> of a global qubit pair amplitudes across shards
      if (((p.sea_mask >> b) & 1ull) || b == p.rare_bit) p.xmasks |= 1u << (1u << (b - nl));
  }
  return DSE_OK;
}

int prepare(dse_ctx* ctx) {
  if (ctx->prepared) return DSE_OK;
  if (ctx->probs.empty()) return fail(ctx, DSE_ERR_STATE, "no problems added");
  int rc = ensure_lanes(ctx);
  if (rc) return rc;
  std::vector<DevProb> dp(ctx->probs.size());
  int64_t total = 0;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    if ((rc = build_tables(ctx, ctx->probs[pi], dp[pi]))) {
      free_device(ctx);
      return rc;
    }
    HostProblem& p = ctx->probs[pi];
    std::vector<int2> its(p.n_tiles);
    for (int64_t t = 0; t < p.n_tiles; ++t) its[t] = make_int2((int)pi, (int)t);
    if (hipMalloc(&p.d_items, its.size() * sizeof(int2)) != hipSuccess) {
      free_device(ctx);
      return fail(ctx, DSE_ERR_OOM, "device allocation of item lists failed");
    }
    HIPC(hipMemcpy(p.d_items, its.data(), its.size() * sizeof(int2), hipMemcpyHostToDevice));
    total += p.n_tiles;
  }
  // partitioned registers: partner shards' buffers (same context) or exchange receive buffers
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    HostProblem& p = ctx->probs[pi];
    if (p.shard_bits == 0) continue;
    for (int m = 1; m < (1 << p.shard_bits); ++m) {
      if (!((p.xmasks >> m) & 1u)) continue;
      if (p.dist) {
        const size_t vbytes = (size_t(1) << p.n_local) * sizeof(double2);
        if (hipMalloc(&p.rbuf_own[m], vbytes) != hipSuccess) {
          free_device(ctx);
          return fail(ctx, DSE_ERR_OOM, "device allocation of exchange buffers failed");
        }
        for (int r = 0; r < 3; ++r) dp[pi].rbuf[m][r] = p.rbuf_own[m];
      } else {
        const HostProblem& q = ctx->probs[p.group_first + (p.shard_rank ^ m)];
        for (int r = 0; r < 3; ++r) dp[pi].rbuf[m][r] = q.buf[r];
      }
    }
  }
  if (hipMalloc(&ctx->d_probs, dp.size() * sizeof(DevProb)) != hipSuccess ||
      hipMalloc(&ctx->d_items, total * sizeof(int2)) != hipSuccess ||
      hipMalloc(&ctx->d_items_iv, total * sizeof(int2)) != hipSuccess) {
    free_device(ctx);
    return fail(ctx, DSE_ERR_OOM, "device allocation of descriptors failed");
  }
  HIPC(hipMemcpy(ctx->d_probs, dp.data(), dp.size() * sizeof(DevProb), hipMemcpyHostToDevice));
  ctx->h_desc = dp;
  ctx->total_items = total;
  HIPC(hipDeviceSynchronize());
  ctx->prepared = true;
  return DSE_OK;
}

// ---- Walsh-Hadamard engine ------------------------------------------------------------------

// WhtGroup of the given high bits: completed to wl tile bits by the lowest carried bits; every
// other local bit is an outer bit.
WhtGroup make_group(const std::vector<int>& bits, int wl, int n_local) {
  WhtGroup g;
  std::memset(&g, 0, sizeof(g));
  const int s = (int)bits.size();
  g.c = wl - s;
  std::vector<int> in(n_local, 0);
  for (int q = 0; q < g.c; ++q) g.pos[q] = q, in[q] = 1;
  for (int i = 0; i < s; ++i) g.pos[g.c + i] = bits[i], in[bits[i]] = 1;
  int o = 0;
  for (int b = 0; b < n_local; ++b)
    if (!in[b]) g.opos[o++] = b;
  g.n_outer = o;
  return g;
}

// balanced split of bits into ceil(|bits| / max_bits) contiguous groups
std::vector<std::vector<int>> split_bits(const std::vector<int>& bits, int max_bits) {
  std::vector<std::vector<int>> out;
  const int h = (int)bits.size();
  if (h == 0) return out;
  const int ng = (h + max_bits - 1) / max_bits;
  int first = 0;
  for (int gi = 0; gi < ng; ++gi) {
    const int s = h / ng + (gi < h % ng ? 1 : 0);
    out.emplace_back(bits.begin() + first, bits.begin() + first + s);
    first += s;
  }
  return out;
}

// Tile-bit groups of a register of n_local local qubits (w.grp, returns G; 0: not possible).
// Group 0 = local bits 0..wl-1.  Unpartitioned: the high bits in balanced groups of <= max_bits,
// the last one is MID's.  Partitioned (S shard bits): the pre-swap groups must transform the top
// S local bits T (they leave with the index swap); MID transforms the shard bits that arrive in
// T's positions together with up to max_bits - S other local high bits.
//
// mid_inpage m > 0 (option wht_mid_inpage, unpartitioned registers): the MID group takes the top m
// high bits below the 2-MiB page (local bits < kWhtPageBit) in place of its lowest above-page
// bits, the other groups the rest.  A pass's tile touches 2^(its group's above-page bits) pages;
// with the contiguous split MID's group lies wholly above the page (N = 30: 256 pages per tile,
// a TLB miss on 61% of its requests) while FWD's keeps every in-page bit (32 pages).
constexpr int kWhtPageBit = 17;  // 2^17 amplitudes of 16 B = 2 MiB
int wht_layout(int n_local, int S, int wl, int max_bits, WhtProb& w, int mid_inpage = 0) {
  const int h = n_local - wl;
  if (h < 1 || h > kWhtMaxOuter || h < S || max_bits <= S) return 0;
  std::vector<int> high;
  for (int b = wl; b < n_local; ++b) high.push_back(b);
  std::vector<std::vector<int>> groups;
  if (S == 0) {
    groups = split_bits(high, max_bits);
    if (mid_inpage > 0 && groups.size() >= 2) {
      std::vector<int> inpage, above;
      for (int b : high) (b < kWhtPageBit ? inpage : above).push_back(b);
      const int smid = (int)groups.back().size();
      const int m = std::min({mid_inpage, (int)inpage.size(), smid});
      if (m > 0 && (int)above.size() >= smid - m) {
        std::vector<int> mid(inpage.end() - m, inpage.end());
        mid.insert(mid.end(), above.end() - (smid - m), above.end());
        std::vector<int> rest;
        for (int b : high)
          if (std::find(mid.begin(), mid.end(), b) == mid.end()) rest.push_back(b);
        groups = split_bits(rest, max_bits);
        groups.push_back(mid);
      }
    }
  } else {
    const std::vector<int> rest(high.begin(), high.end() - S), T(high.end() - S, high.end());
    const int m = std::min(max_bits - S, (int)rest.size());
    std::vector<int> mid(rest.begin(), rest.begin() + m), pre(rest.begin() + m, rest.end());
    pre.insert(pre.end(), T.begin(), T.end());
    groups = split_bits(pre, max_bits);
    mid.insert(mid.end(), T.begin(), T.end());
    groups.push_back(mid);
  }
  if ((int)groups.size() + 1 > kWhtMaxGroups) return 0;
  w.grp[0] = make_group({}, wl, n_local);  // pos = 0..wl-1, outer = the high bits
  w.grp[0].c = 0;                           // group 0 transforms all its tile bits
  for (size_t gi = 0; gi < groups.size(); ++gi) w.grp[gi + 1] = make_group(groups[gi], wl, n_local);
  return (int)groups.size() + 1;
}

// Builds the engine's tables and vectors for the problems it can take: registers of more than one
// tile, whole or partitioned (loopback shards or one shard per process).  Idempotent until
// free_device.
int ensure_wht(dse_ctx* ctx) {
  if (ctx->wht_ready) return DSE_OK;
  std::vector<WhtProb> hw(ctx->probs.size());
  std::memset(hw.data(), 0, hw.size() * sizeof(WhtProb));
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    HostProblem& p = ctx->probs[pi];
    p.wht_groups = 0;
    if (!ctx->wht || p.L < kWhtMinTile || p.L > kWhtMaxTile || p.n_tiles < 2) continue;
    const int n = p.n, nl = p.n_local, S = p.shard_bits;
    WhtProb& w = hw[pi];
    const int gb = ctx->wht_group_bits ? std::min(ctx->wht_group_bits, p.L - 2) : p.L - 2;
    const int G = wht_layout(nl, S, p.L, gb, w, ctx->wht_mid_inpage);
    if (G < 2) continue;
    const double sc = std::ldexp(1.0, -n);
    std::vector<double> cq(size_t(n) * n, 0.0);
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) cq[size_t(i) * n + j] = cq[size_t(j) * n + i] = 0.5 * p.pair[i * n + j] * sc;
    for (int b = 0; b < n; ++b) {
      double re = p.flip[4 * b + 2], im = p.flip[4 * b + 3];
      if (std::fabs(re) <= 1e-15 * std::hypot(re, im)) re = 0.0;  // as build_tables
      w.lin_x[b] = re * sc;
      w.lin_y[b] = im * sc;
    }
    const size_t vbytes = (size_t(1) << nl) * sizeof(double2);
    const int nvec = S > 0 ? 4 : 2;
    bool ok = hipMalloc(&p.d_cquad, cq.size() * sizeof(double)) == hipSuccess &&
              hipMalloc(&p.d_wtab, ((size_t)p.n_tiles * 48 + 2 * (5 * 512 + 16)) * sizeof(double)) == hipSuccess;
    // option wht_contiguous: the X/Y-branch vectors physically contiguous (large translation
    // fragments for the strided passes), else (or when that fails) a plain allocation
    for (int v = 0; v < nvec && ok; ++v) {
      if (ctx->wht_contiguous &&
          hipExtMallocWithFlags((void**)&p.wvec[v], vbytes, hipDeviceMallocContiguous) == hipSuccess)
        continue;
      (void)hipGetLastError();
      ok = hipMalloc(&p.wvec[v], vbytes) == hipSuccess;
    }
    if (!ok) {  // HBM too small for the engine's two extra vectors: this problem keeps the step kernels
      (void)hipGetLastError();
      free_wht(p);
      std::memset(&w, 0, sizeof(w));
      continue;
    }
    HIPC(hipMemcpy(p.d_cquad, cq.data(), cq.size() * sizeof(double), hipMemcpyHostToDevice));
    w.vec_a = p.wvec[0];
    w.vec_b = p.wvec[1];
    w.vec_at = S > 0 ? p.wvec[2] : p.wvec[0];
    w.vec_bt = S > 0 ? p.wvec[3] : p.wvec[1];
    for (int b = 0; b < n; ++b) w.gmap[b] = b;
    if (S > 0) {  // MID state: local bits nl-S+i hold global nl+i, the rank holds global nl-S+i
      for (int i = 0; i < S; ++i) w.gmap[nl - S + i] = nl + i;
      w.fix_mask = ((uint64_t(1) << S) - 1) << (nl - S);
      w.fix_val = (uint64_t)p.shard_rank << (nl - S);
      w.phase0 = __builtin_popcount((unsigned)p.shard_rank);
    }
    w.cquad = p.d_cquad;
    w.ztab = p.d_wtab;
    w.xytab = p.d_wtab + (size_t)p.n_tiles * 16;
    w.qtab = p.d_wtab + (size_t)p.n_tiles * 48;
    w.n = n;
    w.n_local = nl;
    w.wl = p.L;
    w.n_groups = G;
    p.wht_groups = G;
  }
  // the shards of a loopback register run the same launches: all on the engine or none
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    if (P.shard_bits == 0 || P.dist || P.shard_rank != 0) continue;
    bool all = true;
    for (int r = 0; r < (1 << P.shard_bits); ++r) all = all && ctx->probs[pi + r].wht_groups > 0;
    if (all) continue;
    for (int r = 0; r < (1 << P.shard_bits); ++r) {
      free_wht(ctx->probs[pi + r]);
      std::memset(&hw[pi + r], 0, sizeof(WhtProb));
    }
  }
  if (!ctx->d_wht && hipMalloc(&ctx->d_wht, hw.size() * sizeof(WhtProb)) != hipSuccess)
    return fail(ctx, DSE_ERR_OOM, "device allocation of descriptors failed");
  HIPC(hipMemcpy(ctx->d_wht, hw.data(), hw.size() * sizeof(WhtProb), hipMemcpyHostToDevice));
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi)
    if (ctx->probs[pi].wht_groups)
      HIPC(launch_wht_tables(ctx->probs[pi].L, ctx->d_wht + pi, ctx->d_probs + pi, ctx->probs[pi].n_tiles, ctx->lanes[0].stream));
  HIPC(hipStreamSynchronize(ctx->lanes[0].stream));
  ctx->wht_ready = true;
  return DSE_OK;
}

// ---- exchanges of a register partitioned over processes: RCCL, or the host transport ----
// all-to-all of equal chunks (chunk p -> rank p), device buffers
// Exchange timing: xt_begin/xt_end bracket one exchange on stream st with a HIP event pair
// (RCCL path; pairs beyond the pool are not timed); xt_sum adds the finished pairs to ctx->xms.
int xt_begin(dse_ctx* ctx, hipStream_t st, size_t* slot) {
  *slot = SIZE_MAX;
  if (ctx->xev_used >= 4096) return DSE_OK;
  while (ctx->xev.size() < 2 * (ctx->xev_used + 1)) {
    hipEvent_t e;
    HIPC(hipEventCreate(&e));
    ctx->xev.push_back(e);
  }
  *slot = ctx->xev_used++;
  HIPC(hipEventRecord(ctx->xev[2 * *slot], st));
  return DSE_OK;
}

int xt_end(dse_ctx* ctx, hipStream_t st, size_t slot) {
  if (slot != SIZE_MAX) HIPC(hipEventRecord(ctx->xev[2 * slot + 1], st));
  return DSE_OK;
}

int xt_sum(dse_ctx* ctx) {
  for (size_t i = 0; i < ctx->xev_used; ++i) {
    HIPC(hipEventSynchronize(ctx->xev[2 * i + 1]));
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, ctx->xev[2 * i], ctx->xev[2 * i + 1]));
    ctx->xms += ms;
  }
  ctx->xev_used = 0;
  return DSE_OK;
}

double host_ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int xchg_alltoall(dse_ctx* ctx, const void* src, void* dst, size_t cbytes, hipStream_t st) {
  ctx->xbytes += (double)cbytes * (ctx->dist_world - 1);
  if (!ctx->xfn) {
    size_t slot;
    int rc = xt_begin(ctx, st, &slot);
    if (rc) return rc;
    const ncclResult_t r = ncclAllToAll(src, dst, cbytes, ncclUint8, ctx->comm, st);
    if (r != ncclSuccess) return fail(ctx, DSE_ERR_HIP, std::string("ncclAllToAll: ") + ncclGetErrorString(r));
    return xt_end(ctx, st, slot);
  }
  const auto h0 = std::chrono::steady_clock::now();
  struct AddMs {
    dse_ctx* c;
    std::chrono::steady_clock::time_point t0;
    ~AddMs() { c->xms += host_ms_since(t0); }
  } add_ms{ctx, h0};
  const size_t total = cbytes * ctx->dist_world;
  ctx->xsend.resize(total);
  ctx->xrecv.resize(total);
  HIPC(hipMemcpyAsync(ctx->xsend.data(), src, total, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  if (ctx->xfn(ctx->xuser, DSE_XCHG_ALLTOALL, ctx->xsend.data(), ctx->xrecv.data(), cbytes, -1) != 0)
    return fail(ctx, DSE_ERR_HIP, "exchange callback (all-to-all) failed");
  HIPC(hipMemcpyAsync(dst, ctx->xrecv.data(), total, hipMemcpyHostToDevice, st));
  HIPC(hipStreamSynchronize(st));
  return DSE_OK;
}

// in-place sum over ranks of host doubles
int xchg_allreduce_host(dse_ctx* ctx, double* v, size_t count, hipStream_t st) {
  if (ctx->xfn) {
    if (ctx->xfn(ctx->xuser, DSE_XCHG_ALLREDUCE_F64, v, v, count * sizeof(double), -1) != 0)
      return fail(ctx, DSE_ERR_HIP, "exchange callback (all-reduce) failed");
    return DSE_OK;
  }
  // one staging buffer per context, grown on demand
  if (int rc = ctx->d_allreduce.reserve(ctx, count, "all-reduce staging allocation failed")) return rc;
  double* d = ctx->d_allreduce.p;
  hipError_t e = hipMemcpyAsync(d, v, count * sizeof(double), hipMemcpyHostToDevice, st);
  const ncclResult_t r = ncclAllReduce(d, d, count, ncclFloat64, ncclSum, ctx->comm, st);
  if (e == hipSuccess) e = hipMemcpyAsync(v, d, count * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (r != ncclSuccess) return fail(ctx, DSE_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
  HIPC(e);
  return DSE_OK;
}

// Index swap of the X/Y vectors of partitioned registers (local top S bits <-> shard bits):
// chunk p of shard r -> chunk r of shard p; an involution, so back = the same exchange from the
// swapped copies.  Loopback registers: device copies; one shard per process: RCCL all-to-all.
int wht_swap(dse_ctx* ctx, const std::vector<int>& regs, bool back, hipStream_t st, int vsel = 3) {
  for (int first : regs) {
    const HostProblem& P0 = ctx->probs[first];
    const int S = P0.shard_bits;
    const size_t chunk = size_t(1) << (P0.n_local - S);
    const size_t cbytes = chunk * sizeof(double2);
    for (int v = 0; v < 2; ++v) {
      if (!((vsel >> v) & 1)) continue;
      if (P0.dist) {
        const double2* src = P0.wvec[back ? 2 + v : v];
        double2* dst = P0.wvec[back ? v : 2 + v];
        const int rc = xchg_alltoall(ctx, src, dst, cbytes, st);
        if (rc) return rc;
        continue;
      }
      for (int r = 0; r < (1 << S); ++r)
        for (int p = 0; p < (1 << S); ++p) {
          const HostProblem& Pr = ctx->probs[first + r];
          const HostProblem& Pp = ctx->probs[first + p];
          const double2* src = (back ? Pr.wvec[2 + v] : Pr.wvec[v]) + p * chunk;
          double2* dst = (back ? Pp.wvec[v] : Pp.wvec[2 + v]) + r * chunk;
          HIPC(hipMemcpyAsync(dst, src, cbytes, hipMemcpyDeviceToDevice, st));
        }
    }
  }
  return DSE_OK;
}

// One WHT application (mode / term k) over items of problems with wht_groups == G, tile wl;
// regs: first problem of every partitioned register among them (index swaps around MID).
// segs: (items, count) launches of the same wl / G.  fuse: FINAL of term k runs term k + 1's
// FIRST; the caller decides it once for all terms of an evolve (a term that skips FIRST relies on
// the previous term's FINAL_NEXT), never from the registers still active at term k.
int wht_run(dse_ctx* ctx, int wl, int G, const std::vector<std::pair<const int2*, int>>& segs,
            const std::vector<int>& regs, bool fuse, int mode, int k, int q, int set, hipStream_t st) {
  int rc;
  auto part = [&](int pt, int vsel) -> int {
    for (const auto& sg : segs)
      HIPC(launch_wht_part(pt, wl, mode, G, ctx->d_wht, ctx->d_probs, sg.first, sg.second, k, q, set, vsel, st,
                           ctx->n_cu * (wl == 13 ? 1 : 2),
                           ctx->wht_persist | ctx->wht_half << 8 | (int)fuse << 16));
    return DSE_OK;
  };
  if (regs.empty() || !ctx->swap_overlap) {
    for (int pt = WHT_PART_PRE; pt <= WHT_PART_POST; ++pt) {
      if (pt == WHT_PART_MID && !regs.empty() && (rc = wht_swap(ctx, regs, false, st))) return rc;
      if (pt == WHT_PART_POST && !regs.empty() && (rc = wht_swap(ctx, regs, true, st))) return rc;
      if ((rc = part(pt, 3))) return rc;
    }
    return DSE_OK;
  }
  // Partitioned registers: the X-branch vector A and the Y-branch vector B are transformed in
  // separate launches, and each index swap (all-to-all over the shards) runs on swap_stream while
  // the compute stream works on the other vector:
  //   st    FIRST+FWD(A) | FWD(B) |        MID(A) |        MID(B) |        INV(A) |  INV(B)+FINAL
  //   swap               | swap A | swap B        | back A        | back B
  // ev[v]: vector v ready on st for its swap, ev[2+v]: swapped, ev[4+v]: MID done, ev[6+v]: back.
  if (!ctx->swap_stream) {
    HIPC(hipStreamCreateWithFlags(&ctx->swap_stream, hipStreamNonBlocking));
    for (auto& e : ctx->swap_ev) HIPC(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  hipStream_t sw = ctx->swap_stream;
  hipEvent_t* ev = ctx->swap_ev;
  // the swap stream takes over vector v once event i is reached on the compute stream, swaps it
  // (there, or back), and marks event j when done
  auto swap_after = [&](int i, int v, bool back, int j) -> int {
    HIPC(hipEventRecord(ev[i], st));
    HIPC(hipStreamWaitEvent(sw, ev[i], 0));
    const int r = wht_swap(ctx, regs, back, sw, 1 << v);
    if (r) return r;
    HIPC(hipEventRecord(ev[j], sw));
    return DSE_OK;
  };
  auto wait_swap = [&](int j) -> int {
    HIPC(hipStreamWaitEvent(st, ev[j], 0));
    return DSE_OK;
  };
  for (int v = 0; v < 2; ++v)  // PRE of A (with FIRST), then of B; each vector's swap behind it
    if ((rc = part(WHT_PART_PRE, 1 << v)) || (rc = swap_after(v, v, false, 2 + v))) return rc;
  for (int v = 0; v < 2; ++v)  // MID of a vector once it is swapped; its swap back behind it
    if ((rc = wait_swap(2 + v)) || (rc = part(WHT_PART_MID, 1 << v)) || (rc = swap_after(4 + v, v, true, 6 + v)))
      return rc;
  for (int v = 0; v < 2; ++v)  // POST: INV(A), then INV(B) + FINAL
    if ((rc = wait_swap(6 + v)) || (rc = part(WHT_PART_POST, 1 << v))) return rc;
  return DSE_OK;
}

// The three partial arenas (aggregate, site and pair observables) hold the sums of up to `slots`
// output times before a flush copies them back; one slot of any of them stays within this cap
constexpr int64_t kPartialCapBytes = 256ll << 20;

int widest_register(const dse_ctx* ctx) {  // qubits (1 for an empty context)
  int n_max = 1;
  for (const auto& P : ctx->probs) n_max = std::max(n_max, P.n);
  return n_max;
}

// slots per flush of an arena of per_slot bytes per output time: what the cap holds, at most the
// n_t outputs there are and at least the M outputs of one launch (they share a flush)
size_t partial_chunk(int64_t per_slot, int M, int n_t) {
  return (size_t)std::max<int64_t>(M, std::min<int64_t>(n_t, std::max<int64_t>(1, kPartialCapBytes / per_slot)));
}

int ensure_partial(dse_ctx* ctx, size_t slots) {
  if (ctx->partial_slots >= slots) return DSE_OK;
  ctx->partial_slots = 0;
  ctx->d_partial.release();
  if (int rc = ctx->d_partial.reserve(ctx, slots * ctx->total_items * 8, "device allocation of observable partials failed"))
    return rc;
  ctx->partial_slots = slots;
  return DSE_OK;
}

// ---- observable families: site-resolved observables and two-spin correlators ------------------


// The overlap, string and sector families have no option: each is on while any register of the context
// holds references / strings / sets, and its stride follows the most any of them holds.  All reach the
// kernels through the descriptors: h_desc as dse_evolve uploads it, and with `upload` (the hooks: no
// upload follows) the device copy, every time (an evolve that failed before its upload leaves h_desc
// ahead of it).  After prepare.
int set_unit_families_on(dse_ctx* ctx, bool upload) {
  int kmax[kNumObsFamilies] = {};
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    for (ObsFamily f : kObsLaunchOrder)
      if (kObsFamilies[f].per_problem_units) kmax[f] = std::max(kmax[f], kObsFamilies[f].units(P));
    ctx->h_desc[pi].ovl_refs = P.d_ovl_tab;
    ctx->h_desc[pi].ovl_k = P.ovl_k();
    ctx->h_desc[pi].str_tab = P.d_str_tab;
    ctx->h_desc[pi].str_k = P.str_k();
    ctx->h_desc[pi].sec_tab = P.d_sec_tab;
    ctx->h_desc[pi].sec_k = P.sec_k();
  }
  for (ObsFamily f : kObsLaunchOrder) {
    if (!kObsFamilies[f].per_problem_units) continue;
    ctx->fam[f].kmax = kmax[f];
    ctx->fam[f].on = kmax[f] > 0;
  }
  if (upload)
    HIPC(hipMemcpy(ctx->d_probs, ctx->h_desc.data(), ctx->h_desc.size() * sizeof(DevProb), hipMemcpyHostToDevice));
  return DSE_OK;
}

// Refusals of the option and of the hook (`who`), decided before any work (after prepare: the tile
// count is known): no register partitioned over processes, and with slot_cap one output slot of the
// arena, tiles x stride(n_max) doubles, within the cap of the other arenas
int obs_family_refusal(dse_ctx* ctx, ObsFamily f, const char* who) {
  const ObsFamilyDesc& F = kObsFamilies[f];
  for (const auto& P : ctx->probs)
    if (P.dist)
      return fail(ctx, DSE_ERR_ARG, std::string(who) + ": not available for a register partitioned over processes "
                                        "(the all-reduce of the " + F.noun + " sums is not implemented)");
  const int S = F.stride(ctx, widest_register(ctx));
  if (F.slot_cap && ctx->total_items * (int64_t)S * 8 > kPartialCapBytes)
    return fail(ctx, DSE_ERR_ARG, std::string(who) + ": the " + F.noun + " sums of one output (" +
                                      std::to_string(ctx->total_items) + " tiles x " + std::to_string(S) +
                                      " doubles) exceed the 256 MiB partial arena");
  return DSE_OK;
}

// the family's arena: slots x total_items x S doubles, S = its stride of the widest register of the
// context (total_items >= 1: prepare refuses an empty context)
int ensure_family_partial(dse_ctx* ctx, ObsFamily f, size_t slots) {
  ObsFamilyState& A = ctx->fam[f];
  const int S = kObsFamilies[f].stride(ctx, widest_register(ctx));
  if (A.slots >= slots && A.S == S) return DSE_OK;
  A.slots = 0;
  A.d_partial.release();
  const std::string what = std::string("device allocation of ") + kObsFamilies[f].noun + "-observable partials failed";
  if (int rc = A.d_partial.reserve(ctx, slots * ctx->total_items * S, what.c_str())) return rc;
  A.slots = slots;
  A.S = S;
  return DSE_OK;
}

// raw sums v (a record of S doubles) of register P, normalised into o[c][u] at o[(c * units + u) * stride]
void finish_family(const ObsFamilyDesc& F, const HostProblem& P, const double* v, size_t S, double* o, size_t stride) {
  const int units = F.units(P);
  const double n2 = v[family_norm_at(F, units, S)];
  const double inv = n2 > 0.0 ? 1.0 / (F.amplitude ? std::sqrt(n2) : n2) : 0.0;
  for (int u = 0; u < units; ++u)
    for (int c = 0; c < F.comps; ++c) o[((size_t)c * units + u) * stride] = v[F.comps * u + c] * inv;
}

}  // namespace

namespace dse::rt {
// finish_family for register pi's outputs 0 .. n_t - 1, raw sums `stride` doubles apart, into its store
// (a register without a record, an empty store: nothing)
void finish_family_outputs(dse_ctx* ctx, ObsFamily f, size_t pi, const double* raw, size_t stride, int n_t) {
  if (ctx->fam[f].store[pi].empty()) return;
  for (int ti = 0; ti < n_t; ++ti)
    finish_family(kObsFamilies[f], ctx->probs[pi], raw + ti * stride, stride, ctx->fam[f].store[pi].data() + ti, (size_t)n_t);
}
}  // namespace dse::rt

namespace {

size_t obs_store_size(ObsFamily f, const HostProblem& P, int n_t) {
  return (size_t)kObsFamilies[f].comps * kObsFamilies[f].units(P) * n_t;
}
// which registers keep a record (a loopback group's sums live in shard 0's entry; a family whose units
// are the problem's own: the registers that have any)
bool obs_record(const dse_ctx* ctx, ObsFamily f, const HostProblem& P) {
  return ctx->fam[f].on && !(P.shard_bits > 0 && P.shard_rank != 0) &&
         !(kObsFamilies[f].per_problem_units && kObsFamilies[f].units(P) == 0);
}
// registers with a record from the last evolve (0 unless it succeeded with the option on)
int obs_family_problems(const dse_ctx* ctx, ObsFamily f) { return ctx->fam[f].nt > 0 ? ctx->fam[f].problems : 0; }

// A fresh store for this evolve (dse_evolve has already marked the old one invalid, nt = 0; it
// becomes readable again only when the evolve succeeds).  The re-run after a hand-off timeout starts
// over as well (its results overwrite the first pass's), except for the dense registers, whose
// first-pass results are kept like their aggregates (dense_run is not repeated).
void reset_family_store(dse_ctx* ctx, ObsFamily f, int n_t) {
  std::vector<std::vector<double>>& store = ctx->fam[f].store;
  store.resize(ctx->probs.size());
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    const size_t want = obs_record(ctx, f, P) ? obs_store_size(f, P, n_t) : 0;
    if (ctx->rerun && P.dn && store[pi].size() == want) continue;
    store[pi].assign(want, 0.0);
  }
}

// the family's part of flush_partials: tiles in order, a loopback group's members into shard 0's record
int flush_family_partials(dse_ctx* ctx, ObsFamily f, size_t nslots, size_t t0, int n_t) {
  const ObsFamilyDesc& F = kObsFamilies[f];
  ObsFamilyState& A = ctx->fam[f];
  const size_t S = (size_t)A.S;
  std::vector<double> hs(nslots * ctx->total_items * S);
  HIPC(hipMemcpy(hs.data(), A.d_partial.p, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> v(S);
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    if (P.side() || A.store[pi].empty()) continue;
    const size_t n_members = P.shard_bits > 0 ? (size_t(1) << P.shard_bits) : 1;
    const int nv = F.comps * F.units(P), nrm = family_norm_at(F, F.units(P), S);
    for (size_t s = 0; s < nslots; ++s) {
      std::fill(v.begin(), v.end(), 0.0);
      for (size_t mi = pi; mi < pi + n_members; ++mi) {
        const double* row = hs.data() + (s * ctx->total_items + ctx->item_pos[mi]) * S;
        for (int64_t t = 0; t < ctx->probs[mi].n_tiles; ++t) {
          for (int j = 0; j < nv; ++j) v[j] += row[t * S + j];
          v[nrm] += row[t * S + nrm];
        }
      }
      finish_family(F, P, v.data(), S, A.store[pi].data() + (t0 + s), (size_t)n_t);
    }
  }
  return DSE_OK;
}

}  // namespace

namespace dse::rt {
void finish_obs(const HostProblem& P, const double* v, double* o, size_t stride) {
  const double n2 = v[6];
  const double inv = n2 > 0.0 ? 1.0 / n2 : 0.0;
  o[0 * stride] = v[0] * inv;
  o[1 * stride] = v[1] * inv;
  o[2 * stride] = v[2] * inv;
  o[3 * stride] = P.rare_bit >= 0 ? v[3] * inv : P.rare_z;
  o[4 * stride] = P.rare_bit >= 0 ? v[4] * inv : 0.0;
  o[5 * stride] = P.rare_bit >= 0 ? v[5] * inv : 0.0;
  o[6 * stride] = std::sqrt(n2);
}
}  // namespace dse::rt

namespace {

// Observable sums of output slots [t0, t0 + nslots).  A loopback shard group sums the tiles of all
// its shards and writes the result to every shard's row; a dist shard keeps its raw local sums in
// dist_raw for the all-reduce at the end of dse_evolve.
int flush_partials(dse_ctx* ctx, size_t nslots, size_t t0, int n_t, double* obs_out,
                   std::vector<double>* dist_raw) {
  if ((int)sync_lanes(ctx)) return DSE_ERR_HIP;
  if (ctx->d_err_cur) {  // a persistent hand-off timed out: abandon this run (dse_evolve falls back)
    int herr = 0;
    HIPC(hipMemcpy(&herr, ctx->d_err_cur, sizeof(int), hipMemcpyDeviceToHost));
    if (herr) return kRcHandoffTimeout;
  }
  std::vector<double> h(nslots * ctx->total_items * 8);
  HIPC(hipMemcpy(h.data(), ctx->d_partial.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    if (P.side()) continue;  // the small-register engine writes its own sums
    const bool grouped = P.shard_bits > 0 && !P.dist;
    const size_t first_member = grouped ? (size_t)P.group_first : pi;
    const size_t n_members = grouped ? (size_t(1) << P.shard_bits) : 1;
    for (size_t s = 0; s < nslots; ++s) {
      double v[7] = {0, 0, 0, 0, 0, 0, 0};
      for (size_t mi = first_member; mi < first_member + n_members; ++mi) {
        const double* row = h.data() + (s * ctx->total_items + ctx->item_pos[mi]) * 8;
        for (int64_t t = 0; t < ctx->probs[mi].n_tiles; ++t)
          for (int j = 0; j < 7; ++j) v[j] += row[t * 8 + j];
      }
      if (P.dist) {
        double* raw = dist_raw->data() + (pi * (size_t)n_t + t0 + s) * 7;
        for (int j = 0; j < 7; ++j) raw[j] = v[j];
      } else {
        finish_obs(P, v, obs_out + pi * DSE_N_OBS * (size_t)n_t + (t0 + s), (size_t)n_t);
      }
    }
  }
  for (ObsFamily f : kObsReadbackOrder)  // the family sums of the same slots
    if (ctx->fam[f].on)
      if (int rc = flush_family_partials(ctx, f, nslots, t0, n_t)) return rc;
  return DSE_OK;
}

// RCCL exchange for dist shards: every shard sends its role-`role` vector to each partner rank ^ m
// it shares terms with and receives the partner's into rbuf_own[m] (min_degree: only problems
// whose Chebyshev degree reaches the current term).
int dist_exchange(dse_ctx* ctx, int role, int min_degree, hipStream_t st) {
  for (auto& P : ctx->probs) {
    if (!P.dist || P.degree < min_degree || !P.xmasks) continue;
    const size_t bytes = (size_t(1) << P.n_local) * sizeof(double2);
    if (ctx->xfn) {  // host transport: one blocking send/recv per partner, masks in ascending order
      struct AddMs {
        dse_ctx* c;
        std::chrono::steady_clock::time_point t0;
        ~AddMs() { c->xms += host_ms_since(t0); }
      } add_ms{ctx, std::chrono::steady_clock::now()};
      ctx->xsend.resize(bytes);
      ctx->xrecv.resize(bytes);
      HIPC(hipMemcpyAsync(ctx->xsend.data(), P.buf[role], bytes, hipMemcpyDeviceToHost, st));
      HIPC(hipStreamSynchronize(st));
      for (int m = 1; m < (1 << P.shard_bits); ++m) {
        if (!((P.xmasks >> m) & 1u)) continue;
        ctx->xbytes += (double)bytes;
        if (ctx->xfn(ctx->xuser, DSE_XCHG_SENDRECV, ctx->xsend.data(), ctx->xrecv.data(), bytes,
                     ctx->dist_rank ^ m) != 0)
          return fail(ctx, DSE_ERR_HIP, "exchange callback (send/recv) failed");
        HIPC(hipMemcpyAsync(P.rbuf_own[m], ctx->xrecv.data(), bytes, hipMemcpyHostToDevice, st));
        HIPC(hipStreamSynchronize(st));
      }
      continue;
    }
    size_t slot;
    int rc = xt_begin(ctx, st, &slot);
    if (rc) return rc;
    if (ncclGroupStart() != ncclSuccess) return fail(ctx, DSE_ERR_HIP, "ncclGroupStart failed");
    for (int m = 1; m < (1 << P.shard_bits); ++m) {
      if (!((P.xmasks >> m) & 1u)) continue;
      const int peer = ctx->dist_rank ^ m;
      ctx->xbytes += (double)bytes;
      ncclResult_t r1 = ncclSend(P.buf[role], bytes, ncclUint8, peer, ctx->comm, st);
      ncclResult_t r2 = ncclRecv(P.rbuf_own[m], bytes, ncclUint8, peer, ctx->comm, st);
      if (r1 != ncclSuccess || r2 != ncclSuccess) {
        (void)ncclGroupEnd();
        return fail(ctx, DSE_ERR_HIP, std::string("RCCL send/recv: ") + ncclGetErrorString(r1 != ncclSuccess ? r1 : r2));
      }
    }
    const ncclResult_t r = ncclGroupEnd();
    if (r != ncclSuccess) return fail(ctx, DSE_ERR_HIP, std::string("ncclGroupEnd: ") + ncclGetErrorString(r));
    if ((rc = xt_end(ctx, st, slot))) return rc;
  }
  return DSE_OK;
}

int ensure_events(dse_ctx* ctx, Lane& ln, size_t per_pool) {
  for (int p = 0; p < 2; ++p)
    while (ln.ev[p].size() < 2 * per_pool) {
      hipEvent_t e;
      HIPC(hipEventCreate(&e));
      ln.ev[p].push_back(e);
    }
  return DSE_OK;
}

// ---- options (dse_set_option) -------------------------------------------------------------------
// How a value is checked, and what it is stored as
enum class OptCheck {
  Bool,   // any value, NaN too: stored as value != 0.0
  Int,    // any value: stored as (int)value
  Range,  // lo <= value <= hi or one of `also`, else the message: stored as (int)value
  Whole,  // the same, the values of the range whole numbers
};
// Reset: the device layout depends on the option, so when its stored value changes the context's
// streams are drained and its device state is released first (rebuilt by the next prepare)
enum class OptEffect { Store, Reset };

constexpr double kNoValue = std::numeric_limits<double>::quiet_NaN();  // in `also`: equals no value

struct Option {
  const char* key;
  int dse_ctx::*field;
  OptCheck check;
  OptEffect effect = OptEffect::Store;
  double lo = 0.0, hi = 0.0;
  std::string msg;
  double also[2] = {kNoValue, kNoValue};
};

bool option_accepts(const Option& o, double value) {
  if (o.check == OptCheck::Bool || o.check == OptCheck::Int) return true;
  if (value >= o.lo && value <= o.hi && (o.check == OptCheck::Range || value == (int)value)) return true;
  return value == o.also[0] || value == o.also[1];
}

// Every option that is one int of the context.  streams, the observable families, the hand-off
// knobs, the ablation masks, probe_items and max_degree are not: dse_set_option spells them out.
const Option kOptions[] = {
    {"tile_bits", &dse_ctx::tile_bits, OptCheck::Range, OptEffect::Reset, 1, kMaxTile, "tile_bits must be in 1..13"},
    {"persistent", &dse_ctx::persistent, OptCheck::Bool},
    {"swap_overlap", &dse_ctx::swap_overlap, OptCheck::Bool},
    {"wht", &dse_ctx::wht, OptCheck::Bool, OptEffect::Reset},
    // Walsh-Hadamard engine's vectors physically contiguous
    {"wht_contiguous", &dse_ctx::wht_contiguous, OptCheck::Whole, OptEffect::Reset, 0, 1, "wht_contiguous must be 0 or 1"},
    // Walsh-Hadamard engine: FINAL of term k + FIRST of term k + 1
    {"wht_fuse", &dse_ctx::wht_fuse, OptCheck::Whole, OptEffect::Store, 0, 1, "wht_fuse must be 0 or 1"},
    // Walsh-Hadamard plan: MID group's high bits below the page
    {"wht_mid_inpage", &dse_ctx::wht_mid_inpage, OptCheck::Whole, OptEffect::Reset, 0, 8, "wht_mid_inpage must be 0..8"},
    // Walsh-Hadamard passes through half the LDS, two workgroups per CU
    {"wht_half", &dse_ctx::wht_half, OptCheck::Whole, OptEffect::Store, 0, 7, "wht_half must be 0..7"},
    // Walsh-Hadamard passes as persistent launches: bit 1 MID
    {"wht_persist", &dse_ctx::wht_persist, OptCheck::Int},
    {"wht_tile_bits", &dse_ctx::wht_tile_bits, OptCheck::Whole, OptEffect::Reset, 12, 13, "wht_tile_bits must be 0, 12 or 13", {0, kNoValue}},
    {"wht_group_bits", &dse_ctx::wht_group_bits, OptCheck::Range, OptEffect::Reset, 2, 11, "wht_group_bits must be 0 or in 2..11", {0, kNoValue}},
    {"outputs_per_launch", &dse_ctx::outputs_per_launch, OptCheck::Range, OptEffect::Store, 1, kMaxOut,
     "outputs_per_launch must be in 1.." + std::to_string(kMaxOut)},
    // M of an evolve whose registers all span (k_span)
    {"span_outputs", &dse_ctx::span_outputs, OptCheck::Range, OptEffect::Store, 1, kSpanMaxOut,
     "span_outputs must be in 1.." + std::to_string(kSpanMaxOut)},
    // diagnostics: workgroups per chunk of a 2-tile interval launch
    {"coresident", &dse_ctx::coresident, OptCheck::Range, OptEffect::Store, 2, 4096, "coresident must be 0 or in 2..4096", {0, kNoValue}},
    // diagnostics bit mask: 1 one observable launch per output, 2 psi0 by memset/copy, 4 coefficient
    // tables on one host thread
    {"dbg", &dse_ctx::dbg, OptCheck::Int},
    // registers of <= 9 qubits on the one-wave engine (dse_small.hip)
    {"small", &dse_ctx::small, OptCheck::Bool},
    // propagator-matrix mode: 0 off, 1 auto, 2 always (when eligible)
    {"matrix", &dse_ctx::matrix, OptCheck::Whole, OptEffect::Store, 0, 2, "matrix must be 0, 1 or 2"},
    // dense engine: large eigendecompositions at a time (1..8)
    {"eig_streams", &dse_ctx::eig_streams, OptCheck::Range, OptEffect::Store, 1, 8, "eig_streams must be in 1..8"},
    // dense engine eigensolver: 0 dsyevd, 1 auto, 2 half-matrix from 2^10, 3 two-stage from 2^10
    {"eig_impl", &dse_ctx::eig_impl, OptCheck::Range, OptEffect::Store, 0, 3, "eig_impl must be 0, 1, 2 or 3"},
    // two-stage eigensolver: poll rounds before a give-up (< 0: at once)
    {"eig_spin_limit", &dse_ctx::eig_spin, OptCheck::Range, OptEffect::Store, -1, 1 << 30, "eig_spin_limit must be in -1..2^30"},
    // dense engine: refined eigenvalues + double-double phases
    {"dense_refine", &dse_ctx::dense_refine, OptCheck::Bool},
    // dense engine: output times by the non-uniform FFT (0, 1, 2)
    {"dense_nufft", &dse_ctx::dense_nufft, OptCheck::Whole, OptEffect::Store, 0, 2, "dense_nufft must be 0, 1 or 2"},
    // matrix mode: each product's reduction in the product's launch
    {"symv_fused", &dse_ctx::symv_fused, OptCheck::Bool},
    // dense eigen-propagator engine: 0 off, 1 auto (cost model), 2 always
    {"dense", &dse_ctx::dense, OptCheck::Whole, OptEffect::Store, 0, 2, "dense must be 0, 1 or 2"},
    {"small_chunk", &dse_ctx::small_chunk, OptCheck::Range, OptEffect::Store, 1, 1e6, "small_chunk must be in 1..1e6"},
    {"xcd_pairs", &dse_ctx::xcd_pairs, OptCheck::Bool},
    // spanning registers: 0 off, 1..4 top bits (workgroups 2^s per register)
    {"span", &dse_ctx::span, OptCheck::Range, OptEffect::Store, 0, kSpanMaxTop, "span must be in 0..4"},
    // real-component mode for registers of 13 / 14 qubits (imaginary drives)
    {"real", &dse_ctx::real_mode, OptCheck::Whole, OptEffect::Store, 0, 2, "real must be 0, 1 or 2"},
    // the leap path on uniform grids: -1 automatic, 0 never, 1 whenever its conditions hold
    {"leap", &dse_ctx::leap, OptCheck::Whole, OptEffect::Store, -1, 1, "leap must be -1, 0 or 1"},
    // the leap path: workgroups per register and launch, two outputs each
    {"leap_fan", &dse_ctx::leap_fan, OptCheck::Whole, OptEffect::Store, 1, 2, "leap_fan must be 1 or 2"},
    // spanning registers: tile bits L (0 off, -1 auto); n > L qubits span 2^(n-L) tiles
    {"span_tile", &dse_ctx::span_tile, OptCheck::Range, OptEffect::Store, 10, 13, "span_tile must be -1, 0 or in 10..13", {0, -1}},
    // amplitudes per thread of k_span: 2^span_rb (0: 512 threads)
    {"span_rb", &dse_ctx::span_rb, OptCheck::Range, OptEffect::Store, 0, 3, "span_rb must be in 0..3"},
    // auto span policy: span the stiffest registers beside k_interval
    {"span_partial", &dse_ctx::span_partial, OptCheck::Bool},
    // auto span policy: resident launches per interval for all-span
    {"span_chunks", &dse_ctx::span_chunks, OptCheck::Whole, OptEffect::Store, 0, 2, "span_chunks must be 0, 1 or 2"},
    // auto span policy, partial form: log2 tile (10, 11)
    {"span_partial_tile", &dse_ctx::span_partial_tile, OptCheck::Whole, OptEffect::Store, 10, 11, "span_partial_tile must be 10 or 11"},
    {"mixed_launch", &dse_ctx::mixed_launch, OptCheck::Bool},
    {"obs_overlap", &dse_ctx::obs_overlap, OptCheck::Bool},
    {"time_kernels", &dse_ctx::time_every, OptCheck::Range, OptEffect::Store, 0, std::numeric_limits<double>::infinity(),
     "time_kernels must be >= 0"},
};

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int dse_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* dse_create_error(void) { return g_create_err.c_str(); }

int dse_device_memory(int device, double* free_total) {
  if (!free_total) return DSE_ERR_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return DSE_ERR_NODEVICE;
  int prev = 0;
  (void)hipGetDevice(&prev);
  size_t fr = 0, tot = 0;
  const bool ok = hipSetDevice(device) == hipSuccess && hipMemGetInfo(&fr, &tot) == hipSuccess;
  (void)hipSetDevice(prev);
  if (!ok) return DSE_ERR_HIP;
  free_total[0] = (double)fr;
  free_total[1] = (double)tot;
  return DSE_OK;
}

dse_ctx* dse_create(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    g_create_err = "no HIP device available";
    return nullptr;
  }
  if (device < 0 || device >= n) {
    g_create_err = "device index out of range";
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_create_err = "hipSetDevice failed";
    return nullptr;
  }
  dse_ctx* ctx = new (std::nothrow) dse_ctx();
  if (!ctx) {
    g_create_err = "out of host memory";
    return nullptr;
  }
  ctx->device = device;
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
      ctx->n_cu = ncu;
  }
  if (ensure_lanes(ctx) != DSE_OK) {
    g_create_err = "stream creation failed: " + ctx->err;
    delete ctx;
    return nullptr;
  }
  return ctx;
}

void dse_destroy(dse_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)sync_all(ctx);
  free_device(ctx);
  for (auto& p : ctx->probs) free_initial(p), free_overlap_refs(p), free_op_strings(p), free_sectors(p);
  ctx->d_mx.release();
  ctx->d_pulse_tab.release();
  for (auto& e : ctx->pulse_ev)
    if (e) (void)hipEventDestroy(e), e = nullptr;
  destroy_lanes(ctx);
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  delete ctx;
}

const char* dse_last_error(const dse_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int dse_set_option(dse_ctx* ctx, const char* key, double value) {
  if (!ctx || !key) return DSE_ERR_ARG;
  const std::string k(key);
  (void)hipSetDevice(ctx->device);
  for (const Option& o : kOptions) {
    if (k != o.key) continue;
    if (!option_accepts(o, value)) return fail(ctx, DSE_ERR_ARG, o.msg);
    const int v = o.check == OptCheck::Bool ? value != 0.0 : (int)value;
    if (o.effect == OptEffect::Reset && v != ctx->*o.field) {
      (void)sync_all(ctx);
      free_device(ctx);
    }
    ctx->*o.field = v;
    return DSE_OK;
  }
  if (k == "streams") {
    if (!(value >= 1 && value <= 16)) return fail(ctx, DSE_ERR_ARG, "streams must be in 1..16");
    (void)sync_all(ctx);
    ctx->n_streams = (int)value;
    ctx->evolved = false;
    return ensure_lanes(ctx);
  } else if (k == kObsFamilies[kSite].option || k == kObsFamilies[kPair].option) {  // beside the seven aggregates
    if (!(value == 0.0 || value == 1.0)) return fail(ctx, DSE_ERR_ARG, k + " must be 0 or 1");
    ctx->fam[k == kObsFamilies[kSite].option ? kSite : kPair].on = (int)value;
  } else if (k == "handoff_fences") {  // interval kernel: agent release/acquire around each hand-off
    ctx->hk.fences = value != 0.0;
  } else if (k == "spin_limit") {  // diagnostics: partner-flag polls per hand-off (< 0: always fail)
    if (!(value >= -1 && value <= 1 << 30)) return fail(ctx, DSE_ERR_ARG, "spin_limit must be in -1..2^30");
    ctx->hk.spin_limit = (int)value;
  } else if (k == "ablate" || k == "real_ablate" || k == "span_ablate") {
    // diagnostics builds only (-DDSE_DIAG): skip kernel sections (results become wrong); process-wide
    const int m = (int)value;
    const hipError_t e = k == "ablate" ? (set_ablate(m) == hipSuccess ? set_ablate_interval(m) : hipErrorNotSupported)
                         : k == "real_ablate" ? set_real_ablate(m) : set_span_ablate(m);
    if (e == hipErrorNotSupported)
      return fail(ctx, DSE_ERR_ARG, "option " + k + " needs a diagnostics build of libdse (-DDSE_DIAG)");
    if (e != hipSuccess) return fail(ctx, DSE_ERR_ARG, "bad " + k + " mask");
  } else if (k == "probe_items") {  // diagnostics only: dse_time_step_kernel launches this many items
    ctx->probe_items = (int64_t)value;
  } else if (k == "max_degree") {
    if (!(value >= 1)) return fail(ctx, DSE_ERR_ARG, "max_degree must be >= 1");
    ctx->max_degree = value;
  } else {
    return fail(ctx, DSE_ERR_ARG, "unknown option " + k);
  }
  return DSE_OK;
}

}  // extern "C"

namespace {

// Validated host copy of one problem's tables (dse_add_problem / dse_add_problem_sharded).
int make_problem(dse_ctx* ctx, HostProblem& p, int n, const double* field, const double* zz,
                 const double* pair, const double* flip, double shift, uint64_t psi0_index,
                 uint64_t sea_mask, int rare_bit, double rare_z_const) {
  if (n < 1 || n > DSE_MAX_QUBITS) return fail(ctx, DSE_ERR_ARG, "n_qubits out of range 1..34");
  if (!field || !zz || !pair || !flip) return fail(ctx, DSE_ERR_ARG, "null coefficient table");
  const uint64_t dim = uint64_t(1) << n;
  if (psi0_index >= dim) return fail(ctx, DSE_ERR_ARG, "psi0_index >= 2^n");
  if ((sea_mask >> n) != 0) return fail(ctx, DSE_ERR_ARG, "sea_mask has bits >= n");
  if (rare_bit >= n || rare_bit < -1) return fail(ctx, DSE_ERR_ARG, "rare_bit out of range");
  p.n = n;
  p.field.assign(field, field + n);
  p.zz.assign(zz, zz + size_t(n) * n);
  p.pair.assign(pair, pair + size_t(n) * n);
  p.flip.assign(flip, flip + 4 * size_t(n));
  for (double v : p.field)
    if (!std::isfinite(v)) return fail(ctx, DSE_ERR_ARG, "non-finite field");
  for (double v : p.zz)
    if (!std::isfinite(v)) return fail(ctx, DSE_ERR_ARG, "non-finite zz");
  for (double v : p.pair)
    if (!std::isfinite(v)) return fail(ctx, DSE_ERR_ARG, "non-finite pair");
  for (int b = 0; b < n; ++b) {
    const double* f = &p.flip[4 * b];
    if (!(std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]) && std::isfinite(f[3])))
      return fail(ctx, DSE_ERR_ARG, "non-finite flip");
    const double scale = std::fabs(f[0]) + std::fabs(f[1]) + std::fabs(f[2]) + std::fabs(f[3]);
    if (std::fabs(f[0] - f[2]) > 1e-12 * scale || std::fabs(f[1] + f[3]) > 1e-12 * scale)
      return fail(ctx, DSE_ERR_ARG, "flip coefficients are not Hermitian (need c1 = conj(c0))");
  }
  if (!std::isfinite(shift)) return fail(ctx, DSE_ERR_ARG, "non-finite shift");
  p.shift = shift;
  p.psi0 = psi0_index;
  p.sea_mask = sea_mask;
  p.rare_bit = rare_bit;
  p.rare_z = rare_z_const;
  p.n_local = n;
  dse_spectral_bounds(n, p.field.data(), p.zz.data(), p.pair.data(), p.flip.data(), shift, &p.e_min, &p.e_max);
  {  // diagonal 4, drive flip 8 (complex coefficient), pair 4 on the half of the rows where it acts
    double f = 4.0;
    for (int b = 0; b < n; ++b)
      if (p.flip[4 * b] != 0.0 || p.flip[4 * b + 1] != 0.0) f += 8.0;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j)
        if (p.pair[i * n + j] != 0.0) f += 2.0;
    p.flops_per_amp = f;
  }
  return DSE_OK;
}

}  // namespace

extern "C" {

int dse_add_problem(dse_ctx* ctx, int n, const double* field, const double* zz, const double* pair,
                    const double* flip, double shift, uint64_t psi0_index, uint64_t sea_mask,
                    int rare_bit, double rare_z_const) {
  if (!ctx) return DSE_ERR_ARG;
  HostProblem p;
  int rc = make_problem(ctx, p, n, field, zz, pair, flip, shift, psi0_index, sea_mask, rare_bit,
                        rare_z_const);
  if (rc) return rc;
  (void)hipSetDevice(ctx->device);
  (void)sync_all(ctx);
  free_device(ctx);  // device layout is rebuilt lazily
  ctx->probs.push_back(std::move(p));
  return (int)ctx->probs.size() - 1;
}

int dse_add_problem_sharded(dse_ctx* ctx, int n, const double* field, const double* zz,
                            const double* pair, const double* flip, double shift,
                            uint64_t psi0_index, uint64_t sea_mask, int rare_bit,
                            double rare_z_const, int shard_bits, int shard_rank) {
  if (!ctx) return DSE_ERR_ARG;
  if (shard_bits < 1 || shard_bits > kMaxShardBits)
    return fail(ctx, DSE_ERR_ARG, "shard_bits must be in 1..3");
  if (shard_rank < -1 || shard_rank >= (1 << shard_bits))
    return fail(ctx, DSE_ERR_ARG, "shard_rank out of range");
  HostProblem p;
  int rc = make_problem(ctx, p, n, field, zz, pair, flip, shift, psi0_index, sea_mask, rare_bit,
                        rare_z_const);
  if (rc) return rc;
  if (n - shard_bits < kMinTile + 1)
    return fail(ctx, DSE_ERR_ARG, "register too small to partition");
  if (shard_rank >= 0 && ((!ctx->comm && !ctx->xfn) || ctx->dist_world != (1 << shard_bits) ||
                          ctx->dist_rank != shard_rank))
    return fail(ctx, DSE_ERR_STATE, "dist shard needs dse_dist_init with world = 2^shard_bits "
                                    "and rank = shard_rank");
  p.shard_bits = shard_bits;
  p.n_local = n - shard_bits;
  (void)hipSetDevice(ctx->device);
  (void)sync_all(ctx);
  free_device(ctx);
  const int first = (int)ctx->probs.size();
  if (shard_rank >= 0) {
    p.shard_rank = shard_rank;
    p.dist = true;
    ctx->probs.push_back(std::move(p));
    return first;
  }
  for (int r = 0; r < (1 << shard_bits); ++r) {
    HostProblem q = p;
    q.shard_rank = r;
    q.group_first = first;
    ctx->probs.push_back(std::move(q));
  }
  return first;
}

int dse_dist_unique_id(unsigned char* id_out) {
  if (!id_out) return DSE_ERR_ARG;
  static_assert(sizeof(ncclUniqueId) == DSE_DIST_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return DSE_ERR_HIP;
  std::memcpy(id_out, &id, sizeof(id));
  return DSE_OK;
}

int dse_dist_init(dse_ctx* ctx, int rank, int world, const unsigned char* id) {
  if (!ctx || !id) return DSE_ERR_ARG;
  if (world < 2 || world > kMaxShards || (world & (world - 1)) || rank < 0 || rank >= world)
    return fail(ctx, DSE_ERR_ARG, "world must be 2, 4 or 8 and 0 <= rank < world");
  if (ctx->comm || ctx->xfn) return fail(ctx, DSE_ERR_STATE, "dse_dist_init called twice");
  HIPC(hipSetDevice(ctx->device));
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  const ncclResult_t r = ncclCommInitRank(&ctx->comm, world, uid, rank);
  if (r != ncclSuccess) {
    ctx->comm = nullptr;
    return fail(ctx, DSE_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  }
  ctx->dist_rank = rank;
  ctx->dist_world = world;
  return DSE_OK;
}

int dse_dist_init_exchange(dse_ctx* ctx, int rank, int world, dse_exchange_fn fn, void* user) {
  if (!ctx || !fn) return DSE_ERR_ARG;
  if (world < 2 || world > kMaxShards || (world & (world - 1)) || rank < 0 || rank >= world)
    return fail(ctx, DSE_ERR_ARG, "world must be 2, 4 or 8 and 0 <= rank < world");
  if (ctx->comm || ctx->xfn) return fail(ctx, DSE_ERR_STATE, "dse_dist_init called twice");
  ctx->xfn = fn;
  ctx->xuser = user;
  ctx->dist_rank = rank;
  ctx->dist_world = world;
  return DSE_OK;
}

int dse_wht_plan(int n_local, int shard_bits, int tile_bits, int max_bits, int32_t* groups_out) {
  if (!groups_out || (tile_bits != 12 && tile_bits != 13) || n_local < 1 || n_local > kWhtMaxQubits ||
      shard_bits < 0 || shard_bits > kMaxShardBits)
    return DSE_ERR_ARG;
  WhtProb w;
  std::memset(&w, 0, sizeof(w));
  const int mb = max_bits & 0xff;  // bits 8-15: the MID group's in-page bits (option wht_mid_inpage)
  const int gb = mb ? std::min(mb, tile_bits - 2) : tile_bits - 2;
  const int G = wht_layout(n_local, shard_bits, tile_bits, gb, w, (max_bits >> 8) & 0xff);
  for (int g = 0; g < G; ++g) {
    groups_out[g * 14] = w.grp[g].c;
    for (int q = 0; q < tile_bits; ++q) groups_out[g * 14 + 1 + q] = w.grp[g].pos[q];
  }
  return G;
}

int64_t dse_problem_dim(const dse_ctx* ctx, int problem) {
  if (!ctx || problem < 0 || problem >= (int)ctx->probs.size()) return DSE_ERR_ARG;
  const HostProblem& P = ctx->probs[problem];
  return int64_t(1) << (P.dist ? P.n_local : P.n);
}

int dse_num_problems(const dse_ctx* ctx) { return ctx ? (int)ctx->probs.size() : DSE_ERR_ARG; }

int dse_clear(dse_ctx* ctx) {
  if (!ctx) return DSE_ERR_ARG;
  (void)hipSetDevice(ctx->device);
  (void)sync_all(ctx);
  free_device(ctx);
  for (auto& p : ctx->probs) free_initial(p), free_overlap_refs(p), free_op_strings(p), free_sectors(p);  // the initial states, references, strings and sets go with their problems
  ctx->probs.clear();
  return DSE_OK;
}

}  // extern "C"

namespace {

// The problems a hook call on `problem` acts on: the whole loopback group for its shard 0, else
// the problem itself.  Host vectors are the whole register (group) or the local shard.
int hook_members(dse_ctx* ctx, int problem, int* first, int* count) {
  if (problem < 0 || problem >= (int)ctx->probs.size()) return fail(ctx, DSE_ERR_ARG, "bad problem id");
  const HostProblem& P = ctx->probs[problem];
  *first = problem;
  *count = 1;
  if (P.shard_bits > 0 && !P.dist) {
    if (P.shard_rank != 0) return fail(ctx, DSE_ERR_ARG, "use shard 0 of a partitioned register");
    *count = 1 << P.shard_bits;
  }
  return DSE_OK;
}

// buf[1] = H buf[0] for the members [first, first + count) of one register (the engine that
// evolves it: Walsh-Hadamard passes or the step kernels; dist shards exchange first).
int apply_members(dse_ctx* ctx, int first, int count, hipStream_t st) {
  int rc;
  if ((rc = ensure_wht(ctx))) return rc;
  if (ctx->probs[first].wht_groups) {  // all members alike
    const HostProblem& P0 = ctx->probs[first];
    std::vector<std::pair<const int2*, int>> segs;
    for (int i = 0; i < count; ++i) segs.push_back({ctx->probs[first + i].d_items, (int)ctx->probs[first + i].n_tiles});
    std::vector<int> regs;
    if (P0.shard_bits > 0) regs.push_back(first);
    return wht_run(ctx, P0.L, P0.wht_groups, segs, regs, false, MODE_APPLY, 0, 0, 0, st);
  }
  if (ctx->probs[first].dist && (rc = dist_exchange(ctx, 0, 0, st))) return rc;
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    HIPC(launch_step(P.L, MODE_APPLY, ctx->d_probs, P.d_items, (int)P.n_tiles, 0, 0, 0, st));
  }
  return DSE_OK;
}

// ---- dense eigen-propagator engine (dse_dense.h) ------------------------------------------
// A register qualifies when it is whole (not partitioned), holds at most kDenseMaxQubits qubits
// and its drive coefficients are all purely imaginary (H' = D H D^dagger is real) or all real.
bool dense_eligible(const HostProblem& P) {
  if (P.shard_bits != 0 || P.n_local > kDenseMaxQubits) return false;
  if (P.imag) return true;
  for (int b = 0; b < P.n; ++b)
    if (P.flip[4 * b + 1] != 0.0 || P.flip[4 * b + 3] != 0.0) return false;
  return true;
}

// eig_impl 1 from 2^11 amplitudes: eig_sym_lower (rocSOLVER's tridiagonalisation below 2^13, the
// half-matrix one above; dstedc; the 256-reflector back-transformation) against dsyevd measured
// 0.46 vs 0.68 s at 2^13, 2.35 vs 4.12 s at 2^14 (profiles/r03/sytrd_probe.jsonl,
// profiles/r03/ab/sytrd_column_kernels_ab.jsonl)
constexpr size_t kEigHalfMinDim = 2048;
// eig_impl 1 from 2^13: eig_sym_2stage (dse_eig2.hip: band reduction, bulge chase, dstedc, Q2, Q1)
// measured 1.43 s against eig_sym_lower's 2.25 s at 2^14, 0.428 against 0.430 s at 2^13
// (profiles/r04/eig_one_vs_two_stage.jsonl); an N = 14 point of the 30 s grid (two 2^14 registers,
// one 2^13, three solver streams) 3.46-3.75 s with the 2^13 one two-stage against 3.62-3.72 s
// one-stage (profiles/r04/eig_impl_point_ab.jsonl).  Per-register output GEMMs (a register's outputs
// as soon as it is solved, instead of a job's) measured 3.66-3.77 s against 3.45-3.62 s and were
// dropped (profiles/r04/eig_point_outputs_per_register.jsonl).
constexpr size_t kEig2MinDim = 8192;

// The dimensions from which option eig_impl sends a register to eig_sym_lower (half_min) and, of
// those, to eig_sym_2stage (two_min); dsyevd below (SIZE_MAX: never)
struct EigThresholds {
  size_t half_min, two_min;
};
EigThresholds eig_thresholds(int eig_impl) {
  return {eig_impl == 1 ? kEigHalfMinDim : (eig_impl == 2 || eig_impl == 3) ? (size_t)1024 : SIZE_MAX,
          eig_impl == 1 ? kEig2MinDim : eig_impl == 3 ? (size_t)1024 : SIZE_MAX};
}

// Seconds of device time, by the measured rates: the Chebyshev propagator at ~15 TF/s of its
// algorithmic FP64 work (the N = 14 bench runs at 16.5 chip-level) with ~25 extra terms per
// output interval, against one eigendecomposition plus the Psi' GEMM at ~40 TF/s and the
// observable pass.  The eigendecomposition: dsyevd (profiles/r03/probe.jsonl: 0.15 / 0.68 / 4.1 s
// at dim 4096 / 8192 / 16384, 3 ms for 39 registers of dim 128 together: 6.4e-13 dim^3 + 4.9e-9
// dim^2, + 20 ms from dim 1024 up), or with eig_impl from 2^11 eig_sym_lower (0.13 / 0.46 / 2.35
// s: 2.96e-13 dim^3 + 3.73e-9 dim^2 + 0.047).  The long reference grid (30 s, 20 000 outputs)
// goes dense at every register size; the 1 ms head-to-head grid at N = 14 and config 2 (N = 12,
// 2 ms) stay on Chebyshev.
bool dense_cheaper(const HostProblem& P, const double* t, int n_t, int eig_impl) {
  if (n_t < 2) return false;
  const double dim = std::ldexp(1.0, P.n_local);
  const double alpha = 0.5 * (P.e_max - P.e_min);
  const double terms = alpha * (t[n_t - 1] - t[0]) + 25.0 * (n_t - 1);
  const double cheb = terms * dim * (P.flops_per_amp > 0 ? P.flops_per_amp : 300.0) / 15e12;
  const size_t d = (size_t)dim;
  const auto [half_min, two_min] = eig_thresholds(eig_impl);  // the solver eig_impl takes for this size
  double eig = d >= half_min ? 0.047 + 2.96e-13 * dim * dim * dim + 3.73e-9 * dim * dim
                             : 1e-4 + 6.4e-13 * dim * dim * dim + 4.9e-9 * dim * dim + (dim >= 1024 ? 2e-2 : 0.0);
  if (d >= two_min && dim >= 16384.0) eig *= 0.61;  // two-stage: 1.43 vs 2.35 s at 2^14 (level at 2^13)
  const double dense = eig + 4.0 * dim * dim * n_t / 40e12 + (double)n_t * dim * P.n_local * 32.0 / 2e12;
  return dense < cheb;
}

struct DevArena {  // device allocations of one dense_run, freed on every exit path
  std::vector<void*> ptrs;
  ~DevArena() { free_all(); }
  void free_all() {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
  template <typename T>
  T* get(size_t count) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return static_cast<T*>(p);
  }
};

// Every problem with P.dn: H' built on the device, diagonalised (rocSOLVER dsyevd, batched for
// registers of equal size below 2^10 amplitudes, one call per register above), outputs in blocks of
// TB times as Psi' = V [cos | -sin] (rocBLAS dgemm_strided_batched), observables and the final
// state from Psi'.  Work proceeds in rounds that fit 60% of the free device memory: every job
// (registers of one size) of a round is built, then all its eigendecompositions run on up to
// eig_streams solver streams at once (largest first, across sizes), then the output GEMMs.
// Blocking; writes obs_out.

struct DenseJob {  // registers of one size, built, solved and output together
  int n = 0, cnt = 0, TB = 1;
  size_t dim = 0, pstride = 0;
  double per = 0.0;       // modelled device bytes per register
  std::vector<int> list;  // problem indices
  DevArena ba;
  double *V = nullptr, *lam = nullptr, *lam_lo = nullptr, *E = nullptr, *Pm = nullptr, *Psi = nullptr, *obs = nullptr;
  double* diag_dd = nullptr;
  double* fam[kNumObsFamilies] = {};  // enabled families: [cnt][n_t][stride(n)] raw sums
  double* c = nullptr;  // custom psi(t0): [cnt][2 dim] projected coefficients (else not allocated)
  double* tabs = nullptr;
  rocblas_int* info = nullptr;
  DenseProb* d_desc = nullptr;
};

// half-matrix eigensolver scratch of one solver stream: a copy of H' (the solver's A; V receives the
// eigenvectors), tau and the tridiagonalisation workspace
struct EigScratch {
  double *A = nullptr, *tau = nullptr, *work = nullptr;
};

// What one dense_run holds across its rounds
struct DenseRun {
  const double* t = nullptr;  // dse_evolve's arguments
  int n_t = 0;
  double* obs_out = nullptr;
  std::vector<int> order;  // dense problems, by register size
  size_t idx = 0;          // the first of them not yet in a round
  hipStream_t st = nullptr;  // dense_stream
  DevArena arena;
  std::vector<double> tau;  // t - t[0], and its device copy
  double* d_tau = nullptr;
  // the non-uniform FFT's grid and device buffers (sized for the largest eligible register), or none
  NufftGrid ngrid;
  NufftScratch nscr;
  DevArena nufft_arena;
  bool use_nufft = false;
  // solver scratch per solver stream, sized for the largest such register so far; kept across rounds
  std::unique_ptr<DevArena> scr_arena;
  std::vector<EigScratch> scr;
  size_t scr_dim = 0, scr_work = 0;
  double out_ms = 0.0, eig_ms = 0.0;
};

struct DenseTask {
  DenseJob* j;
  int i;  // register within the job; -1: the whole job, batched
};

// One round: the jobs that fit 60% of the free memory, their eigendecompositions as tasks over K
// solver streams, and the queue between the workers and the output stage
struct DenseRound {
  std::vector<std::unique_ptr<DenseJob>> jobs;
  std::vector<DenseTask> tasks;
  int K = 1;
  EigThresholds thr{SIZE_MAX, SIZE_MAX};  // eig_thresholds of the option; half_min SIZE_MAX without scratch
  std::atomic<size_t> next{0};
  std::atomic<bool> abort_all{false};
  std::vector<rocblas_status> wst;  // per worker: the first failure
  std::vector<int> wrc;
  std::vector<hipError_t> werr;
  std::mutex qm;
  std::condition_variable qcv;
  std::deque<DenseJob*> ready;       // jobs whose registers are all solved: their outputs next
  std::map<DenseJob*, int> pending;  // per job: its registers not yet solved
  int workers_left = 0;
  std::chrono::steady_clock::time_point e0, e1;  // the solves: from the first task to the last worker's end
};

std::vector<int> dense_order(const dse_ctx* ctx) {  // the dense problems by register size, else by index
  std::vector<int> order;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi)
    if (ctx->probs[pi].dn) order.push_back((int)pi);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ctx->probs[a].n_local < ctx->probs[b].n_local; });
  return order;
}

// dense_stream, the rocBLAS handle on it, and the output times on the device
int dense_setup_stream(dse_ctx* ctx, DenseRun& R) {
  if (!ctx->dense_stream) HIPC(hipStreamCreateWithFlags(&ctx->dense_stream, hipStreamNonBlocking));
  if (!ctx->blas && rocblas_create_handle(&ctx->blas) != rocblas_status_success)
    return fail(ctx, DSE_ERR_HIP, "rocblas_create_handle failed");
  R.st = ctx->dense_stream;
  if (rocblas_set_stream(ctx->blas, R.st) != rocblas_status_success)
    return fail(ctx, DSE_ERR_HIP, "rocblas_set_stream failed");
  R.tau.resize(R.n_t);
  for (int i = 0; i < R.n_t; ++i) R.tau[i] = R.t[i] - R.t[0];
  R.d_tau = R.arena.get<double>(R.n_t);
  if (!R.d_tau) return fail(ctx, DSE_ERR_OOM, "dense engine: allocation failed");
  HIPC(hipMemcpyAsync(R.d_tau, R.tau.data(), R.n_t * sizeof(double), hipMemcpyHostToDevice, R.st));
  return DSE_OK;
}

// use_nufft with its grid and buffers when the option, the grid and the memory allow (else the GEMM outputs)
int dense_setup_nufft(dse_ctx* ctx, DenseRun& R) {
  const int n_t = R.n_t;
  ctx->nufft_problems = 0;
  if (!(ctx->dense_nufft && (ctx->dense_nufft == 2 || n_t >= kNufftMinOutputs))) return DSE_OK;
  size_t nmax = 0;
  double lam_max = 0.0;
  for (int pi : R.order) {
    const HostProblem& P = ctx->probs[pi];
    if ((size_t(1) << P.n_local) < (size_t)kNufftMinDim && ctx->dense_nufft != 2) continue;
    nmax = std::max(nmax, size_t(1) << P.n_local);
    lam_max = std::max({lam_max, std::fabs(P.e_min - P.shift), std::fabs(P.e_max - P.shift)});
  }
  if (!nmax || !nufft_grid(R.tau.data(), n_t, lam_max, R.ngrid)) return DSE_OK;
  NufftScratch& nscr = R.nscr;
  nscr.U = R.nufft_arena.get<double2>((size_t)R.ngrid.M * nmax);
  nscr.U2 = R.nufft_arena.get<double2>((size_t)R.ngrid.M * nmax);
  nscr.c = R.nufft_arena.get<double>(nmax);
  nscr.off = R.nufft_arena.get<int>((size_t)R.ngrid.M + 1);
  nscr.nnz_cap = nmax * (size_t)(kNufftW + 2);
  nscr.src = R.nufft_arena.get<int>(nscr.nnz_cap);
  nscr.wt = R.nufft_arena.get<double>(4 * nscr.nnz_cap);
  nscr.scale = R.nufft_arena.get<double>(n_t);
  nscr.delta = R.nufft_arena.get<double>(n_t);
  R.use_nufft = nscr.U && nscr.U2 && nscr.c && nscr.off && nscr.src && nscr.wt && nscr.scale && nscr.delta;
  if (R.use_nufft) {
    HIPC(hipMemcpyAsync(nscr.scale, R.ngrid.scale.data(), n_t * sizeof(double), hipMemcpyHostToDevice, R.st));
    HIPC(hipMemcpyAsync(nscr.delta, R.ngrid.delta.data(), n_t * sizeof(double), hipMemcpyHostToDevice, R.st));
    HIPC(hipStreamSynchronize(R.st));
  } else {  // no room: the GEMM outputs
    (void)hipGetLastError();
    R.nufft_arena.free_all();
  }
  return DSE_OK;
}

// The next job: the registers of R.order[R.idx]'s size that fit `room` bytes (at least one when the
// round is still empty), with its device buffers.  J stays null when the round is full: no room by the
// model, or an allocation failed beside earlier jobs (the register waits for the next round).
int dense_alloc_job(dse_ctx* ctx, const DenseRun& R, double room, bool round_empty, std::unique_ptr<DenseJob>& J) {
  const int n = ctx->probs[R.order[R.idx]].n_local, n_t = R.n_t;
  const size_t dim = size_t(1) << n;
  // outputs per block: P and Psi' of a problem take 2 x dim x 2 TB doubles (<= 256 MiB each)
  const int TB = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_t, (size_t(256) << 20) / (16 * dim)));
  const size_t pstride = dim * 2 * (size_t)TB;
  size_t fS[kNumObsFamilies] = {}, fsum = 0;  // the enabled families' sums per output
  for (ObsFamily f : kObsLaunchOrder)
    if (ctx->fam[f].on) fsum += fS[f] = (size_t)kObsFamilies[f].stride(ctx, n);
  const double per = (double)((dim * dim + 2 * pstride + 5 * dim + (size_t)n_t * (8 + fsum) + 2 * n * n + 4 * n) * sizeof(double));
  size_t same = 0;
  while (R.idx + same < R.order.size() && ctx->probs[R.order[R.idx + same]].n_local == n) ++same;
  size_t cnt = (size_t)std::max(0.0, room / per);
  if (cnt == 0 && !round_empty) return DSE_OK;
  cnt = std::max<size_t>(1, std::min(cnt, same));
  J = std::make_unique<DenseJob>();
  J->n = n, J->dim = dim, J->TB = TB, J->pstride = pstride, J->cnt = (int)cnt, J->per = per;
  J->list.assign(R.order.begin() + R.idx, R.order.begin() + R.idx + cnt);
  DevArena& ba = J->ba;
  J->V = ba.get<double>(dim * dim * cnt);
  J->lam = ba.get<double>(dim * cnt);
  J->lam_lo = ba.get<double>(dim * cnt);
  J->diag_dd = ba.get<double>(2 * dim * cnt);
  J->E = ba.get<double>(dim * cnt);
  J->info = ba.get<rocblas_int>(cnt);
  J->Pm = ba.get<double>(pstride * cnt);
  J->Psi = ba.get<double>(pstride * cnt);
  J->obs = ba.get<double>((size_t)n_t * 8 * cnt);
  for (ObsFamily f : kObsLaunchOrder)
    if (fS[f]) J->fam[f] = ba.get<double>((size_t)n_t * fS[f] * cnt);
  bool any_custom = false;
  for (size_t i = 0; i < cnt; ++i) any_custom = any_custom || ctx->probs[J->list[i]].init_kind != 0;
  bool ok = !any_custom || (J->c = ba.get<double>(2 * dim * cnt));
  if (ok) {
    J->tabs = ba.get<double>((size_t)(2 * n * n + 5 * n) * cnt);
    J->d_desc = ba.get<DenseProb>(cnt);
  }
  ok = ok && J->V && J->lam && J->lam_lo && J->diag_dd && J->E && J->info && J->Pm && J->Psi && J->obs && J->tabs &&
       J->d_desc;
  for (ObsFamily f : kObsLaunchOrder) ok = ok && !(fS[f] && !J->fam[f]);
  if (ok) return DSE_OK;
  J.reset();
  if (!round_empty) return DSE_OK;
  return fail(ctx, DSE_ERR_OOM, "dense engine: allocation failed (dim " + std::to_string(dim) + ")");
}


// The job's tables and descriptors on the device, and H' of its registers in V
int dense_fill_job(dse_ctx* ctx, const DenseRun& R, DenseJob& J) {
  const int n = J.n, n_t = R.n_t;
  const size_t dim = J.dim, cnt = (size_t)J.cnt, tsz = (size_t)(2 * n * n + 5 * n);
  std::vector<double> htabs(tsz * cnt, 0.0);
  std::vector<DenseProb> desc(cnt);
  for (size_t i = 0; i < cnt; ++i) {
    const HostProblem& P = ctx->probs[J.list[i]];
    double* h = htabs.data() + tsz * i;
    std::copy(P.field.begin(), P.field.begin() + n, h);
    std::copy(P.zz.begin(), P.zz.begin() + n * n, h + n);
    std::copy(P.pair.begin(), P.pair.begin() + n * n, h + n + n * n);
    std::copy(P.flip.begin(), P.flip.begin() + 4 * n, h + n + 2 * n * n);
    double* d = J.tabs + tsz * i;
    DenseProb& D = desc[i];
    D.n = n;
    D.rot = P.imag ? 1 : 0;
    D.sea_mask = P.sea_mask;
    D.rare_bit = P.rare_bit;
    D.n_sea = __builtin_popcountll(P.sea_mask);
    D.x0 = P.init_kind ? 0 : P.psi0;  // custom psi(t0): the whole phase i^|x| is in phi0
    if (P.init_kind) {             // (buf[0] holds psi(t0) until k_dense_final overwrites it)
      D.init = P.buf[0];
      D.c = J.c + 2 * dim * i;
    }
    D.shift = P.shift;
    D.field = d;
    D.zz = d + n;
    D.pair = d + n + n * n;
    D.flip = d + n + 2 * n * n;
    D.V = J.V + dim * dim * i;
    D.lam = J.lam + dim * i;
    D.lam_lo = J.lam_lo + dim * i;
    D.diag_dd = J.diag_dd + 2 * dim * i;
    D.refine = ctx->dense_refine;
    D.obs = J.obs + (size_t)n_t * 8 * i;
    D.final_state = P.buf[0];
    for (ObsFamily f : kObsLaunchOrder)
      D.*kObsFamilies[f].dense_out = J.fam[f] ? J.fam[f] + (size_t)n_t * kObsFamilies[f].stride(ctx, n) * i : nullptr;
    D.ovl_refs = P.d_ovl_tab;
    D.ovl_k = P.ovl_k();
    D.tau = R.d_tau;
    D.str_tab = P.d_str_tab;
    D.str_k = P.str_k();
    D.sec_tab = P.d_sec_tab;
    D.sec_k = P.sec_k();
  }
  hipStream_t st = R.st;
  HIPC(hipMemcpyAsync(J.tabs, htabs.data(), htabs.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(J.d_desc, desc.data(), desc.size() * sizeof(DenseProb), hipMemcpyHostToDevice, st));
  HIPC(hipMemsetAsync(J.V, 0, dim * dim * cnt * sizeof(double), st));
  HIPC(launch_dense_h(J.d_desc, (int)cnt, (int)dim, st));
  HIPC(hipStreamSynchronize(st));  // the host tables may go
  return DSE_OK;
}

// The round's eigendecompositions: one task per large register, one batched task per job of small
// ones, largest first
void dense_list_tasks(DenseRound& Rd) {
  for (auto& J : Rd.jobs) {
    if (J->dim >= 1024)
      for (int i = 0; i < J->cnt; ++i) Rd.tasks.push_back({J.get(), i});
    else
      Rd.tasks.push_back({J.get(), -1});
  }
  std::stable_sort(Rd.tasks.begin(), Rd.tasks.end(),
                   [](const DenseTask& x, const DenseTask& y) { return x.j->dim > y.j->dim; });
  for (const DenseTask& T : Rd.tasks) Rd.pending[T.j] += 1;
}

// K solver streams, each with a rocBLAS handle (kept in the context)
int dense_ensure_solver_streams(dse_ctx* ctx, int K) {
  while ((int)ctx->eig_h.size() < K) {
    hipStream_t es = nullptr;
    rocblas_handle eh = nullptr;
    HIPC(hipStreamCreateWithFlags(&es, hipStreamNonBlocking));
    if (rocblas_create_handle(&eh) != rocblas_status_success || rocblas_set_stream(eh, es) != rocblas_status_success) {
      if (eh) (void)rocblas_destroy_handle(eh);
      (void)hipStreamDestroy(es);
      return fail(ctx, DSE_ERR_HIP, "rocblas handle for the eigensolver streams failed");
    }
    ctx->eig_st.push_back(es);
    ctx->eig_h.push_back(eh);
  }
  return DSE_OK;
}

// The half-matrix and two-stage solvers' scratch per solver stream, sized for the round's largest such
// register.  Without room beside the round's jobs the round solves with dsyevd in place (half_min).
void dense_ensure_scratch(DenseRun& R, DenseRound& Rd) {
  size_t half_dim = 0, two_dim = 0;
  for (const DenseTask& T : Rd.tasks)
    if (T.i >= 0 && T.j->dim >= Rd.thr.half_min) {
      half_dim = std::max(half_dim, T.j->dim);
      if (T.j->dim >= Rd.thr.two_min) two_dim = std::max(two_dim, T.j->dim);
    }
  const size_t work_b = std::max(sytrd_workspace((int)half_dim), two_dim ? eig2_workspace((int)two_dim) : (size_t)0);
  if (half_dim <= R.scr_dim && work_b <= R.scr_work) return;
  R.scr.clear();
  R.scr_arena.reset(new DevArena);
  R.scr_dim = 0, R.scr_work = 0;
  for (int w = 0; w < Rd.K; ++w) {
    EigScratch S;
    S.A = R.scr_arena->get<double>(half_dim * half_dim);
    S.tau = R.scr_arena->get<double>(half_dim);
    S.work = R.scr_arena->get<double>(work_b / sizeof(double) + 1);
    if (!S.A || !S.tau || !S.work) break;
    R.scr.push_back(S);
  }
  if ((int)R.scr.size() == Rd.K) {
    R.scr_dim = half_dim, R.scr_work = work_b;
  } else {
    (void)hipGetLastError();
    R.scr.clear();
    R.scr_arena.reset();
    Rd.thr.half_min = SIZE_MAX;
  }
}

// Task T on solver stream w, to the end of its stream's work: the two-stage, the half-matrix or
// rocSOLVER's solver by the register's size (the batched dsyevd for a whole job of small ones).
// False: a failure, left in werr / wst / wrc[w].
bool dense_solve_task(dse_ctx* ctx, const DenseRun& R, DenseRound& Rd, int w, const DenseTask& T) {
  DenseJob& J = *T.j;
  hipStream_t es = ctx->eig_st[w];
  rocblas_handle eh = ctx->eig_h[w];
  hipError_t& err = Rd.werr[w];
  rocblas_status& rst = Rd.wst[w];
  int& rc = Rd.wrc[w];
  const rocblas_int dim = (rocblas_int)J.dim;
  if (T.i >= 0 && J.dim >= Rd.thr.half_min) {
    const size_t i = (size_t)T.i;
    const EigScratch& S = R.scr[w];
    double* Vi = J.V + J.dim * J.dim * i;
    err = hipMemcpyAsync(S.A, Vi, J.dim * J.dim * sizeof(double), hipMemcpyDeviceToDevice, es);
    if (err == hipSuccess && J.dim >= Rd.thr.two_min) {
      rc = eig_sym_2stage(eh, es, dim, S.A, dim, J.lam + J.dim * i, Vi, dim, J.E + J.dim * i, S.work, J.info + i,
                          ctx->n_cu, ctx->eig_spin);
      if (rc == kEig2PollTimeout) {  // a poll gave up (workgroups not co-resident): H' again, dsyevd
        ctx->eig_fallbacks++;
        rc = 0;
        err = hipMemsetAsync(Vi, 0, J.dim * J.dim * sizeof(double), es);
        if (err == hipSuccess) err = launch_dense_h(J.d_desc + i, 1, (int)J.dim, es);
        if (err == hipSuccess)
          rst = rocsolver_dsyevd(eh, rocblas_evect_original, rocblas_fill_upper, dim, Vi, dim, J.lam + J.dim * i,
                                 J.E + J.dim * i, J.info + i);
      }
    } else if (err == hipSuccess) {
      rc = eig_sym_lower(eh, es, dim, S.A, dim, J.lam + J.dim * i, Vi, dim, J.E + J.dim * i, S.tau, S.work, J.info + i);
    }
  } else if (T.i >= 0) {
    const size_t i = (size_t)T.i;
    rst = rocsolver_dsyevd(eh, rocblas_evect_original, rocblas_fill_upper, dim, J.V + J.dim * J.dim * i, dim,
                           J.lam + J.dim * i, J.E + J.dim * i, J.info + i);
  } else {
    rst = rocsolver_dsyevd_strided_batched(eh, rocblas_evect_original, rocblas_fill_upper, dim, J.V, dim,
                                           (rocblas_stride)(J.dim * J.dim), J.lam, (rocblas_stride)J.dim, J.E,
                                           (rocblas_stride)J.dim, J.info, J.cnt);
  }
  const hipError_t se = hipStreamSynchronize(es);
  if (err == hipSuccess) err = se;
  return err == hipSuccess && rst == rocblas_status_success && rc == 0;
}

// Solver worker w: tasks largest first; a job whose last register is solved goes to the output queue
void dense_worker(dse_ctx* ctx, const DenseRun& R, DenseRound& Rd, int w) {
  for (size_t ti = Rd.next++; ti < Rd.tasks.size() && !Rd.abort_all; ti = Rd.next++) {
    const DenseTask& T = Rd.tasks[ti];
    if (!dense_solve_task(ctx, R, Rd, w, T)) {
      Rd.abort_all = true;
      break;
    }
    std::lock_guard<std::mutex> lk(Rd.qm);
    if (--Rd.pending[T.j] == 0) {
      Rd.ready.push_back(T.j);
      Rd.qcv.notify_one();
    }
  }
  std::lock_guard<std::mutex> lk(Rd.qm);
  if (--Rd.workers_left == 0) Rd.e1 = std::chrono::steady_clock::now();
  Rd.qcv.notify_one();
}

// The aggregates, then every family the context records (kObsLaunchOrder), of the tb columns `cols` of
// the n-qubit registers d[0 .. count) into rows t0 .. t0 + tb of their records: the dense engine's
// blocks on both paths and matrix mode's states.  A family is launched iff the context records it
// (fam[f].on), and that is when d[p].*dense_out is set: dense_alloc_job gives a job the buffer of every
// family that is on or fails, matrix_run does the same in its arena; the site and pair kernels write
// through that pointer unchecked.
hipError_t launch_dense_outputs(const dse_ctx* ctx, const DenseProb* d, int count, int n, const DenseCols& cols, int tb,
                                int t0, hipStream_t st) {
  const int dim = 1 << n;
  hipError_t e = launch_dense_obs(d, count, dim, cols, tb, t0, st);
  for (ObsFamily f : kObsLaunchOrder)
    if (e == hipSuccess && ctx->fam[f].on)
      e = kObsFamilies[f].launch_dense(d, count, dim, cols, tb, t0, kObsFamilies[f].stride(ctx, n), st);
  return e;
}

// Job J's outputs by the non-uniform FFT: per register, Psi' interleaved, the observables per block
int dense_outputs_nufft(dse_ctx* ctx, DenseRun& R, DenseJob& J) {
  const int n_t = R.n_t;
  const size_t dim = J.dim;
  hipStream_t st = R.st;
  const DenseCols cols = DenseCols::interleaved(J.Psi, (int)dim);
  for (int i = 0; i < J.cnt; ++i) {
    const DenseProb* di = J.d_desc + i;
    auto per_block = [&](int tb0, int tb) -> int {
      if (launch_dense_outputs(ctx, di, 1, J.n, cols, tb, tb0, st) != hipSuccess) return -1;
      if (tb0 + tb == n_t && launch_dense_final(di, 1, (int)dim, cols, tb, R.tau[n_t - 1], st) != hipSuccess)
        return -1;
      return 0;
    };
    const HostProblem& P = ctx->probs[J.list[i]];
    // the low parts exist only after k_dense_rq: without the refinement none are passed (zero)
    const double* lo = ctx->dense_refine ? J.lam_lo + dim * i : nullptr;
    const int rc = nufft_outputs(ctx->nufft, st, R.ngrid, R.nscr, J.V + dim * dim * i, J.lam + dim * i, lo, P.psi0,
                                 (int)dim, J.Psi, J.TB, per_block, P.init_kind ? J.c + 2 * dim * i : nullptr);
    if (rc) return fail(ctx, DSE_ERR_HIP, "dense engine: non-uniform FFT outputs failed (" + std::to_string(rc) + ")");
    ctx->nufft_problems++;
  }
  return DSE_OK;
}

// Job J's outputs in blocks of TB times: Psi' = V [cos | -sin] for all its registers at once
int dense_outputs_gemm(dse_ctx* ctx, DenseRun& R, DenseJob& J) {
  const int n_t = R.n_t, cnt = J.cnt;
  const size_t dim = J.dim, pstride = J.pstride;
  const DenseProb* desc = J.d_desc;
  hipStream_t st = R.st;
  const double one = 1.0, zero = 0.0;
  for (int tb0 = 0; tb0 < n_t; tb0 += J.TB) {
    const int tb = std::min(J.TB, n_t - tb0);
    HIPC(launch_dense_phase(desc, cnt, (int)dim, R.d_tau + tb0, tb, J.Pm, pstride, st));
    if (J.c) HIPC(launch_dense_phase_c(desc, cnt, (int)dim, R.d_tau + tb0, tb, J.Pm, pstride, st));
    const rocblas_status rs = rocblas_dgemm_strided_batched(
        ctx->blas, rocblas_operation_none, rocblas_operation_none, (rocblas_int)dim, 2 * tb, (rocblas_int)dim, &one,
        J.V, (rocblas_int)dim, (rocblas_stride)(dim * dim), J.Pm, (rocblas_int)dim, (rocblas_stride)pstride, &zero,
        J.Psi, (rocblas_int)dim, (rocblas_stride)pstride, cnt);
    if (rs != rocblas_status_success)
      return fail(ctx, DSE_ERR_HIP, "rocblas dgemm failed (status " + std::to_string((int)rs) + ")");
    const DenseCols cols = DenseCols::split(J.Psi, pstride, (int)dim, tb);
    HIPC(launch_dense_outputs(ctx, desc, cnt, J.n, cols, tb, tb0, st));
    if (tb0 + tb == n_t) HIPC(launch_dense_final(desc, cnt, (int)dim, cols, tb, R.tau[n_t - 1], st));
  }
  return DSE_OK;
}

// Job J's sums back on the host and normalised: the families into their stores, the aggregates into
// obs_out.  out_ms: the output stage since o0, up to the families' results.
int dense_read_back(dse_ctx* ctx, DenseRun& R, DenseJob& J, std::chrono::steady_clock::time_point o0) {
  const int n_t = R.n_t, cnt = J.cnt;
  hipStream_t st = R.st;
  std::vector<double> h((size_t)n_t * 8 * cnt);
  HIPC(hipMemcpyAsync(h.data(), J.obs, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  std::vector<double> hf[kNumObsFamilies];
  for (ObsFamily f : kObsLaunchOrder) {
    if (!J.fam[f]) continue;
    hf[f].resize((size_t)n_t * kObsFamilies[f].stride(ctx, J.n) * cnt);
    HIPC(hipMemcpyAsync(hf[f].data(), J.fam[f], hf[f].size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPC(hipStreamSynchronize(st));
  for (ObsFamily f : kObsReadbackOrder) {
    const size_t S = (size_t)kObsFamilies[f].stride(ctx, J.n);
    for (int i = 0; i < cnt && J.fam[f]; ++i)
      finish_family_outputs(ctx, f, (size_t)J.list[i], hf[f].data() + (size_t)i * n_t * S, S, n_t);
  }
  R.out_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - o0).count();
  for (int i = 0; i < cnt; ++i) {
    const int pi = J.list[i];
    for (int ti = 0; ti < n_t; ++ti)
      finish_obs(ctx->probs[pi], h.data() + ((size_t)i * n_t + ti) * 8, R.obs_out + (size_t)pi * DSE_N_OBS * n_t + ti,
                 (size_t)n_t);
  }
  return DSE_OK;
}

// The output stage of job J, every register of it: Psi' by the transform or the GEMM, observables and
// the final state from Psi', on dense_stream
int dense_outputs(dse_ctx* ctx, DenseRun& R, DenseJob& J) {
  hipStream_t st = R.st;
  std::vector<rocblas_int> hinfo(J.cnt);
  HIPC(hipMemcpyAsync(hinfo.data(), J.info, J.cnt * sizeof(rocblas_int), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  for (int i = 0; i < J.cnt; ++i)
    if (hinfo[i] != 0)
      return fail(ctx, DSE_ERR_CONVERGENCE, "dense engine: eigensolver did not converge (info " +
                                                std::to_string(hinfo[i]) + ")");
  const auto o0 = std::chrono::steady_clock::now();
  if (ctx->dense_refine) HIPC(launch_dense_rq(J.d_desc, J.cnt, (int)J.dim, st));
  if (J.c) HIPC(launch_dense_project(J.d_desc, J.cnt, (int)J.dim, st));  // c = V^T phi0 of the custom states
  const bool nufft = R.use_nufft && (J.dim >= (size_t)kNufftMinDim || ctx->dense_nufft == 2);
  if (int rc = nufft ? dense_outputs_nufft(ctx, R, J) : dense_outputs_gemm(ctx, R, J)) return rc;
  return dense_read_back(ctx, R, J, o0);
}

// One round's solves and outputs: K workers take the tasks, and this thread runs the output stage of
// each job as its last register is solved (dense_stream) while the other solves go on (outputs per
// register as each solve ends measured the same, profiles/r05/fullsweep_outputs_ab.jsonl)
int dense_run_round(dse_ctx* ctx, DenseRun& R, DenseRound& Rd) {
  const int K = Rd.K;
  Rd.wst.assign(K, rocblas_status_success);
  Rd.wrc.assign(K, 0);
  Rd.werr.assign(K, hipSuccess);
  Rd.workers_left = K;
  Rd.e1 = Rd.e0;
  std::vector<std::thread> th;
  for (int w = 0; w < K; ++w) th.emplace_back(dense_worker, ctx, std::cref(R), std::ref(Rd), w);
  int orc = DSE_OK;
  size_t done = 0;
  const size_t n_out_tasks = Rd.jobs.size();
  while (done < n_out_tasks) {
    DenseJob* J = nullptr;
    {
      std::unique_lock<std::mutex> lk(Rd.qm);
      Rd.qcv.wait(lk, [&] { return !Rd.ready.empty() || Rd.workers_left == 0; });
      if (Rd.ready.empty()) break;  // the workers stopped early: an error below
      J = Rd.ready.front();
      Rd.ready.pop_front();
    }
    orc = dense_outputs(ctx, R, *J);
    if (orc != DSE_OK) {
      Rd.abort_all = true;
      break;
    }
    ++done;
  }
  for (auto& x : th) x.join();
  if (orc != DSE_OK) return orc;
  for (int w = 0; w < K; ++w) {
    if (Rd.werr[w] != hipSuccess)
      return fail(ctx, DSE_ERR_HIP, std::string("eigensolver stream: ") + hipGetErrorString(Rd.werr[w]));
    if (Rd.wst[w] != rocblas_status_success)
      return fail(ctx, DSE_ERR_HIP, "rocsolver dsyevd failed (status " + std::to_string((int)Rd.wst[w]) + ")");
    if (Rd.wrc[w] != 0)
      return fail(ctx, DSE_ERR_HIP, "half-matrix eigensolver failed (step " + std::to_string(-Rd.wrc[w]) + ")");
  }
  if (done < n_out_tasks) return fail(ctx, DSE_ERR_HIP, "dense engine: eigensolver workers stopped early");
  R.eig_ms += std::chrono::duration<double, std::milli>(Rd.e1 - Rd.e0).count();
  return DSE_OK;
}

int dense_run(dse_ctx* ctx, const double* t, int n_t, double* obs_out, double* ms_all, double* ms_eig) {
  DenseRun R;
  R.t = t, R.n_t = n_t, R.obs_out = obs_out;
  R.order = dense_order(ctx);
  if (R.order.empty()) return DSE_OK;
  const auto c0 = std::chrono::steady_clock::now();
  int rc;
  if ((rc = dense_setup_stream(ctx, R)) || (rc = dense_setup_nufft(ctx, R))) return rc;
  while (R.idx < R.order.size()) {
    DenseRound Rd;  // jobs while 60% of the free memory lasts (at least one register)
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const double budget = 0.6 * (double)free_b;
    for (double used = 0.0; R.idx < R.order.size();) {
      std::unique_ptr<DenseJob> J;
      if ((rc = dense_alloc_job(ctx, R, budget - used, Rd.jobs.empty(), J))) return rc;
      if (!J) break;
      if ((rc = dense_fill_job(ctx, R, *J))) return rc;
      used += J->per * (double)J->cnt;
      R.idx += (size_t)J->cnt;
      Rd.jobs.push_back(std::move(J));
    }
    Rd.e0 = std::chrono::steady_clock::now();
    dense_list_tasks(Rd);
    Rd.K = std::max(1, std::min(ctx->eig_streams, (int)Rd.tasks.size()));
    if ((rc = dense_ensure_solver_streams(ctx, Rd.K))) return rc;
    Rd.thr = eig_thresholds(ctx->eig_impl);
    dense_ensure_scratch(R, Rd);
    if ((rc = dense_run_round(ctx, R, Rd))) return rc;
  }
  if (ms_all) *ms_all = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
  if (ms_eig) *ms_eig = R.eig_ms;
  ctx->dense_out_ms = R.out_ms;
  return DSE_OK;
}

// ---- propagator-matrix mode ----------------------------------------------------------------
// One evolution alone in a context runs its Chebyshev terms on one workgroup per tile: a chain of
// ~alpha t_final + 30 (n_t - 1) terms at ~11 us each on one CU (config 2, N = 12: ~9e3 terms,
// ~0.1 s) while the other 255 CUs idle.  On a uniform grid the whole evolution is psi_j =
// U^j psi_0 with U = exp(-iH dt): U's 2^n columns are independent Chebyshev evolutions over one
// interval (k_interval in column mode: 2^n workgroups, the whole chip), then the outputs are
// n_t - 1 dependent products psi_{j+1} = U psi_j (rocBLAS zgemv, HBM-bound) and one observable
// launch over all states.
bool matrix_eligible(const HostProblem& P, const double* t, int n_t, double* dt_out) {
  if (P.shard_bits != 0 || P.n_tiles != 1 || !interval_supported(P.L) || n_t < 17) return false;
  if (P.n_local > 13) return false;
  const double dt = (t[n_t - 1] - t[0]) / (n_t - 1);
  for (int i = 1; i < n_t; ++i)
    if (std::fabs((t[i] - t[i - 1]) - dt) > 1e-9 * dt) return false;
  *dt_out = dt;
  return true;
}

// seconds: the chain on one workgroup (~11.4 us per term at 2^12 amplitudes, linear in the tile)
// against the column build spread over the chip plus n_t - 1 matrix-vector products.  Real build
// (k_ucols, imaginary or real drives): ~10 us per term and workgroup at 2^12 amplitudes with two
// workgroups per CU (one at 2^13, LDS), products over the half matrix at ~5 TB/s plus ~5 us for the
// reduction launch; complex build (k_interval column mode): as the chain's terms, two workgroups
// per CU below 2^13, products over the whole matrix (zgemv) at ~3 TB/s.
// device bytes of matrix_run for register P on n_t outputs (U's stored tiles or columns, the
// states, the products' partials; the small tables are within the rounding)
double matrix_bytes(const HostProblem& P, int n_t) {
  const double dim = std::ldexp(1.0, P.n_local);
  const double nb = dim / kSymvBlock;
  const bool real = dense_eligible(P) && ucols_supported(P.L) && P.n_local == P.L;
  const double u = real ? nb * (nb + 1) / 2 * kSymvBlock * kSymvBlock : dim * dim;
  return 16.0 * (u + dim * n_t + (real ? nb * dim : 0.0)) + (1 << 20);
}

bool matrix_cheaper(const HostProblem& P, double dt, int n_t, int n_cu) {
  const double dim = std::ldexp(1.0, P.n_local);
  const double alpha = 0.5 * (P.e_max - P.e_min);
  const double z = alpha * dt;
  const double deg1 = z + 12.0 * std::cbrt(z + 1.0) + 20.0;
  const double t_term = 11.4e-6 * std::max(dim / 4096.0, 0.25);
  const double chain = (n_t - 1) * deg1 * t_term;
  const bool real = dense_eligible(P) && ucols_supported(P.L) && P.n_local == P.L;
  const double slots = (double)n_cu * (P.L < 13 ? 2.0 : 1.0);
  const double t_col = real ? 10e-6 * std::max(dim / 4096.0, 0.25) : t_term;
  const double build = std::ceil(dim / slots) * deg1 * t_col;
  const double chain_u = (n_t - 1) * (real ? dim * dim * 8.0 / 5e12 + 5e-6 : dim * dim * 16.0 / 3e12);
  return build + chain_u < chain;
}

int matrix_run(dse_ctx* ctx, int pi, const double* t, int n_t, double dt, double tol, double* obs_out,
               double* h_apps) {
  HostProblem& P = ctx->probs[pi];
  const int n = P.n_local;
  const size_t dim = size_t(1) << n;
  hipStream_t st = ctx->lanes[0].stream;
  // Chebyshev coefficients of one interval dt (one set, one output)
  const double alpha = std::max(0.5 * (P.e_max - P.e_min), 1e-300);
  const double beta = 0.5 * (P.e_max + P.e_min);
  std::vector<std::pair<double, double>> a;
  std::vector<double> J;
  int deg = 1, kmax = 0;
  {
    const int rc = cheb_series(alpha, beta, dt, tol, ctx->max_degree, &deg, &a, &kmax, &J);
    if (rc == DSE_ERR_CONVERGENCE) return fail(ctx, DSE_ERR_CONVERGENCE, "Chebyshev degree exceeds max_degree");
    if (rc != DSE_OK) return fail(ctx, DSE_ERR_ARG, "bessel failed");
  }
  // U's rotated form is symmetric when the drives are all imaginary (parity twist s_r s_c) or all
  // real: the column build runs in real arithmetic (k_ucols) and the products read the tiles on and
  // above the diagonal (k_symv); otherwise the complex column build and rocBLAS zgemv on the whole
  // column-major matrix
  const bool real_build = dense_eligible(P) && ucols_supported(P.L) && P.n_local == P.L;
  std::vector<double2> row(deg + 2, make_double2(0.0, 0.0));  // complex build: a_k
  std::vector<double> cf(deg + 1);                               // real build: (-1)^{k/2} c_k
  row[0] = make_double2((double)deg, 0.0);
  for (int k = 0; k <= deg; ++k) {
    const double ck = (k == 0 ? 1.0 : 2.0) * J[k];
    row[1 + k] = make_double2(a[k].first, a[k].second);
    cf[k] = ((k >> 1) & 1) ? -ck : ck;
  }
  // device buffers: kept in the context between calls (ctx->d_mx.p)
  const size_t nb = dim / kSymvBlock;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = align_up(off + std::max<size_t>(bytes, 1), 256);
    return o;
  };
  const size_t u_elems = real_build ? nb * (nb + 1) / 2 * kSymvBlock * kSymvBlock : dim * dim;
  const size_t oU = take(u_elems * sizeof(double2)), oS = take(dim * (size_t)n_t * sizeof(double2)),
               oPart = take(real_build ? nb * dim * sizeof(double2) : 0), oObs = take((size_t)n_t * 8 * sizeof(double)),
               oDesc = take(sizeof(DenseProb)), oProb = take(sizeof(DevProb)),
               oCoef = take(std::max(row.size() * sizeof(double2), cf.size() * sizeof(double))), oErr = take(sizeof(int)),
               oCnt = take(nb * sizeof(int));
  // the enabled observable families: their sums of the same states, kept with the mode's other buffers
  // (taken last and only with the option on: every other offset, and the size with it off, as before)
  size_t oFam[kNumObsFamilies] = {};
  for (ObsFamily f : kObsLaunchOrder)
    if (ctx->fam[f].on) oFam[f] = take((size_t)n_t * kObsFamilies[f].stride(ctx, n) * sizeof(double));
  if (int rc = ctx->d_mx.reserve(ctx, off, "propagator-matrix mode: allocation failed")) return rc;
  unsigned char* base = ctx->d_mx.p;
  double2* U = reinterpret_cast<double2*>(base + oU);     // tiles (real build) or columns: U e_c
  double2* S = reinterpret_cast<double2*>(base + oS);     // psi(t_j), consecutive
  double2* part = real_build ? reinterpret_cast<double2*>(base + oPart) : nullptr;
  double* d_obs = reinterpret_cast<double*>(base + oObs);
  DenseProb* d_desc = reinterpret_cast<DenseProb*>(base + oDesc);
  DevProb* d_p = reinterpret_cast<DevProb*>(base + oProb);
  int* d_err = reinterpret_cast<int*>(base + oErr);
  int* d_cnt = reinterpret_cast<int*>(base + oCnt);
  DevProb d = ctx->h_desc[pi];
  d.beta = beta;
  d.s1 = 1.0 / alpha;
  d.degree = deg;
  HIPC(hipMemsetAsync(d_err, 0, sizeof(int), st));
  HIPC(hipMemsetAsync(d_cnt, 0, nb * sizeof(int), st));
  DevArena ar;  // complex build only: the basis columns
  // HIP events: build | products | (observables), read back for dse_stats (matrix_*)
  hipEvent_t mev[3] = {nullptr, nullptr, nullptr};
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() {
      for (int i = 0; i < 3; ++i)
        if (e[i]) (void)hipEventDestroy(e[i]);
    }
  } mev_guard{mev};
  for (auto& e : mev) HIPC(hipEventCreate(&e));
  HIPC(hipEventRecord(mev[0], st));
  if (real_build) {
    double* d_cf = reinterpret_cast<double*>(base + oCoef);
    HIPC(hipMemcpyAsync(d_cf, cf.data(), cf.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_p, &d, sizeof(DevProb), hipMemcpyHostToDevice, st));
    HIPC(launch_ucols(P.L, d_p, d_cf, deg, P.imag ? 1 : 0, std::cos(-beta * dt), std::sin(-beta * dt), U, (int)dim,
                      0, (int)P.psi0, S + dim, st));
  } else {
    if (!ctx->blas && rocblas_create_handle(&ctx->blas) != rocblas_status_success)
      return fail(ctx, DSE_ERR_HIP, "rocblas_create_handle failed");
    if (rocblas_set_stream(ctx->blas, st) != rocblas_status_success)
      return fail(ctx, DSE_ERR_HIP, "rocblas_set_stream failed");
    double2* B0 = ar.get<double2>(dim * dim);  // columns: e_c, then scratch
    int2* d_items = ar.get<int2>(dim);
    BasisInit* d_init = ar.get<BasisInit>(dim);
    if (!B0 || !d_items || !d_init) return fail(ctx, DSE_ERR_OOM, "propagator-matrix mode: allocation failed");
    double2* d_row = reinterpret_cast<double2*>(base + oCoef);
    d.buf[0] = B0;
    d.buf[1] = B0;
    d.buf[2] = U;
    d.coef = d_row;
    d.kcap1 = deg + 1;
    d.n_acc = 1;
    d.xacc_q = 0;
    std::vector<int2> items(dim);
    std::vector<BasisInit> init(dim);
    for (size_t c = 0; c < dim; ++c) {
      items[c] = make_int2(0, (int)c);
      init[c].ptr = B0 + c * dim;
      init[c].n = dim;
      init[c].one_at = (int64_t)c;
    }
    HIPC(hipMemcpyAsync(d_row, row.data(), row.size() * sizeof(double2), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_p, &d, sizeof(DevProb), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_items, items.data(), dim * sizeof(int2), hipMemcpyHostToDevice, st));
    HIPC(hipMemcpyAsync(d_init, init.data(), dim * sizeof(BasisInit), hipMemcpyHostToDevice, st));
    HIPC(launch_basis_init(d_init, (int)dim, dim, st));
    HIPC(launch_interval(P.L, P.imag, d_p, d_items, (int)dim, 0, 0, 1, d_err, d_err, ctx->hk, st, (long)dim));
  }
  HIPC(hipEventRecord(mev[1], st));
  // psi_0 = e_x0, psi_1 = U e_x0 (column x0), psi_{j+1} = U psi_j.  A custom psi_0 (in buf[0], written
  // by dse_evolve's initialisation) has no column to copy: psi_1 = U psi_0 is the first product (the
  // real build still wrote column psi0_index into psi_1's place; that product overwrites it)
  const bool custom0 = P.init_kind != 0;
  if (custom0) {
    HIPC(hipMemcpyAsync(S, P.buf[0], dim * sizeof(double2), hipMemcpyDeviceToDevice, st));
  } else {
    HIPC(hipMemsetAsync(S, 0, dim * sizeof(double2), st));
    static const double2 one_c = {1.0, 0.0};
    HIPC(hipMemcpyAsync(S + P.psi0, &one_c, sizeof(double2), hipMemcpyHostToDevice, st));
    if (!real_build)  // (the real build wrote column x0 itself)
      HIPC(hipMemcpyAsync(S + dim, U + P.psi0 * dim, dim * sizeof(double2), hipMemcpyDeviceToDevice, st));
  }
  const rocblas_double_complex one(1.0, 0.0), zero(0.0, 0.0);
  const int j_first = custom0 ? 0 : 1;
  for (int j = j_first; j + 1 < n_t && real_build; ++j) {
    if (ctx->symv_fused) {
      HIPC(launch_symv(U, (int)dim, S + dim * j, part, P.imag ? 1 : 0, st, d_cnt, S + dim * (j + 1)));
    } else {
      HIPC(launch_symv(U, (int)dim, S + dim * j, part, P.imag ? 1 : 0, st));
      HIPC(launch_symv_reduce(part, (int)dim, S + dim * (j + 1), st));
    }
  }
  for (int j = j_first; j + 1 < n_t && !real_build; ++j) {
    const rocblas_status rs = rocblas_zgemv(ctx->blas, rocblas_operation_none, (rocblas_int)dim, (rocblas_int)dim,
                                            &one, reinterpret_cast<const rocblas_double_complex*>(U),
                                            (rocblas_int)dim,
                                            reinterpret_cast<const rocblas_double_complex*>(S + dim * j), 1,
                                            &zero, reinterpret_cast<rocblas_double_complex*>(S + dim * (j + 1)), 1);
    if (rs != rocblas_status_success)
      return fail(ctx, DSE_ERR_HIP, "rocblas zgemv failed (status " + std::to_string((int)rs) + ")");
  }
  HIPC(hipEventRecord(mev[2], st));
  DenseProb D = {};
  D.n = n;
  D.rot = 0;
  D.sea_mask = P.sea_mask;
  D.rare_bit = P.rare_bit;
  D.n_sea = __builtin_popcountll(P.sea_mask);
  D.x0 = P.psi0;
  D.obs = d_obs;
  for (ObsFamily f : kObsLaunchOrder)
    if (ctx->fam[f].on) D.*kObsFamilies[f].dense_out = reinterpret_cast<double*>(base + oFam[f]);
  D.ovl_refs = P.d_ovl_tab;  // (tau null: the states are in the computational frame, the shift's phase in U)
  D.ovl_k = P.ovl_k();
  D.str_tab = P.d_str_tab;
  D.str_k = P.str_k();
  D.sec_tab = P.d_sec_tab;
  D.sec_k = P.sec_k();
  HIPC(hipMemcpyAsync(d_desc, &D, sizeof(DenseProb), hipMemcpyHostToDevice, st));
  const DenseCols cols = DenseCols::interleaved(reinterpret_cast<const double*>(S), (int)dim);
  HIPC(launch_dense_outputs(ctx, d_desc, 1, n, cols, n_t, 0, st));
  std::vector<double> hfam[kNumObsFamilies];
  for (ObsFamily f : kObsLaunchOrder) {
    if (!ctx->fam[f].on) continue;
    const ObsFamilyDesc& F = kObsFamilies[f];
    hfam[f].resize((size_t)n_t * F.stride(ctx, n));
    HIPC(hipMemcpyAsync(hfam[f].data(), D.*F.dense_out, hfam[f].size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPC(hipMemcpyAsync(P.buf[0], S + dim * (size_t)(n_t - 1), dim * sizeof(double2), hipMemcpyDeviceToDevice, st));
  std::vector<double> h((size_t)n_t * 8);
  int herr = 0;
  HIPC(hipMemcpyAsync(h.data(), d_obs, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  if (herr) return fail(ctx, DSE_ERR_HIP, "propagator-matrix mode: column build failed");
  for (int ti = 0; ti < n_t; ++ti)
    finish_obs(P, h.data() + (size_t)ti * 8, obs_out + (size_t)pi * DSE_N_OBS * n_t + ti, (size_t)n_t);
  for (ObsFamily f : kObsLaunchOrder)
    if (ctx->fam[f].on) finish_family_outputs(ctx, f, (size_t)pi, hfam[f].data(), (size_t)kObsFamilies[f].stride(ctx, n), n_t);
  P.degree = deg;
  *h_apps = (double)deg * (double)dim;
  float b_ms = 0.f, p_ms = 0.f;
  HIPC(hipEventElapsedTime(&b_ms, mev[0], mev[1]));
  HIPC(hipEventElapsedTime(&p_ms, mev[1], mev[2]));
  ctx->mx_build_ms = b_ms;
  ctx->mx_products_ms = p_ms;
  ctx->mx_products = (double)std::max(0, n_t - 1 - j_first);
  ctx->mx_bytes_per_product = (double)(u_elems * sizeof(double2) + dim * sizeof(double2));
  return DSE_OK;
}

// ---- hooks on a given state -------------------------------------------------------------------

// the hook's state `in` (the members' parts consecutive) into role 0 of members first .. first + count - 1
int upload_member_states(dse_ctx* ctx, int first, int count, const double2* in, hipStream_t st) {
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    const size_t amps = size_t(1) << P.n_local;
    HIPC(hipMemcpyAsync(P.buf[0], in + i * amps, amps * sizeof(double2), hipMemcpyHostToDevice, st));
  }
  return DSE_OK;
}

int64_t member_tiles(const dse_ctx* ctx, int first, int count) {
  int64_t tiles = 0;
  for (int i = 0; i < count; ++i) tiles += ctx->probs[first + i].n_tiles;
  return tiles;
}

// dse_site_observables / dse_pair_observables: family f of the state psi of register `problem`
int obs_family_hook(dse_ctx* ctx, ObsFamily f, int problem, const double* psi, double* out) {
  const ObsFamilyDesc& F = kObsFamilies[f];
  if (!ctx) return DSE_ERR_ARG;
  if (!psi || !out) return fail(ctx, DSE_ERR_ARG, "null pointer");
  int first = 0, count = 1;
  int rc = hook_members(ctx, problem, &first, &count);
  if (rc) return rc;
  if (F.hook_refuses_shard_early && ctx->probs[first].dist)
    return fail(ctx, DSE_ERR_ARG, std::string(F.hook) + ": not available for a dist shard");
  HIPC(hipSetDevice(ctx->device));
  if ((rc = prepare(ctx)) || (rc = set_unit_families_on(ctx, true))) return rc;
  if (!F.hook_refuses_shard_early && (rc = obs_family_refusal(ctx, f, F.hook))) return rc;
  if (F.per_problem_units && F.units(ctx->probs[first]) == 0)
    return fail(ctx, DSE_ERR_STATE, std::string(F.hook) + ": the problem has no " + F.option);
  const int64_t tiles = member_tiles(ctx, first, count);
  if ((rc = ensure_family_partial(ctx, f, 1))) return rc;
  const size_t S = (size_t)ctx->fam[f].S;
  double* const d_partial = ctx->fam[f].d_partial.p;
  hipStream_t st = ctx->lanes[0].stream;
  if ((rc = upload_member_states(ctx, first, count, reinterpret_cast<const double2*>(psi), st))) return rc;
  int64_t off = 0;
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    HIPC(F.launch(P.L, ctx->d_probs, P.d_items, (int)P.n_tiles, 0, d_partial + off * S, (int)S, st, 1, 0, 0));
    off += P.n_tiles;
  }
  std::vector<double> h(tiles * S);
  HIPC(hipMemcpyAsync(h.data(), d_partial, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  const int units = F.units(ctx->probs[first]);
  const int nv = F.comps * units, nrm = family_norm_at(F, units, S);
  std::vector<double> v(S, 0.0);
  for (int64_t t = 0; t < tiles; ++t) {
    for (int j = 0; j < nv; ++j) v[j] += h[t * S + j];
    v[nrm] += h[t * S + nrm];
  }
  finish_family(F, ctx->probs[first], v.data(), S, out, 1);
  ctx->evolved = false;
  return DSE_OK;
}

// dse_get_site_obs / dse_get_pair_obs: register `problem`'s record of the last evolve (a register
// without one, a non-zero shard, holds an empty store: its size differs)
int obs_family_get(dse_ctx* ctx, ObsFamily f, int problem, double* out) {
  if (!ctx) return DSE_ERR_ARG;
  if (!out) return fail(ctx, DSE_ERR_ARG, "null pointer");
  int first = 0, count = 1;
  int rc = hook_members(ctx, problem, &first, &count);
  if (rc) return rc;
  const ObsFamilyState& A = ctx->fam[f];
  const bool no_units = kObsFamilies[f].per_problem_units && kObsFamilies[f].units(ctx->probs[problem]) == 0;
  if (A.nt <= 0 || (size_t)problem >= A.store.size() || (kObsFamilies[f].get_needs_option && !A.on) || no_units ||
      A.store[problem].size() != obs_store_size(f, ctx->probs[problem], A.nt))
    return fail(ctx, DSE_ERR_STATE, std::string("no ") + kObsFamilies[f].noun + " observables (" +
                                        (kObsFamilies[f].per_problem_units
                                             ? std::string("give the problem ") + kObsFamilies[f].option
                                             : std::string("set option ") + kObsFamilies[f].option + " = 1") +
                                        " and call dse_evolve first)");
  std::copy(A.store[problem].begin(), A.store[problem].end(), out);
  return DSE_OK;
}

}  // namespace

extern "C" {

int dse_apply_h(dse_ctx* ctx, int problem, const double* psi_in, double* psi_out) {
  if (!ctx) return DSE_ERR_ARG;
  if (!psi_in || !psi_out) return fail(ctx, DSE_ERR_ARG, "null state");
  int first = 0, count = 1;
  int rc = hook_members(ctx, problem, &first, &count);
  if (rc) return rc;
  HIPC(hipSetDevice(ctx->device));
  if ((rc = prepare(ctx))) return rc;
  hipStream_t st = ctx->lanes[0].stream;
  double2* out = reinterpret_cast<double2*>(psi_out);
  if ((rc = upload_member_states(ctx, first, count, reinterpret_cast<const double2*>(psi_in), st))) return rc;
  if ((rc = apply_members(ctx, first, count, st))) return rc;
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    const size_t amps = size_t(1) << P.n_local;
    HIPC(hipMemcpyAsync(out + i * amps, P.buf[1], amps * sizeof(double2), hipMemcpyDeviceToHost, st));
  }
  HIPC(hipStreamSynchronize(st));
  ctx->evolved = false;
  return DSE_OK;
}

int dse_observables(dse_ctx* ctx, int problem, const double* psi, double* obs7) {
  if (!ctx) return DSE_ERR_ARG;
  if (!psi || !obs7) return fail(ctx, DSE_ERR_ARG, "null pointer");
  int first = 0, count = 1;
  int rc = hook_members(ctx, problem, &first, &count);
  if (rc) return rc;
  HIPC(hipSetDevice(ctx->device));
  if ((rc = prepare(ctx))) return rc;
  const int64_t tiles = member_tiles(ctx, first, count);
  if ((rc = ensure_partial(ctx, 1))) return rc;
  hipStream_t st = ctx->lanes[0].stream;
  if ((rc = upload_member_states(ctx, first, count, reinterpret_cast<const double2*>(psi), st))) return rc;
  if (ctx->probs[first].dist && (rc = dist_exchange(ctx, 0, 0, st))) return rc;
  int64_t off = 0;
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    HIPC(launch_obs(P.L, ctx->d_probs, P.d_items, (int)P.n_tiles, 0, ctx->d_partial.p + off * 8, st));
    off += P.n_tiles;
  }
  std::vector<double> h(tiles * 8);
  HIPC(hipMemcpyAsync(h.data(), ctx->d_partial.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int64_t t = 0; t < tiles; ++t)
    for (int j = 0; j < 7; ++j) v[j] += h[t * 8 + j];
  if (ctx->probs[first].dist && (rc = xchg_allreduce_host(ctx, v, 7, st))) return rc;  // all shards
  finish_obs(ctx->probs[first], v, obs7, 1);
  ctx->evolved = false;
  return DSE_OK;
}

int dse_site_observables(dse_ctx* ctx, int problem, const double* psi, double* out) { return obs_family_hook(ctx, kSite, problem, psi, out); }
int dse_site_obs_outputs(const dse_ctx* ctx) { return ctx ? ctx->fam[kSite].nt : DSE_ERR_ARG; }
int dse_get_site_obs(dse_ctx* ctx, int problem, double* out) { return obs_family_get(ctx, kSite, problem, out); }

int dse_pair_observables(dse_ctx* ctx, int problem, const double* psi, double* out) { return obs_family_hook(ctx, kPair, problem, psi, out); }
int dse_pair_obs_outputs(const dse_ctx* ctx) { return ctx ? ctx->fam[kPair].nt : DSE_ERR_ARG; }
int dse_pair_obs_problems(const dse_ctx* ctx) { return ctx ? obs_family_problems(ctx, kPair) : DSE_ERR_ARG; }
int dse_get_pair_obs(dse_ctx* ctx, int problem, double* out) { return obs_family_get(ctx, kPair, problem, out); }

int dse_overlaps(dse_ctx* ctx, int problem, const double* psi, double* out) { return obs_family_hook(ctx, kOverlap, problem, psi, out); }
int dse_overlap_outputs(const dse_ctx* ctx) { return ctx ? ctx->fam[kOverlap].nt : DSE_ERR_ARG; }
int dse_overlap_problems(const dse_ctx* ctx) { return ctx ? obs_family_problems(ctx, kOverlap) : DSE_ERR_ARG; }
int dse_get_overlaps(dse_ctx* ctx, int problem, double* out) { return obs_family_get(ctx, kOverlap, problem, out); }

int dse_op_string_values(dse_ctx* ctx, int problem, const double* psi, double* out) { return obs_family_hook(ctx, kString, problem, psi, out); }
int dse_op_string_outputs(const dse_ctx* ctx) { return ctx ? ctx->fam[kString].nt : DSE_ERR_ARG; }
int dse_op_string_problems(const dse_ctx* ctx) { return ctx ? obs_family_problems(ctx, kString) : DSE_ERR_ARG; }
int dse_get_op_strings(dse_ctx* ctx, int problem, double* out) { return obs_family_get(ctx, kString, problem, out); }

int dse_sector_values(dse_ctx* ctx, int problem, const double* psi, double* out) { return obs_family_hook(ctx, kSector, problem, psi, out); }
int dse_sector_outputs(const dse_ctx* ctx) { return ctx ? ctx->fam[kSector].nt : DSE_ERR_ARG; }
int dse_sector_problems(const dse_ctx* ctx) { return ctx ? obs_family_problems(ctx, kSector) : DSE_ERR_ARG; }
int dse_get_sectors(dse_ctx* ctx, int problem, double* out) { return obs_family_get(ctx, kSector, problem, out); }

int dse_has_feature(const char* name) {
  if (!name) return 0;
  const std::string k(name);
  return k == "site_obs" || k == "initial_state" || k == "pair_obs" || k == "overlap_obs" || k == "pulse" ||
         k == "set_hamiltonian" || k == "op_strings" || k == "sector_obs" || k == "leap";
}

int dse_leap_problems(const dse_ctx* ctx) { return ctx ? ctx->leap_problems : DSE_ERR_ARG; }

// the leap path's uniform-grid rule: max_m |t_m - (t_0 + m delta)| <= 2 ulp(|t_last|) with
// delta = (t_last - t_0) / (n_t - 1)
int dse_uniform_spacing(const double* t, int n_t, double* delta) {
  if (!t || n_t < 1) return DSE_ERR_ARG;
  if (delta) *delta = 0.0;
  if (n_t < 2) return 0;
  const double d = (t[n_t - 1] - t[0]) / (n_t - 1);
  const double last = std::fabs(t[n_t - 1]);
  const double ulp = std::nextafter(last, std::numeric_limits<double>::infinity()) - last;
  if (!(d > 0.0)) return 0;
  for (int m = 0; m < n_t; ++m)
    if (!(std::fabs(t[m] - (t[0] + m * d)) <= 2.0 * ulp)) return 0;
  if (delta) *delta = d;
  return 1;
}

// ---- spanning registers (dse_span.hip) ------------------------------------------------------

// option span_tile = -1: the automatic choice takes the first of these (tile bits, resident
// launches) whose workgroups fit: 2^10 tiles one per CU, all at once (a lone N = 14 register over
// 16 CUs: 78 vs 85 ms at 150 kHz); 2^11 at the kernel's occupancy, all at once (one GPU's share of
// an 8-GPU strong split); 2^11 in two resident launches per interval (span_cuts; the registers in
// degree order, so the stiff ones share the first): one GPU's share of a 4-GPU split, 169 against
// 225 ms on k_interval, while three launches (a 2-GPU share) lose, 246 against 234 ms
// (profiles/r06/span_chunks_shard{4,2}.jsonl)
constexpr int kSpanAutoTiles[3][2] = {{10, 1}, {11, 1}, {11, 2}};

// amplitudes per thread of k_span for an L-bit tile: 2^rb (option span_rb, else 512 threads)
int span_rb_for(const dse_ctx* ctx, int L) { return ctx->span_rb > 0 ? ctx->span_rb : L - 9; }

// whether register P can span its top s bits (2^s tiles of n - s bits)
bool span_eligible(const dse_ctx* ctx, const HostProblem& P, int s) {
  if (P.side() || P.shard_bits != 0 || s < 1 || s > kSpanMaxTop) return false;
  const int L = P.n_local - s;
  return L >= 1 && span_supported(L, span_rb_for(ctx, L));
}

// The tables k_span reads for register P cut into 2^s tiles of L bits, RB of them register bits
// (dse_internal.h SpanTab).  Same coefficients as build_tables, sorted by k_span's layout.
int build_span_table(const HostProblem& P, int L, int RB, int s, SpanTab& T) {
  const int n = P.n;
  const int TB = L - RB;
  const int npi = (TB * (TB - 1) / 2 + TB - 1) / TB;
  const int iw = 4 + npi;
  if (TB * iw > kSpanMaxIt || L > 16 || RB > 4 || s > kSpanMaxTop || n != L + s) return DSE_ERR_ARG;
  std::memset(&T, 0, sizeof(T));
  T.n_it = TB * iw;
  auto it = [&](int j, int e) -> double2& { return T.it[j * iw + e]; };
  std::vector<std::pair<uint32_t, double>> tpairs;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const double g = P.pair[i * n + j];
      if (g == 0.0) continue;
      if (j < TB) {
        tpairs.push_back({(1u << i) | (1u << j), g});
      } else if (j < L && i < TB) {
        const int r = j - TB;
        (r & 1 ? it(i, 2 + r / 2).y : it(i, 2 + r / 2).x) = g;
      } else if (j < L) {
        T.rr_g[rr_index(i - TB, j - TB)] = g;
      } else if (i < L) {
        T.ug[j - L][i] = g;
        T.u_mask |= 1 << (j - L);
      } else {
        SpanOp& o = T.ops[T.n_ops++];
        o.kind = 2;
        o.b = i - L;
        o.b2 = j - L;
        o.pmask = (1u << o.b) | (1u << o.b2);
        o.c[0] = g;
        T.need_raw = 1;
      }
    }
  if ((int)tpairs.size() > TB * npi) return DSE_ERR_ARG;
  for (size_t p = 0; p < tpairs.size(); ++p) {
    double2& e = it((int)(p / npi), 4 + (int)(p % npi));
    e.x = __builtin_bit_cast(double, (uint64_t)tpairs[p].first);
    e.y = tpairs[p].second;
  }
  for (int b = 0; b < n; ++b) {
    double f[4];
    for (int c = 0; c < 4; c += 2) {  // as build_tables: cos(pi/2) residues dropped
      f[c] = P.flip[4 * b + c];
      f[c + 1] = P.flip[4 * b + c + 1];
      if (std::fabs(f[c]) <= 1e-15 * std::hypot(f[c], f[c + 1])) f[c] = 0.0;
    }
    if (f[0] == 0.0 && f[1] == 0.0 && f[2] == 0.0 && f[3] == 0.0) continue;
    if (b < TB) {
      it(b, 0) = make_double2(f[0], f[1]);
      it(b, 1) = make_double2(f[2], f[3]);
    } else if (b < L) {
      for (int c = 0; c < 4; ++c) T.rflip[b - TB][c] = f[c];
      T.rflip_mask |= 1 << (b - TB);
    } else {
      for (int c = 0; c < 4; ++c) T.uflip[b - L][c] = f[c];
    }
  }
  // operands: u of every top bit with crossing pairs; the raw partner under the drive of every
  // top bit without them (and with a drive)
  for (int b = 0; b < s; ++b) {
    const bool has_flip = T.uflip[b][0] != 0.0 || T.uflip[b][1] != 0.0 || T.uflip[b][2] != 0.0 || T.uflip[b][3] != 0.0;
    if (!((T.u_mask >> b) & 1) && !has_flip) continue;
    SpanOp& o = T.ops[T.n_ops++];
    o.kind = ((T.u_mask >> b) & 1) ? 0 : 1;
    o.b = o.b2 = b;
    o.pmask = 1u << b;
    if (o.kind == 1) {
      for (int c = 0; c < 4; ++c) o.c[c] = T.uflip[b][c];
      T.need_raw = 1;
    }
  }
  return DSE_OK;
}

// ---- real-component registers (dse_real.hip) ---------------------------------------------------

bool real_eligible(const HostProblem& P) {
  return !P.side() && P.span_s == 0 && P.shard_bits == 0 && P.imag && (P.n_local == 13 || P.n_local == 14);
}

// RealTab of register P (n = 13 or 14: 9 thread bits, n - 9 register bits): the coefficients of
// H' = D H D^dagger, D|x> = i^|x| |x>: pairs -g (i^{+-2}), drives by the output bit value v of the
// flipped bit: v = 0 -> +Im c0, v = 1 -> -Im c1 (i^{-+1} times the imaginary coefficient, k_dense_h)
int build_real_table(const HostProblem& P, RealTab& T) {
  const int n = P.n, TB = 9, RB = n - TB;
  if (RB < 4 || RB > kRealRB) return DSE_ERR_ARG;
  std::memset(&T, 0, sizeof(T));
  auto row = [&](int j, int e) -> double& {
    double2& d = T.it[j * 6 + e / 2];
    return (e & 1) ? d.y : d.x;
  };
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const double g = -P.pair[i * n + j];
      if (g == 0.0) continue;
      if (j < TB) {  // canonical slot of (i, j): lexicographic over a < b < 9, 4 per iteration
        const int p = i * TB - i * (i + 1) / 2 + (j - i - 1);
        row(p / 4, 8 + p % 4) = g;
      } else if (i < TB) {
        row(i, 2 + (j - TB)) = g;
      } else {
        T.rr_g[real_rr_index(i - TB, j - TB)] = g;
      }
    }
  for (int b = 0; b < n; ++b) {
    double f[4];
    for (int c = 0; c < 4; c += 2) {  // as build_tables: cos(pi/2) residues dropped
      f[c] = P.flip[4 * b + c];
      f[c + 1] = P.flip[4 * b + c + 1];
      if (std::fabs(f[c]) <= 1e-15 * std::hypot(f[c], f[c + 1])) f[c] = 0.0;
    }
    if (f[0] != 0.0 || f[2] != 0.0) return DSE_ERR_ARG;  // not an imaginary drive
    if (f[1] == 0.0 && f[3] == 0.0) continue;
    if (b < TB) {
      row(b, 0) = f[1];
      row(b, 1) = -f[3];
    } else {
      T.rflip[b - TB][0] = f[1];
      T.rflip[b - TB][1] = -f[3];
      T.rflip_mask |= 1 << (b - TB);
    }
  }
  // a custom psi(t0): k_real_split writes [a | b] = [Re phi0 | Im phi0] with the whole phase i^|x|
  // in phi0, so the combine rotates back by i^{-|x|} alone
  T.x0 = P.init_kind ? kRealFromBuffer : P.psi0;
  T.x0pop = P.init_kind ? 0 : __builtin_popcountll(P.psi0);
  return DSE_OK;
}

}  // extern "C"

namespace {

// ---- dse_evolve: the plan of one call and the phases that fill and run it ----------------------

struct IntervalGroup { int m0, n_out, set; };  // up to M consecutive output intervals: one launch per lane group

// Kernel timing of the launch loop (option time_every): per lane and event pool the counters of the
// launches under an event pair, and the sums drain() adds them to once the events have completed
struct LaunchTimer {
  // of one launch: algorithmic flops, HBM bytes (streaming; the persistent kernels' traffic is not
  // modelled: 0) and amplitudes x Chebyshev terms
  struct Rec { double flops, bytes, amp_terms; };
  std::vector<std::vector<Rec>> recs;  // [lane * 2 + pool][event pair]
  double step_ms = 0.0, launches = 0.0, flops = 0.0, bytes = 0.0, amp_terms = 0.0;
  double lane0_ms = 0.0, lane0_launches = 0.0, lane0_amp_terms = 0.0;  // lane 0 alone (stats)

  // launch() between two event records when the interval is timed and the pool has a pair left
  // (records beyond the pool are skipped, not timed), bare otherwise
  template <class F>
  int run(dse_ctx* ctx, Lane& ln, size_t li, int pool, bool timed, const Rec& r, F&& launch) {
    if (!timed || 2 * ln.ev_used[pool] + 2 > ln.ev[pool].size()) return launch();
    const size_t i = ln.ev_used[pool]++;
    HIPC(hipEventRecord(ln.ev[pool][2 * i], ln.stream));
    if (int rc = launch()) return rc;
    HIPC(hipEventRecord(ln.ev[pool][2 * i + 1], ln.stream));
    recs[li * 2 + pool].push_back(r);
    return DSE_OK;
  }
  int drain(dse_ctx* ctx, Lane& ln, size_t li, int pool) {
    if (ln.ev_used[pool] == 0) return DSE_OK;
    HIPC(hipEventSynchronize(ln.ev[pool][2 * ln.ev_used[pool] - 1]));
    for (size_t i = 0; i < ln.ev_used[pool]; ++i) {
      float ms = 0.f;
      HIPC(hipEventElapsedTime(&ms, ln.ev[pool][2 * i], ln.ev[pool][2 * i + 1]));
      const Rec& r = recs[li * 2 + pool][i];
      step_ms += ms;
      flops += r.flops;
      amp_terms += r.amp_terms;
      if (li == 0) lane0_ms += ms, lane0_amp_terms += r.amp_terms, lane0_launches += 1.0;
      bytes += r.bytes;
    }
    launches += (double)ln.ev_used[pool];
    ln.ev_used[pool] = 0;
    recs[li * 2 + pool].clear();
    return DSE_OK;
  }
};

// What the phases of one dse_evolve decide and count; a phase reads another's results here or in ctx
struct EvolvePlan {
  const double* t = nullptr;  // the call's arguments
  int n_t = 0;
  double tol = 0.0, *obs_out = nullptr;
  std::chrono::steady_clock::time_point wall0, tmark;
  bool persistent = false, any_small = false, any_big = false, any_dense = false, any_dist = false;
  bool any_dist_step = false;  // dist shards on the step kernels: per-term shard exchange
  bool used_wht = false, all_span = true, imag_all = true;
  bool obs_ovl = false;  // persistent with option obs_overlap
  int matrix_pi = -1;    // the register in propagator-matrix mode (matrix_run), or -1; its time step
  double matrix_dt = 0.0;
  int M = 1;  // outputs per launch
  double leap_dt = 0.0;  // > 0: the evolve runs on the leap path (choose_leap), the grid's spacing
  std::vector<IntervalGroup> groups;
  std::vector<std::vector<double>> set_tau;  // per coefficient set: offsets t[m0 + j + 1] - t[m0], j < n_out
  size_t chunk = 1;                          // output slots of the partial arenas per flush
  int n_lanes = 1;
  int64_t cap = 2;  // workgroups of one 2-tile interval launch (all resident at once), even
  std::vector<int2> items, span_items, real_items;
  int* d_err = nullptr;  // the hand-off error word (persistent)
  int max_deg = 1;
  size_t slot = 0, t_flushed = 0;  // the launch loop: arena slots in use; output times already flushed
  std::vector<double> dist_raw;    // raw sums of the registers partitioned over processes
  // counters (stats)
  double small_happl = 0.0, small_launches = 0.0, dense_ms = 0.0, dense_eig_ms = 0.0, matrix_happl = 0.0;
  double launches = 0.0, amp_updates = 0.0, all_bytes = 0.0, all_flops = 0.0;
  LaunchTimer timer;

  // DSE_HOST_TIMING=1: host time of each phase of this call on stderr (diagnostics)
  void phase(const char* name) {
    static const bool host_timing = std::getenv("DSE_HOST_TIMING") != nullptr;
    if (!host_timing) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[dse_evolve] %-12s %9.3f ms\n", name,
                 std::chrono::duration<double, std::milli>(now - tmark).count());
    tmark = now;
  }
};

int check_times(dse_ctx* ctx, const EvolvePlan& pl) {
  if (!pl.t || !pl.obs_out) return fail(ctx, DSE_ERR_ARG, "null pointer");
  if (pl.n_t < 1) return fail(ctx, DSE_ERR_ARG, "n_t must be >= 1");
  if (!(pl.tol > 0.0 && pl.tol < 1e-2)) return fail(ctx, DSE_ERR_ARG, "tol must be in (0, 1e-2)");
  for (int i = 0; i < pl.n_t; ++i)
    if (!std::isfinite(pl.t[i])) return fail(ctx, DSE_ERR_ARG, "non-finite time");
  for (int i = 1; i < pl.n_t; ++i)
    if (!(pl.t[i] > pl.t[i - 1])) return fail(ctx, DSE_ERR_ARG, "times must be strictly increasing");
  return DSE_OK;
}

// ---- execution mode ----
// small registers (n <= 9): the one-wave engine (dse_small.hip) on its own stream, whatever the
// other problems run on.  Of the rest -- persistent: every problem fits one or two
// register-block tiles -> one k_interval launch per group of output intervals and lane;
// streaming: per-term kernels, one output per group.
int choose_engines(dse_ctx* ctx, EvolvePlan& pl) {
  int rc;
  // dense engine first (option "dense"): a register it takes is off every Chebyshev path
  for (auto& P : ctx->probs) {
    P.dn = ctx->dense && dense_eligible(P) && (ctx->dense == 2 || dense_cheaper(P, pl.t, pl.n_t, ctx->eig_impl));
    pl.any_dense = pl.any_dense || P.dn;
  }
  for (auto& P : ctx->probs) {
    P.mx = false;
    P.sm = !P.dn && ctx->small && P.shard_bits == 0 && P.n_local <= kSmallMaxQubits;
    pl.any_small = pl.any_small || P.sm;
  }
  // a context whose Chebyshev work is one register: propagator-matrix mode (matrix_run) when the
  // persistent kernel is allowed and the model prefers it
  int n_cheb = 0, last = -1;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi)
    if (!ctx->probs[pi].side()) ++n_cheb, last = (int)pi;
  if (n_cheb == 1 && ctx->matrix && ctx->persistent) {
    HostProblem& P = ctx->probs[last];
    // the matrix-mode buffers must fit 80% of the free memory (plus what the context already
    // holds for them); otherwise the register stays on the per-interval kernels
    size_t free_b = 0, total_b = 0;
    HIPC(hipMemGetInfo(&free_b, &total_b));
    const bool fits = matrix_bytes(P, pl.n_t) <= 0.8 * (double)free_b + (double)ctx->d_mx.cap;
    if (fits && matrix_eligible(P, pl.t, pl.n_t, &pl.matrix_dt) &&
        (ctx->matrix == 2 || matrix_cheaper(P, pl.matrix_dt, pl.n_t, ctx->n_cu))) {
      P.mx = true;
      pl.matrix_pi = last;
    }
  }
  for (auto& P : ctx->probs) pl.any_big = pl.any_big || !P.side();
  for (ObsFamily f : kObsLaunchOrder)
    if (ctx->fam[f].on && (rc = obs_family_refusal(ctx, f, kObsFamilies[f].option))) return rc;
  for (ObsFamily f : kObsLaunchOrder) reset_family_store(ctx, f, pl.n_t);
  pl.persistent = ctx->persistent != 0;
  return DSE_OK;
}

// the all-span candidates kSpanAutoTiles[ti0, ti1): the smallest tile whose workgroups fit (0: none)
int all_span_tile(dse_ctx* ctx, bool persistent, int ti0, int ti1) {
  int tl = 0;
  for (int ti = ti0; ti < ti1 && tl == 0; ++ti) {
    const int L = kSpanAutoTiles[ti][0], chunks = kSpanAutoTiles[ti][1];
    int64_t wg = 0;
    bool all = persistent && ctx->span == 0;
    for (auto& P : ctx->probs) {
      if (P.side()) continue;
      const int s = P.n_local - L;
      if (!span_eligible(ctx, P, s)) all = false;
      wg += int64_t(1) << std::max(0, s);
    }
    int per_cu = 1;
    if (ti > 0 && span_occupancy(L, span_rb_for(ctx, L), true, &per_cu) != hipSuccess) per_cu = 0;
    if (all && wg > 0 && chunks <= ctx->span_chunks && wg <= (int64_t)chunks * per_cu * ctx->n_cu) tl = L;
  }
  return tl;
}

// Partial span (option span_partial, round 6): when the registers do not all fit spanned (one
// GPU's share of a 2-GPU split: 96 registers), the ones with the longest predicted chains span
// over 2^11-amplitude tiles on a lane of their own while the rest stay on k_interval, as long
// as every workgroup of both launches fits the chip at once (each takes a CU: residency of
// every hand-off partner is guaranteed, whatever order the two streams' workgroups land in).
// Predicted chain of a register: its spectral half-width (degree per interval ~ alpha dt) times
// the measured term time of its kernel under load (kTermUs); applied when the longest chain
// shrinks by at least 10%.  True when it set the span_s of some registers.
bool choose_partial_span(dse_ctx* ctx) {
  if (ctx->span != 0 || !ctx->span_partial || std::min<int>(ctx->n_streams, (int)ctx->probs.size()) < 2) return false;
  const int Lp = ctx->span_partial_tile;
  // term time under load: k_interval 1-tile, 2-tile; k_span over 2^Lp-amplitude tiles
  const double kTermUs[3] = {19.5, 24.0, Lp == 11 ? 14.0 : 11.0};
  struct C {
    double chain;
    int pi, kind;  // kind 0 / 1: k_interval of 1 / 2 tiles, 2: spanned
  };
  std::vector<C> cs;
  int64_t wg = 0;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    if (P.side()) continue;
    // (and kTermUs has entries for 1- and 2-tile registers only)
    if (P.shard_bits != 0 || !(P.n_tiles == 1 || P.n_tiles == 2) || !interval_supported(P.L)) return false;
    wg += P.n_tiles;
    const double alpha = 0.5 * (P.e_max - P.e_min);
    cs.push_back({alpha * kTermUs[P.n_tiles - 1], (int)pi, (int)P.n_tiles - 1});
  }
  auto worst = [&]() { return std::max_element(cs.begin(), cs.end(), [](const C& a, const C& b) { return a.chain < b.chain; }); };
  if (cs.empty() || wg > ctx->n_cu) return false;
  const double before = worst()->chain;
  std::vector<int> spanned;
  for (;;) {
    auto w = worst();
    if (w->kind == 2) break;
    const HostProblem& P = ctx->probs[w->pi];
    const int sp = P.n_local - Lp;
    if (!span_eligible(ctx, P, sp)) break;
    const int64_t extra = (int64_t(1) << sp) - P.n_tiles;
    if (wg + extra > ctx->n_cu) break;
    wg += extra;
    w->chain = w->chain / kTermUs[w->kind] * kTermUs[2];
    w->kind = 2;
    spanned.push_back(w->pi);
  }
  if (spanned.empty() || worst()->chain > 0.9 * before) return false;
  for (int pi : spanned) ctx->probs[pi].span_s = ctx->probs[pi].n_local - Lp;
  return true;
}

// spanning registers (options span / span_tile): every register that fits runs on k_span over
// 2^s tiles.  span_tile = -1 (default, auto): when the context's registers are few enough that
// all their 2^11-amplitude tiles fit the chip in at most two resident launches (one GPU's share
// of a 4- or 8-GPU strong split, a lone simulate_rare register), a shorter chain per register;
// otherwise none spans (kSpanAutoTiles).  Then whether the evolve is persistent at all.
void choose_span(dse_ctx* ctx, EvolvePlan& pl) {
  const bool persistent = pl.persistent;
  int tile = ctx->span_tile;
  auto assign = [&]() {
    for (auto& P : ctx->probs) {
      const int s = tile > 0 ? P.n_local - tile : ctx->span;
      P.span_s = (persistent && span_eligible(ctx, P, s)) ? s : 0;
    }
  };
  // order: every register spanned in one resident launch; else the partial span; else every
  // register spanned in two resident launches (the partial form measured faster on the 4-GPU
  // share, 151 against 167 ms, profiles/r06/span_partial_shards.jsonl)
  if (tile < 0) tile = all_span_tile(ctx, persistent, 0, 2);
  assign();
  const bool automatic = ctx->span_tile < 0 && tile == 0;
  const bool partial = automatic && persistent && choose_partial_span(ctx);
  if (automatic && !partial && (tile = all_span_tile(ctx, persistent, 2, 3)) > 0) assign();
  for (auto& P : ctx->probs) {
    if (P.side()) continue;
    if (P.span_s == 0 && (!(interval_supported(P.L) && P.n_tiles <= 2) || P.shard_bits > 0)) pl.persistent = false;
    pl.any_dist = pl.any_dist || P.dist;
  }
  if (!pl.persistent)
    for (auto& P : ctx->probs) P.span_s = 0;
}

// real-component mode: option real = 1 when every Chebyshev register qualifies (one launch kind
// per interval); real = 2 the 2-tile (14-qubit) registers only, on their own stream beside the
// 1-tile registers' k_interval launches (neither kernel waits on another workgroup, so the two
// persistent launches share the chip without a residency condition)
void choose_real(dse_ctx* ctx, const EvolvePlan& pl) {
  bool real_mode = pl.persistent && ctx->real_mode && !ctx->obs_overlap;
  int n_cheb = 0;
  for (auto& P : ctx->probs) {
    if (P.side()) continue;
    ++n_cheb;
    if (ctx->real_mode == 1) real_mode = real_mode && real_eligible(P);
  }
  for (auto& P : ctx->probs)
    P.rl = real_mode && n_cheb > 0 && !P.side() && (ctx->real_mode == 1 || (real_eligible(P) && P.n_tiles == 2));
}

// the spacing delta of a uniform output grid, max_m |t_m - (t_0 + m delta)| <= 2 ulp(|t_last|) with
// delta = (t_last - t_0) / (n_t - 1); 0 when the grid is not uniform (or has one point)
double uniform_spacing(const double* t, int n_t) {
  double delta = 0.0;
  return dse_uniform_spacing(t, n_t, &delta) == 1 ? delta : 0.0;
}

// The leap path (option leap; dse_real.hip at k_leap_combine): on a uniform grid, from basis states,
// a launch needs one real recurrence per register (k_real's component 0 on p_m) and the outputs
// follow from the time recurrence.  Taken when the evolve is persistent without obs_overlap, every
// Chebyshev register is real_eligible (13 or 14 qubits, imaginary drives, whole) and starts from its
// basis state, outputs_per_launch is 2, alpha delta leap_fan < 400 and the grid is uniform.  leap = -1 (default) is part of the
// automatic layout policy: only with span_tile = -1, real = 0 and the hand-off kernels' own knobs
// (spin_limit, handoff_fences, xcd_pairs, coresident) at their defaults, so a caller that pins
// k_interval, k_span or k_real keeps the kernel it names.
void choose_leap(dse_ctx* ctx, EvolvePlan& pl) {
  pl.leap_dt = 0.0;
  for (auto& P : ctx->probs) P.lp = false;
  const bool automatic = ctx->span_tile == -1 && ctx->real_mode == 0 && ctx->hk.spin_limit == HandoffKnobs().spin_limit &&
                         ctx->hk.fences == 0 && ctx->xcd_pairs == 1 && ctx->coresident == 0;
  if (ctx->leap == 0 || (ctx->leap < 0 && !automatic) || !pl.persistent || ctx->obs_overlap) return;
  // the time recurrence amplifies a launch's rounding by the number of launches after it: two outputs per
  // series only (one per series doubles the launches: 5e-13 of norm after 30 outputs against 6e-14, measured)
  if (ctx->outputs_per_launch != kMaxOut) return;
  const double delta = uniform_spacing(pl.t, pl.n_t);
  if (!(delta > 0.0)) return;
  int n_cheb = 0;
  for (auto& P : ctx->probs) {
    if (P.side()) continue;
    ++n_cheb;
    if (!real_eligible(P) || P.init_kind != 0) return;
    // (as choose_outputs_per_launch's rule for two outputs per series; the fan-out's series reach twice as far)
    if (!(0.5 * (P.e_max - P.e_min) * delta * ctx->leap_fan < 400.0)) return;
  }
  if (n_cheb == 0) return;
  pl.leap_dt = delta;
  for (auto& P : ctx->probs) P.rl = P.lp = !P.side();
}

// streaming: registers of more than one 2^13 tile take the Walsh-Hadamard engine (option wht)
int choose_wht(dse_ctx* ctx, EvolvePlan& pl) {
  pl.any_dist_step = pl.any_dist;
  if (pl.persistent) return DSE_OK;
  if (int rc = ensure_wht(ctx)) return rc;
  pl.any_dist_step = false;
  for (auto& P : ctx->probs) {
    pl.used_wht = pl.used_wht || P.wht_groups > 0;
    pl.any_dist_step = pl.any_dist_step || (P.dist && P.wht_groups == 0);
  }
  return DSE_OK;
}

// Outputs per launch M: the Chebyshev series of e^{-iH tau} converges after ~ alpha tau +
// O((alpha tau)^{1/3}) terms, so M outputs from one series (one propagator sum per output, same
// vectors T_k(H~) psi) need fewer H applications than M series of one interval each when alpha
// dt is small (the N = 14 sweep on its 1 ms grid: -23% for the stiffest problem at M = 4).  On
// coarse grids (alpha dt >= 400) the saving is nil and the coefficient tables grow, so M = 1.
void choose_outputs_per_launch(dse_ctx* ctx, EvolvePlan& pl) {
  double max_z = 0.0;
  for (int m = 0; m + 1 < pl.n_t; ++m)
    for (auto& P : ctx->probs)
      if (!P.side()) max_z = std::max(max_z, 0.5 * (P.e_max - P.e_min) * (pl.t[m + 1] - pl.t[m]));
  // k_span staggers its outputs' sums over the terms (coef_nterm phases), so an evolve whose
  // registers all span takes up to kSpanMaxOut outputs per series (option span_outputs);
  // k_interval and k_real update every output's sum in one term, from registers: at most two
  for (auto& P : ctx->probs)
    if (!P.side()) pl.all_span = pl.all_span && P.span_s > 0 && !P.rl;
  if (pl.persistent && max_z < 400.0)
    pl.M = std::max(1, std::min(pl.all_span ? ctx->span_outputs : ctx->outputs_per_launch, pl.n_t - 1));
  // the leap path's fan-out: leap_fan workgroups per register, kMaxOut outputs each, from the same p_m
  if (pl.leap_dt > 0.0) pl.M = std::max(1, std::min(kMaxOut * ctx->leap_fan, pl.n_t - 1));
  pl.obs_ovl = pl.persistent && ctx->obs_overlap;
}

// groups of M consecutive output intervals -> coefficient sets (distinct offset lists)
int group_intervals(dse_ctx* ctx, EvolvePlan& pl) {
  const double* t = pl.t;
  const int n_t = pl.n_t, M = pl.M;
  if (pl.leap_dt > 0.0) {  // the leap path: one set, the offsets j delta; a tail launch takes its first rows
    std::vector<double> tau(M);
    for (int j = 0; j < M; ++j) tau[j] = (j + 1) * pl.leap_dt;
    pl.set_tau.push_back(tau);
  }
  for (int m0 = 0; m0 + 1 < n_t; m0 += M) {
    IntervalGroup g;
    g.m0 = m0;
    g.n_out = std::min(M, n_t - 1 - m0);
    if (pl.leap_dt > 0.0) {
      g.set = 0;
      pl.groups.push_back(g);
      continue;
    }
    std::vector<double> tau(g.n_out);
    for (int j = 0; j < g.n_out; ++j) tau[j] = t[m0 + j + 1] - t[m0];
    g.set = -1;
    for (size_t q = 0; q < pl.set_tau.size(); ++q)
      if (pl.set_tau[q] == tau) {
        g.set = (int)q;
        break;
      }
    if (g.set < 0) {
      if (pl.set_tau.size() >= 4096) return fail(ctx, DSE_ERR_ARG, "more than 4096 distinct output intervals");
      g.set = (int)pl.set_tau.size();
      pl.set_tau.push_back(tau);
    }
    pl.groups.push_back(g);
  }
  if (pl.set_tau.empty()) pl.set_tau.push_back(std::vector<double>(1, 0.0));
  return DSE_OK;
}

// Chebyshev coefficients per problem (cheb_rows: [set][output j][term k]), all problems' rows
// gathered into one arena and uploaded with one copy.  Problems are independent: computed on up to
// 16 host threads (Bessel series of every distinct offset set, ~3 us each), then gathered in
// problem order.
int build_coefficients(dse_ctx* ctx, EvolvePlan& pl) {
  using Row = std::pair<double, double>;
  static_assert(sizeof(Row) == sizeof(double2), "cheb_rows fills the device's double2 rows");
  const int M = pl.M;
  std::vector<std::vector<Row>> coef_rows(ctx->probs.size());
  std::vector<int> coef_rc(ctx->probs.size(), DSE_OK);
  std::vector<std::string> coef_msg(ctx->probs.size());
  auto coef_one = [&](size_t pi) {
    HostProblem& P = ctx->probs[pi];
    if (P.side()) return;
    const double alpha = std::max(0.5 * (P.e_max - P.e_min), 1e-300);
    const double beta = 0.5 * (P.e_max + P.e_min);
    int deg = 1, kmax = 0;
    // (the leap path's rows carry no e^{-i beta tau}: a_k real for even k, imaginary for odd k; the
    // combine applies the phase of each output's own time)
    // Its series are cut at tol / launches.  A truncation error E of C_j shifts cos(theta) of every
    // eigenmode in every launch alike; where |cos(theta)| = 1 the time recurrence then grows like
    // cosh(N sqrt(2 E)) - 1 = N^2 E over N launches (measured on the bench's 50 launches at E = tol = 1e-14:
    // 9e-12 of norm, against the N E = 6e-13 of the chained propagators), so E = tol / N keeps the
    // evolve's total at the chained schemes' N tol.  J_k falls so fast that this is 4 to 6 terms of 191.
    const double tol = P.lp ? pl.tol / (double)std::max<size_t>(1, pl.groups.size()) : pl.tol;
    coef_rc[pi] = cheb_rows(alpha, P.lp ? 0.0 : beta, pl.set_tau, M, tol, ctx->max_degree, &deg, &coef_rows[pi], &kmax);
    if (coef_rc[pi] == DSE_ERR_CONVERGENCE)
      coef_msg[pi] = "Chebyshev degree " + std::to_string(kmax) + " exceeds max_degree; use a finer output grid";
    else if (coef_rc[pi] != DSE_OK)
      coef_msg[pi] = "bessel failed";
    if (coef_rc[pi] != DSE_OK) return;
    P.degree = deg;
    if (P.lp)  // the leap path: the degree of each workgroup's pair of rows, which its launch items carry
      for (int g = 0; g * kMaxOut < M; ++g) {
        P.leap_k[g] = 1;
        for (int j = g * kMaxOut; j < std::min(M, (g + 1) * kMaxOut); ++j)
          P.leap_k[g] = std::max(P.leap_k[g], (int)coef_rows[pi][(size_t)j * (deg + 2)].first);
      }
    DevProb& d = ctx->h_desc[pi];
    d.kcap1 = deg + 1;
    d.degree = deg;
    d.beta = beta;
    d.s1 = 1.0 / alpha;
    d.n_acc = M;
    d.xacc_q = pl.obs_ovl ? M - 1 : 0;
  };
  if (ctx->dbg & 4)
    for (size_t pi = 0; pi < ctx->probs.size(); ++pi) coef_one(pi);
  else
    parallel_for(ctx->probs.size(), coef_one);
  Arena coef_arena;
  std::vector<size_t> coef_off(ctx->probs.size(), 0);
  size_t coef_total = 0;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    if (coef_rc[pi] != DSE_OK) return fail(ctx, coef_rc[pi], coef_msg[pi]);
    coef_total += align_up(coef_rows[pi].size() * sizeof(Row), 64);
  }
  coef_arena.host.reserve(coef_total);
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi)
    if (!ctx->probs[pi].side()) coef_off[pi] = coef_arena.place(coef_rows[pi].size() * sizeof(Row));
  parallel_for(ctx->probs.size(), [&](size_t pi) {
    if (!coef_rows[pi].empty())
      std::memcpy(coef_arena.host.data() + coef_off[pi], coef_rows[pi].data(), coef_rows[pi].size() * sizeof(Row));
  });

  pl.phase("coefficients");
  if (int rc = upload_arena(ctx, coef_arena, ctx->d_coef, ctx->lanes[0].stream)) return rc;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    HostProblem& P = ctx->probs[pi];
    if (P.side()) continue;
    P.coef = reinterpret_cast<double2*>(ctx->d_coef.p + coef_off[pi]);
    ctx->h_desc[pi].coef = P.coef;
  }
  pl.phase("coef upload");
  return DSE_OK;
}

int place_output_buffers(dse_ctx* ctx, const EvolvePlan& pl) {
  const int M = pl.M;
  int rc;
  // intermediate outputs of multi-output launches: (M - 1) state vectors per problem, two sets
  // (one per launch parity) when the observables are overlapped
  const size_t xsets = pl.obs_ovl ? 2 : 1;
  size_t xneed = 0, xoff = 0;
  if (M > 1)
    for (auto& P : ctx->probs)
      if (!P.side()) xneed += xsets * ((size_t)(M - 1) << P.n_local);
  if ((rc = ctx->d_xacc.reserve(ctx, xneed, "output accumulator allocation failed", true))) return rc;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const bool use = M > 1 && !ctx->probs[pi].side();
    ctx->h_desc[pi].xacc = use ? ctx->d_xacc.p + xoff : nullptr;
    if (use) xoff += xsets * ((size_t)(M - 1) << ctx->probs[pi].n_local);
  }
  // real-component registers: tables, [a | b] inputs and per-output, per-component sums
  Arena tabs;
  std::vector<size_t> tab_off(ctx->probs.size(), 0), phase_off(ctx->probs.size(), 0);
  size_t need = 0;  // in double2 units
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    ctx->h_desc[pi].rtab = nullptr;
    ctx->h_desc[pi].rin = nullptr;
    ctx->h_desc[pi].racc = nullptr;
    ctx->h_desc[pi].lphase = nullptr;
    ctx->h_desc[pi].lhist = nullptr;
    if (!P.rl) continue;
    RealTab T;
    if ((rc = build_real_table(P, T)) != DSE_OK) return fail(ctx, rc, "real-mode tables: drives not imaginary");
    tab_off[pi] = tabs.add(&T, sizeof(T));
    need += ((size_t)1 + 2 * (size_t)M) << P.n_local;
    if (P.lp) {  // e^{-i beta (t_m - t0)} of every output (the given t_m, not m delta), and the history ring
      const double beta = 0.5 * (P.e_max + P.e_min);
      std::vector<double2> ph(pl.n_t);
      for (int m = 0; m < pl.n_t; ++m) {
        const double a = -beta * (pl.t[m] - pl.t[0]);
        ph[m] = make_double2(std::cos(a), std::sin(a));
      }
      phase_off[pi] = tabs.add(ph.data(), ph.size() * sizeof(double2));
      need += (size_t)kLeapRing << P.n_local;
    }
  }
  if (need == 0) return DSE_OK;
  if ((rc = upload_arena(ctx, tabs, ctx->d_real_tab, ctx->lanes[0].stream))) return rc;
  HIPC(hipStreamSynchronize(ctx->lanes[0].stream));
  if ((rc = ctx->d_real.reserve(ctx, need, "real-mode buffer allocation failed", true))) return rc;
  size_t off = 0;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
    const HostProblem& P = ctx->probs[pi];
    if (!P.rl) continue;
    DevProb& d = ctx->h_desc[pi];
    d.rtab = reinterpret_cast<const RealTab*>(ctx->d_real_tab.p + tab_off[pi]);
    d.rin = reinterpret_cast<double*>(ctx->d_real.p + off);  // [a | b]: 2 x 2^n doubles
    d.racc = ctx->d_real.p + off + ((size_t)1 << P.n_local);
    off += ((size_t)1 + 2 * (size_t)M) << P.n_local;
    if (P.lp) {
      d.lphase = reinterpret_cast<const double2*>(ctx->d_real_tab.p + phase_off[pi]);
      d.lhist = ctx->d_real.p + off;
      off += (size_t)kLeapRing << P.n_local;
    }
  }
  return DSE_OK;
}

// persistent: the hand-off slots of the 2-tile problems and the spanning registers' tables,
// descriptors, slots and flags; then the problem descriptors, complete, to the device
int place_handoff_buffers(dse_ctx* ctx, const EvolvePlan& pl) {
  int rc;
  if (pl.persistent) {
    // hand-off slots of the 2-tile problems: [2 tiles][kXSlots][2^L] amplitudes each
    // (dse_interval.hip)
    size_t need = 0;
    for (auto& P : ctx->probs)
      if (P.n_tiles == 2) need += (size_t)2 * kXSlots << P.L;
    if ((rc = ctx->d_xslots.reserve(ctx, need, "hand-off slot allocation failed", true))) return rc;
    size_t off = 0;
    for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
      const HostProblem& P = ctx->probs[pi];
      ctx->h_desc[pi].xslots = P.n_tiles == 2 ? ctx->d_xslots.p + off : nullptr;
      if (P.n_tiles == 2) off += (size_t)2 * kXSlots << P.L;
    }
    // spanning registers: tables (one arena), descriptors, hand-off slots and flags
    size_t slot_need = 0, flag_need = 0;
    Arena tabs;
    std::vector<size_t> tab_off(ctx->probs.size(), 0);
    for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
      const HostProblem& P = ctx->probs[pi];
      if (!P.span_s) continue;
      const int Ls = P.n_local - P.span_s;
      SpanTab T;
      if (build_span_table(P, Ls, span_rb_for(ctx, Ls), P.span_s, T) != DSE_OK)
        return fail(ctx, DSE_ERR_ARG, "spanning-register tables do not fit (n = " + std::to_string(P.n) + ")");
      tab_off[pi] = tabs.add(&T, sizeof(T));
      slot_need += (size_t)(P.span_s + 1) * kXSlots << P.n_local;
      flag_need += (size_t)kSpanWaves << P.span_s;
    }
    if (flag_need > 0) {
      if ((rc = upload_arena(ctx, tabs, ctx->d_span_tab, ctx->lanes[0].stream))) return rc;
      HIPC(hipStreamSynchronize(ctx->lanes[0].stream));
      if ((rc = ctx->d_span_slots.reserve(ctx, slot_need, "span slot allocation failed", true))) return rc;
      if ((rc = ctx->d_span_flags.reserve(ctx, flag_need, "span flag allocation failed", true))) return rc;
      if ((rc = ctx->d_span.reserve(ctx, ctx->probs.size(), "span descriptor allocation failed", true))) return rc;
      std::vector<SpanDesc> sd(ctx->probs.size());
      size_t so = 0, fo = 0;
      for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
        const HostProblem& P = ctx->probs[pi];
        std::memset(&sd[pi], 0, sizeof(SpanDesc));
        if (!P.span_s) continue;
        sd[pi].tab = reinterpret_cast<const SpanTab*>(ctx->d_span_tab.p + tab_off[pi]);
        sd[pi].slots = ctx->d_span_slots.p + so;
        sd[pi].flags = ctx->d_span_flags.p + fo;
        sd[pi].s = P.span_s;
        sd[pi].L = P.n_local - P.span_s;
        so += (size_t)(P.span_s + 1) * kXSlots << P.n_local;
        fo += (size_t)kSpanWaves << P.span_s;
      }
      HIPC(hipMemcpy(ctx->d_span.p, sd.data(), sd.size() * sizeof(SpanDesc), hipMemcpyHostToDevice));
    }
  }
  HIPC(hipMemcpy(ctx->d_probs, ctx->h_desc.data(), ctx->h_desc.size() * sizeof(DevProb), hipMemcpyHostToDevice));
  return DSE_OK;
}

// Order of a lane's groups, which is the order of `items` and so of every launch: by tile size L;
// within one L the real-component group first, then the spanning groups by descending
// 16 span_L + span_rb, then the mixed group, then the problems of 1 tile, then of 2 (streaming:
// ascending tiles per problem)
struct GroupKey {
  int L;
  GroupKind kind;
  int span_L, span_rb, tiles;  // span_*: kind Span, tiles: kind Tiles; else 0
  bool operator<(const GroupKey& o) const {
    auto rank = [](GroupKind k) { return k == GroupKind::Real ? 0 : k == GroupKind::Span ? 1 : k == GroupKind::Mixed ? 2 : 3; };
    return std::make_tuple(L, rank(kind), -(16 * span_L + span_rb), tiles) <
           std::make_tuple(o.L, rank(o.kind), -(16 * o.span_L + o.span_rb), o.tiles);
  }
};

// per term k of the group's longest series: the items still active and the algorithmic bytes and
// flops of the term's launch (pis in degree order)
void fill_group_terms(const dse_ctx* ctx, LaneGroup& g, const std::vector<int>& pis) {
  const int gdeg = ctx->probs[pis.front()].degree;
  g.active.assign(gdeg + 2, 0);
  g.bytes.assign(gdeg + 2, 0.0);
  g.flops.assign(gdeg + 2, 0.0);
  const double T = (double)(int64_t(1) << g.L);
  for (int k = 0; k <= gdeg + 1; ++k) {
    int64_t c = 0;
    double by = 0.0, fl = 0.0;
    for (int pi : pis) {
      const int K = ctx->probs[pi].degree;
      if (K < k) continue;
      c += ctx->probs[pi].n_tiles;
      fl += (double)ctx->probs[pi].n_tiles * T * ctx->probs[pi].flops_per_amp;
      // read w_{k-1}, read+write w_{k-2}/w_k (48 B/amp), plus acc read+write on update terms
      const bool upd = (k >= 2) && (((k - 1) % 3 == 0) || k == K);
      by += (double)ctx->probs[pi].n_tiles * T * (upd ? 80.0 : 48.0);
    }
    g.active[k] = (int)c;
    g.bytes[k] = by;
    g.flops[k] = fl;
  }
}

// ---- lanes ----
// persistent: 2-tile problems on lane 0 (their workgroup pairs must be co-resident), 1-tile
// problems on lane 1.  streaming: problems by degree dealt round-robin over the lanes.
int assign_lanes(dse_ctx* ctx, EvolvePlan& pl) {
  const bool persistent = pl.persistent;
  // dist shards: one lane, so the RCCL exchanges are stream-ordered with every launch
  int n_big = 0;
  for (auto& P : ctx->probs) n_big += P.side() ? 0 : 1;
  const int n_lanes = pl.n_lanes = pl.any_dist ? 1 : std::max(1, std::min<int>(ctx->n_streams, n_big));
  for (auto& P : ctx->probs) pl.imag_all = pl.imag_all && (P.side() || P.imag);
  // 2-tile interval launches go out in chunks whose workgroups can all be resident at once (the
  // pairs hand off every term): the occupancy query x compute units, even.
  if (persistent) {
    int per_cu = 1;
    if (ctx->coresident > 0) {
      pl.cap = ctx->coresident;
    } else {
      HIPC(interval_occupancy(13, pl.imag_all, &per_cu));
      pl.cap = (int64_t)std::max(1, per_cu) * ctx->n_cu;
    }
    pl.cap = std::max<int64_t>(2, pl.cap / 2 * 2);
  }
  const int64_t cap = pl.cap;
  // Mixed launches (option mixed_launch): the 1- and 2-tile problems of one tile size share one
  // launch per interval instead of one stream each, so the 1-tile problems run in the CUs the
  // light 2-tile problems leave, inside the launch, and never hold a CU the next launch's stiff
  // pairs need.  Only when every 2-tile workgroup fits at once (2P <= cap): the 1-tile problems
  // and the lightest pairs beyond the first cap workgroups are dispatched as CUs free up, and a
  // pair whose partner is still queued waits only for a workgroup that needs no partner.
  std::map<int, std::pair<int64_t, int64_t>> tiles_per_L;  // L -> (1-tile problems, 2-tile problems)
  for (auto& P : ctx->probs)
    if (!P.side() && !P.span_s && !P.rl && P.shard_bits == 0 && (P.n_tiles == 1 || P.n_tiles == 2))
      (P.n_tiles == 1 ? tiles_per_L[P.L].first : tiles_per_L[P.L].second) += 1;
  auto mixed_L = [&](const HostProblem& P) {
    if (!persistent || !ctx->mixed_launch || P.side() || P.span_s || P.rl || P.shard_bits != 0 || P.n_tiles > 2)
      return false;
    const auto it = tiles_per_L.find(P.L);
    return it != tiles_per_L.end() && it->second.first > 0 && it->second.second > 0 &&
           2 * it->second.second <= cap;
  };
  std::vector<int> order;
  for (size_t pi = 0; pi < ctx->probs.size(); ++pi)
    if (!ctx->probs[pi].side()) order.push_back((int)pi);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return ctx->probs[a].degree > ctx->probs[b].degree;
  });
  std::vector<std::map<GroupKey, std::vector<int>>> lane_probs(n_lanes);  // lane -> group -> problems
  for (size_t i = 0; i < order.size(); ++i) {
    const HostProblem& P = ctx->probs[order[i]];
    const bool mixed = mixed_L(P);
    const int Ls = P.n_local - P.span_s;
    GroupKey key = {P.L, GroupKind::Tiles, 0, 0, 0};
    if (P.rl) key.kind = GroupKind::Real;
    else if (P.span_s) key.kind = GroupKind::Span, key.span_L = Ls, key.span_rb = span_rb_for(ctx, Ls);
    else if (mixed) key.kind = GroupKind::Mixed;
    else key.tiles = (int)P.n_tiles;
    int lane = (int)(i % n_lanes);
    if (persistent) lane = (P.n_tiles == 2 || n_lanes == 1 || mixed || P.span_s || P.rl) ? 0 : 1;
    // partial span: the spanned registers on a lane of their own, concurrent with k_interval's
    if (persistent && P.span_s && !pl.all_span && n_lanes >= 2) lane = n_lanes >= 3 ? 2 : 1;
    // shards of one register read each other's vectors: same lane, hence the same launches
    if (P.shard_bits > 0 && !P.dist) lane = P.group_first % n_lanes;
    lane_probs[lane][key].push_back(order[i]);
  }
  std::vector<int2>& items = pl.items;
  items.reserve(ctx->total_items);
  ctx->item_pos.assign(ctx->probs.size(), 0);
  for (int li = 0; li < (int)ctx->lanes.size(); ++li) {
    Lane& ln = ctx->lanes[li];
    ln.groups.clear();
    ln.max_deg = 0;
    if (li >= n_lanes) continue;
    for (auto& kv : lane_probs[li]) {
      LaneGroup g;
      g.L = kv.first.L;
      g.kind = kv.first.kind;
      g.tiles = kv.first.tiles;
      g.span_L = kv.first.span_L;
      g.span_rb = kv.first.span_rb;
      g.off = (int64_t)items.size();
      for (int pi : kv.second) {  // already in degree order
        ctx->item_pos[pi] = (int64_t)items.size();
        for (int64_t tt = 0; tt < ctx->probs[pi].n_tiles; ++tt) items.push_back(make_int2(pi, (int)tt));
        ln.max_deg = std::max(ln.max_deg, ctx->probs[pi].degree);
      }
      g.count = (int64_t)items.size() - g.off;
      g.wht_groups = persistent ? 0 : ctx->probs[kv.second.front()].wht_groups;
      for (int pi : kv.second)
        if (ctx->probs[pi].wht_groups != g.wht_groups) g.wht_groups = 0;
      if (g.wht_groups)
        for (int pi : kv.second) {
          const HostProblem& P = ctx->probs[pi];
          if (P.shard_bits == 0) continue;
          const int first = P.dist ? pi : P.group_first;
          if (P.dist || P.shard_rank == 0) g.wht_regs.push_back({first, P.degree});
        }
      fill_group_terms(ctx, g, kv.second);
      ln.groups.push_back(std::move(g));
    }
    pl.max_deg = std::max(pl.max_deg, ln.max_deg);
  }
  HIPC(hipMemcpy(ctx->d_items, items.data(), items.size() * sizeof(int2), hipMemcpyHostToDevice));
  return DSE_OK;
}

// Interval-kernel order of 2-tile groups: the two tiles of a problem exchange data every
// term, so place them 8 blocks apart -- blocks b and b + 8 land on one XCD under the
// observed round-robin dispatch and then hand off through that XCD's L2 (speed only; the
// hand-off protocol does not depend on placement).  Chunks of one launch are multiples of 16.
int order_interval_items(dse_ctx* ctx, const EvolvePlan& pl) {
  const std::vector<int2>& items = pl.items;
  const int64_t cap = pl.cap;
  std::vector<int2> iv = items;
  for (auto& ln : ctx->lanes)
    for (auto& g : ln.groups) {
      if (g.kind == GroupKind::Mixed) {
        // mixed group: the stiffest pairs first (as many as fit beside the 1-tile problems), then
        // the 1-tile problems, then the remaining pairs, each segment in degree order; pairs in
        // blocks of 16 with their tiles 8 apart, as below
        std::vector<int2> pr, sg;
        for (int64_t i = 0; i < g.count; ++i) {
          const int2 e = items[g.off + i];
          (ctx->probs[e.x].n_tiles == 2 ? pr : sg).push_back(e);
        }
        const int64_t np = (int64_t)pr.size() / 2, ns = (int64_t)sg.size();
        const int64_t h = std::min<int64_t>(np, std::max<int64_t>(0, (cap - ns) / 2));
        int64_t o = g.off;
        auto put_pairs = [&](int64_t p0, int64_t p1) {
          for (int64_t b0 = p0; b0 < p1; b0 += 8) {
            const int64_t m = std::min<int64_t>(8, p1 - b0);
            if (ctx->xcd_pairs) {
              for (int64_t i = 0; i < m; ++i) {
                iv[o + i] = pr[2 * (b0 + i)];
                iv[o + m + i] = pr[2 * (b0 + i) + 1];
              }
            } else {
              for (int64_t i = 0; i < 2 * m; ++i) iv[o + i] = pr[2 * b0 + i];
            }
            o += 2 * m;
          }
        };
        put_pairs(0, h);
        for (const int2& e : sg) iv[o++] = e;
        put_pairs(h, np);
        continue;
      }
      if (g.kind != GroupKind::Tiles || g.tiles != 2 || !ctx->xcd_pairs) continue;
      for (int64_t off = 0; off < g.count; off += cap) {
        const int64_t cnt = std::min<int64_t>(cap, g.count - off);
        for (int64_t b0 = 0; b0 < cnt; b0 += 16) {
          const int64_t m = std::min<int64_t>(16, cnt - b0) / 2;  // problems in this block
          for (int64_t i = 0; i < m; ++i) {
            iv[g.off + off + b0 + i] = items[g.off + off + b0 + 2 * i];
            iv[g.off + off + b0 + m + i] = items[g.off + off + b0 + 2 * i + 1];
          }
        }
      }
    }
  HIPC(hipMemcpy(ctx->d_items_iv, iv.data(), iv.size() * sizeof(int2), hipMemcpyHostToDevice));
  return DSE_OK;
}

// the problems of a group, in item order
std::vector<int> group_problems(const EvolvePlan& pl, const LaneGroup& g) {
  std::vector<int> pis;
  for (int64_t i = 0; i < g.count; ++i) {
    const int2 e = pl.items[g.off + i];
    if (pis.empty() || pis.back() != e.x) pis.push_back(e.x);
  }
  return pis;
}

// spanning groups: launch items (problem, tile); the tiles of one register 8 items apart, so
// under the round-robin dispatch of workgroups to the 8 XCDs they share one XCD's L2 (speed
// only), in blocks of 8 registers padded with items x = -1 (return at once)
int order_span_items(dse_ctx* ctx, EvolvePlan& pl) {
  std::vector<int2>& sitems = pl.span_items;
  for (auto& ln : ctx->lanes)
    for (auto& g : ln.groups) {
      if (g.kind != GroupKind::Span) continue;
      const std::vector<int> pis = group_problems(pl, g);
      g.span_off = (int64_t)sitems.size();
      int per_cu = 1;
      HIPC(span_occupancy(g.span_L, g.span_rb, pl.imag_all, &per_cu));
      const int64_t resident = (int64_t)std::max(1, per_cu) * ctx->n_cu;
      g.span_cuts.assign(1, 0);
      g.span_am.assign(1, 0.0);
      g.span_fl.assign(1, 0.0);
      for (size_t b0 = 0; b0 < pis.size(); b0 += 8) {
        int s = 0;  // the block's widest register sets its size (span_tile mixes 13 and 14 qubits)
        for (size_t i = b0; i < std::min(pis.size(), b0 + 8); ++i) s = std::max(s, ctx->probs[pis[i]].span_s);
        const size_t base = sitems.size();
        if ((int64_t)(base + ((size_t)8 << s)) - g.span_off - g.span_cuts.back() > resident &&
            (int64_t)base - g.span_off > g.span_cuts.back()) {
          g.span_cuts.push_back((int64_t)base - g.span_off);  // this block starts the next launch
          g.span_am.push_back(0.0);
          g.span_fl.push_back(0.0);
        }
        for (size_t i = b0; i < std::min(pis.size(), b0 + 8); ++i) {
          const HostProblem& P = ctx->probs[pis[i]];
          g.span_am.back() += std::ldexp(1.0, P.n_local) * P.degree;
          g.span_fl.back() += std::ldexp(1.0, P.n_local) * P.degree * P.flops_per_amp;
        }
        sitems.resize(base + ((size_t)8 << s), make_int2(-1, 0));
        for (size_t i = b0; i < std::min(pis.size(), b0 + 8); ++i)
          for (int h = 0; h < (1 << ctx->probs[pis[i]].span_s); ++h)
            sitems[base + (size_t)h * 8 + (i - b0)] = make_int2(pis[i], h);
      }
      g.span_count = (int64_t)sitems.size() - g.span_off;
      g.span_cuts.push_back(g.span_count);
    }
  return DSE_OK;
}

// real-component groups: items (problem, component) in degree order, then (problem, 0) per
// problem for the combine launch
void order_real_items(dse_ctx* ctx, EvolvePlan& pl) {
  std::vector<int2>& ritems = pl.real_items;
  for (auto& ln : ctx->lanes)
    for (auto& g : ln.groups) {
      if (g.kind != GroupKind::Real) continue;
      const std::vector<int> pis = group_problems(pl, g);
      g.real_off = (int64_t)ritems.size();
      if (pl.leap_dt > 0.0) {
        // the leap path: p_m alone; item (problem, g) runs the launch's outputs 2 g, 2 g + 1.  The longest
        // series first (the last pair's), each pair's items in degree order, so a launch of n outputs
        // takes the last ceil(n / kMaxOut) * |pis| items
        for (int g2 = (pl.M + kMaxOut - 1) / kMaxOut - 1; g2 >= 0; --g2)
          for (int pi : pis) ritems.push_back(make_int2(pi, g2 | (ctx->probs[pi].leap_k[g2] << kLeapKShift)));
      } else {
        for (int pi : pis) ritems.push_back(make_int2(pi, 0)), ritems.push_back(make_int2(pi, 1));
      }
      g.real_count = (int64_t)ritems.size() - g.real_off;
      g.real_poff = (int64_t)ritems.size();
      for (int pi : pis) ritems.push_back(make_int2(pi, 0));
      g.real_np = (int64_t)pis.size();
    }
}

// the real and span items (persistent only) to the device; the hand-off flags and the error word, zeroed
int upload_items_and_flags(dse_ctx* ctx, EvolvePlan& pl) {
  int rc;
  if (!pl.real_items.empty()) {
    if ((rc = ctx->d_real_items.reserve(ctx, pl.real_items.size(), "real item allocation failed"))) return rc;
    HIPC(hipMemcpy(ctx->d_real_items.p, pl.real_items.data(), pl.real_items.size() * sizeof(int2), hipMemcpyHostToDevice));
  }
  if (!pl.span_items.empty()) {
    if ((rc = ctx->d_span_items.reserve(ctx, pl.span_items.size(), "span item allocation failed"))) return rc;
    HIPC(hipMemcpy(ctx->d_span_items.p, pl.span_items.data(), pl.span_items.size() * sizeof(int2), hipMemcpyHostToDevice));
  }
  if (pl.persistent) {
    const size_t need = 2 * kIvWaves * ctx->probs.size() + 1;  // flags, error word
    if ((rc = ctx->d_flags.reserve(ctx, need, "flag allocation failed"))) return rc;
    HIPC(hipMemset(ctx->d_flags.p, 0, need * sizeof(int)));
    pl.d_err = ctx->d_flags.p + 2 * kIvWaves * ctx->probs.size();
  }
  ctx->d_err_cur = pl.d_err;  // checked by every flush_partials (reset by dse_evolve on return)
  return DSE_OK;
}

// ---- psi(t0) = |psi0>, or the register's stored or product state ----
int write_initial_states(dse_ctx* ctx, const EvolvePlan& pl) {
  hipStream_t st0 = ctx->lanes[0].stream;
  std::vector<BasisInit> init;
  std::vector<HostProblem*> custom;  // registers (shards) that start from a stored or product state
  uint64_t max_amps = 0;
  for (auto& P : ctx->probs) {
    // the re-run after a hand-off timeout keeps the dense registers' first-pass results, whose
    // final state k_dense_final wrote into buf[0]
    if (ctx->rerun && P.dn) continue;
    if (P.init_kind) {
      custom.push_back(&P);
      continue;
    }
    BasisInit e;
    e.ptr = P.buf[0];
    e.n = uint64_t(1) << P.n_local;
    // the shard holding psi0 (every unsharded register)
    e.one_at = ((P.psi0 >> P.n_local) == (uint64_t)P.shard_rank)
                   ? (int64_t)(P.psi0 & ((uint64_t(1) << P.n_local) - 1)) : -1;
    init.push_back(e);
    max_amps = std::max(max_amps, e.n);
  }
  if (int rc = ctx->d_init.reserve(ctx, init.size(), "initial-state list allocation failed")) return rc;
  if (ctx->dbg & 2) {
    for (auto& e : init) {
      HIPC(hipMemsetAsync(e.ptr, 0, e.n * sizeof(double2), st0));
      static const double2 one = {1.0, 0.0};
      if (e.one_at >= 0) HIPC(hipMemcpyAsync(e.ptr + e.one_at, &one, sizeof(double2), hipMemcpyHostToDevice, st0));
    }
  } else {
    HIPC(hipMemcpyAsync(ctx->d_init.p, init.data(), init.size() * sizeof(BasisInit), hipMemcpyHostToDevice, st0));
    for (size_t i0 = 0; i0 < init.size(); i0 += 65535)
      HIPC(launch_basis_init(ctx->d_init.p + i0, (int)std::min<size_t>(65535, init.size() - i0), max_amps, st0));
  }
  // custom psi(t0) (the re-run after a hand-off timeout comes through here again: the same state)
  for (HostProblem* P : custom) {
    if (P->init_kind == 1)
      HIPC(hipMemcpyAsync(P->buf[0], P->init_state, (size_t(1) << P->n_local) * sizeof(double2),
                          hipMemcpyDeviceToDevice, st0));
    else
      HIPC(launch_product_state(P->buf[0], P->d_init_amp, P->n, P->n_local, (uint64_t)P->shard_rank, st0));
  }
  for (auto& ln : ctx->lanes)  // real-component registers: [a | b] = [e_x0 | 0], or split from buf[0]
    for (auto& g : ln.groups)
      if (g.kind == GroupKind::Real && pl.leap_dt > 0.0) {  // p_0 = e_x0 and the history's entry 0
        HIPC(launch_leap_init(ctx->d_probs, ctx->d_real_items.p + g.real_poff, (int)g.real_np, st0));
      } else if (g.kind == GroupKind::Real) {
        HIPC(launch_real_init(ctx->d_probs, ctx->d_real_items.p + g.real_poff, (int)g.real_np, st0));
        if (!custom.empty())
          HIPC(launch_real_split(ctx->d_probs, ctx->d_real_items.p + g.real_poff, (int)g.real_np, st0));
      }
  HIPC(hipStreamSynchronize(st0));
  return DSE_OK;
}

// the engines beside the per-interval launches: small registers, dense registers, matrix mode
int run_side_engines(dse_ctx* ctx, EvolvePlan& pl) {
  int rc;
  if (pl.any_small && (rc = small_launch(ctx, pl.t, pl.n_t, pl.tol, &pl.small_happl, &pl.small_launches))) return rc;
  // (the re-run after a hand-off timeout keeps the first pass's dense results: dense_run completed
  // and wrote them before any interval launch, and its register choice depends only on t)
  if (pl.any_dense && !ctx->rerun && (rc = dense_run(ctx, pl.t, pl.n_t, pl.obs_out, &pl.dense_ms, &pl.dense_eig_ms)))
    return rc;
  if (pl.matrix_pi >= 0 &&
      (rc = matrix_run(ctx, pl.matrix_pi, pl.t, pl.n_t, pl.matrix_dt, pl.tol, pl.obs_out, &pl.matrix_happl)))
    return rc;
  return DSE_OK;
}

// output slots per flush: what every arena in use holds under kPartialCapBytes (for the pair
// arena one slot fits the cap: obs_family_refusal); the arenas; the timing events
int size_obs_chunks(dse_ctx* ctx, EvolvePlan& pl) {
  const int64_t tiles = ctx->total_items;
  const int n_max = widest_register(ctx);
  int rc;
  pl.chunk = partial_chunk(tiles * 64, pl.M, pl.n_t);
  for (ObsFamily f : kObsLaunchOrder)
    if (ctx->fam[f].on)
      pl.chunk = std::min(pl.chunk, partial_chunk(tiles * kObsFamilies[f].stride(ctx, n_max) * 8, pl.M, pl.n_t));
  for (ObsFamily f : kObsLaunchOrder)
    if (ctx->fam[f].on && (rc = ensure_family_partial(ctx, f, pl.chunk))) return rc;
  if ((rc = ensure_partial(ctx, pl.chunk))) return rc;
  if (ctx->time_every > 0)
    for (auto& ln : ctx->lanes) {
      // timed launches per interval and pool: one per term and group (streaming), one per
      // co-resident chunk and group (persistent); records beyond the pool are skipped, not timed
      size_t need = 1;
      for (const auto& g : ln.groups)
        need += pl.persistent ? (g.kind == GroupKind::Span ? g.span_cuts.size() - 1 : (size_t)((g.count + pl.cap - 1) / pl.cap))
                              : (size_t)(ln.max_deg + 1);
      if ((rc = ensure_events(ctx, ln, need))) return rc;
    }
  return DSE_OK;
}

// The aggregate, site and pair observables of one lane group: state role bsel of its problems into
// arena slot `slot`; with n_out > 1 outputs j < n_out - 1 from the intermediate accumulators of
// parity xq into the slots before it (out_stride_slots = 1)
int launch_group_obs(dse_ctx* ctx, const LaneGroup& g, int bsel, size_t slot, int n_out,
                            size_t out_stride_slots, int xq, hipStream_t st) {
  const size_t at = slot * ctx->total_items + g.off, stride = out_stride_slots * (size_t)ctx->total_items;
  HIPC(launch_obs(g.L, ctx->d_probs, ctx->d_items + g.off, (int)g.count, bsel, ctx->d_partial.p + at * 8, st, n_out,
                  stride * 8, xq));
  for (ObsFamily f : kObsLaunchOrder) {
    const ObsFamilyState& A = ctx->fam[f];
    if (A.on)
      HIPC(kObsFamilies[f].launch(g.L, ctx->d_probs, ctx->d_items + g.off, (int)g.count, bsel, A.d_partial.p + at * A.S,
                                  A.S, st, n_out, stride * A.S, xq));
  }
  return DSE_OK;
}

// observables of n_out consecutive output slots (one launch per lane group): outputs
// j < n_out - 1 from the intermediate accumulators, the last from state role bsel_q
// obs_ovl: on each lane's obs_stream behind the lane's interval launches of parity xq (event
// ev_iv[xq]), then ev_obs[xq] for the launches two groups later, which rewrite these buffers
int launch_all_obs(dse_ctx* ctx, const EvolvePlan& pl, int bsel_q, size_t slot, int n_out, int xq) {
  for (auto& ln : ctx->lanes) {
    if (ln.groups.empty()) continue;
    hipStream_t os = pl.obs_ovl ? ln.obs_stream : ln.stream;
    if (pl.obs_ovl) {
      HIPC(hipEventRecord(ln.ev_iv[xq], ln.stream));
      HIPC(hipStreamWaitEvent(os, ln.ev_iv[xq], 0));
    }
    for (auto& g : ln.groups)
      if (int rc = launch_group_obs(ctx, g, bsel_q, slot, n_out, 1, xq, os)) return rc;
    if (pl.obs_ovl) {
      HIPC(hipEventRecord(ln.ev_obs[xq], os));
      ln.obs_pending[xq] = true;
    }
  }
  return DSE_OK;
}

// Persistent: all K terms of the intervals of G in one launch of lane group g; 2-tile groups in
// co-resident chunks of cap items; mixed groups in one launch; spanning registers in one k_span
// launch per chunk of span_cuts (each chunk's registers' tiles all resident at once: the cuts are
// sized to the chip's resident capacity), flags zeroed first
int launch_persistent_group(dse_ctx* ctx, EvolvePlan& pl, Lane& ln, size_t li, LaneGroup& g,
                                   const IntervalGroup& G, int gi) {
  const int T = 1 << g.L, q = gi & 1, pool = gi & 1, set = G.set;
  const bool timed = ctx->time_every > 0 && (gi % ctx->time_every) == 0;
  const bool span = g.kind == GroupKind::Span, real = g.kind == GroupKind::Real;
  if (span) HIPC(hipMemsetAsync(ctx->d_span_flags.p, 0, ctx->d_span_flags.cap * sizeof(int), ln.stream));
  else if (g.kind == GroupKind::Mixed || (g.kind == GroupKind::Tiles && g.tiles != 1))
    HIPC(zero_flags(ctx->d_items + g.off, (int)g.count, ctx->d_flags.p, ln.stream));
  auto launch_g = [&](int64_t off, int cnt) -> hipError_t {
    if (real && pl.leap_dt > 0.0) {  // only the workgroups that have outputs (order_real_items)
      const int64_t cnt_l = (G.n_out + kMaxOut - 1) / kMaxOut * g.real_np;
      return launch_real(ctx->d_probs, ctx->d_real_items.p + g.real_off + g.real_count - cnt_l, (int)cnt_l, set, G.n_out,
                         1, ln.stream);
    }
    if (real)
      return launch_real(ctx->d_probs, ctx->d_real_items.p + g.real_off, (int)g.real_count, set, G.n_out, 0, ln.stream);
    if (span)  // chunk [off, off + cnt) of the group's span launches
      return launch_span(g.span_L, g.span_rb, pl.imag_all, ctx->d_probs, ctx->d_span.p,
                         ctx->d_span_items.p + g.span_off + g.span_cuts[off],
                         (int)(g.span_cuts[off + cnt] - g.span_cuts[off]), q, set, G.n_out, pl.d_err, ctx->hk,
                         ln.stream);
    return launch_interval(g.L, pl.imag_all, ctx->d_probs, ctx->d_items_iv + g.off + off, cnt, q, set, G.n_out,
                           ctx->d_flags.p, pl.d_err, ctx->hk, ln.stream);
  };
  // span: off / cnt count chunks of span_cuts, not items
  const int64_t gcap = span ? 1 : (g.kind == GroupKind::Tiles && g.tiles == 2) ? pl.cap : g.count;
  const int64_t gn = span ? (int64_t)g.span_cuts.size() - 1 : g.count;
  for (int64_t off = 0; off < gn; off += gcap) {
    const int cnt = (int)std::min<int64_t>(gcap, gn - off);
    double fl = 0.0, am = 0.0;
    if (span) {  // the chunk's registers
      am = g.span_am[off];
      fl = g.span_fl[off];
    } else {
      for (int64_t i = off; i < off + cnt; ++i) {
        const HostProblem& P = ctx->probs[pl.items[g.off + i].x];
        am += (double)T * P.degree;
        fl += (double)T * P.degree * P.flops_per_amp;
      }
    }
    if (int rc = pl.timer.run(ctx, ln, li, pool, timed, {fl, 0.0, am}, [&]() -> int {
          HIPC(launch_g(off, cnt));
          return DSE_OK;
        }))
      return rc;
    pl.launches += 1.0;
    pl.amp_updates += am;
    pl.all_flops += fl;
  }
  // real-component registers: psi of every output (computational frame) and the next [a | b]
  if (real && pl.leap_dt > 0.0)  // the leap path: the outputs by the time recurrence, and the next p_m
    HIPC(launch_leap_combine(ctx->d_probs, ctx->d_real_items.p + g.real_poff, (int)g.real_np, q, G.n_out, G.m0, ln.stream));
  else if (real)
    HIPC(launch_real_combine(ctx->d_probs, ctx->d_real_items.p + g.real_poff, (int)g.real_np, q, G.n_out, ln.stream));
  return DSE_OK;
}

// Streaming: the interval of G term by term, one launch of the step kernels or one pass set of the
// Walsh-Hadamard engine per term over the items still active
int launch_streaming_group(dse_ctx* ctx, EvolvePlan& pl, Lane& ln, size_t li, LaneGroup& g,
                                  const IntervalGroup& G, int gi) {
  const int T = 1 << g.L, q = gi & 1, pool = gi & 1, set = G.set;
  const bool timed = ctx->time_every > 0 && (gi % ctx->time_every) == 0;
  int rc;
  if (pl.any_dist_step && (rc = dist_exchange(ctx, q ? 2 : 0, 1, ln.stream))) return rc;
  // fused FINAL + FIRST for the whole evolve, or not at all: a group with any partitioned
  // register (index swaps around MID) runs unfused, also on the terms past that register's degree
  const bool fuse = ctx->wht_fuse && g.wht_regs.empty();
  auto step = [&](int mode, int na, int k) -> int {
    if (g.wht_groups) {
      std::vector<int> regs;
      for (const auto& rg : g.wht_regs)
        if (rg.second >= k) regs.push_back(rg.first);
      return wht_run(ctx, g.L, g.wht_groups, {{ctx->d_items + g.off, na}}, regs, fuse, mode, k, q, set,
                     ln.stream);
    }
    HIPC(launch_step(g.L, mode, ctx->d_probs, ctx->d_items + g.off, na, k, q, set, ln.stream));
    return DSE_OK;
  };
  if ((rc = step(MODE_FIRST, g.active[1], 1))) return rc;
  for (int k = 2; k < (int)g.active.size(); ++k) {
    const int na = g.active[k];
    if (na <= 0) break;
    if (pl.any_dist_step && (rc = dist_exchange(ctx, ((k - 1) & 1) ? 1 : (q ? 2 : 0), k, ln.stream))) return rc;
    if ((rc = pl.timer.run(ctx, ln, li, pool, timed, {g.flops[k], g.bytes[k], (double)na * T},
                           [&]() { return step(MODE_GEN, na, k); })))
      return rc;
    pl.launches += 1.0;
    pl.amp_updates += (double)na * T;
    pl.all_bytes += g.bytes[k];
    pl.all_flops += g.flops[k];
  }
  return DSE_OK;
}

int flush_slots(dse_ctx* ctx, EvolvePlan& pl) {
  if (int rc = flush_partials(ctx, pl.slot, pl.t_flushed, pl.n_t, pl.obs_out, &pl.dist_raw)) return rc;
  pl.t_flushed += pl.slot;
  pl.slot = 0;
  return DSE_OK;
}

// observables of psi(t0), then per group of intervals: every lane's launches, the observables of
// the group's outputs, a flush when the arenas are full
int run_intervals(dse_ctx* ctx, EvolvePlan& pl) {
  int rc;
  pl.timer.recs.assign(ctx->lanes.size() * 2, {});
  for (auto& ln : ctx->lanes) ln.obs_pending[0] = ln.obs_pending[1] = false;
  pl.dist_raw.assign(pl.any_dist ? ctx->probs.size() * (size_t)pl.n_t * 7 : 0, 0.0);
  if (pl.any_dist && (rc = dist_exchange(ctx, 0, 0, ctx->lanes[0].stream))) return rc;
  if ((rc = launch_all_obs(ctx, pl, 0, pl.slot++, 1, 1))) return rc;
  for (int gi = 0; gi < (int)pl.groups.size(); ++gi) {
    const IntervalGroup& G = pl.groups[gi];
    const int q = gi & 1;
    for (size_t li = 0; li < ctx->lanes.size(); ++li) {
      Lane& ln = ctx->lanes[li];
      if (ln.groups.empty()) continue;
      if ((rc = pl.timer.drain(ctx, ln, li, q))) return rc;
      if (pl.obs_ovl && ln.obs_pending[q]) {  // the observables that read what this group rewrites
        HIPC(hipStreamWaitEvent(ln.stream, ln.ev_obs[q], 0));
        ln.obs_pending[q] = false;
      }
      for (auto& g : ln.groups)
        if ((rc = pl.persistent ? launch_persistent_group(ctx, pl, ln, li, g, G, gi)
                                : launch_streaming_group(ctx, pl, ln, li, g, G, gi)))
          return rc;
    }
    // new psi of every problem sits in acc(q) = buf[q ? 0 : 2]; outputs j < n_out - 1 of a
    // multi-output launch in the intermediate accumulators
    if (pl.any_dist && (rc = dist_exchange(ctx, q ? 0 : 2, 0, ctx->lanes[0].stream))) return rc;
    // the group's outputs share one launch: one chunk
    if (pl.slot + G.n_out > pl.chunk && (rc = flush_slots(ctx, pl))) return rc;
    if (ctx->dbg & 1) {  // one output per launch, on the lanes' own streams
      for (int j = 0; j < G.n_out; ++j)
        for (auto& ln : ctx->lanes)
          for (auto& g : ln.groups)
            if ((rc = launch_group_obs(ctx, g, j == G.n_out - 1 ? (q ? 0 : 2) : 3 + j, pl.slot + j, 1, 0, q, ln.stream)))
              return rc;
    } else if ((rc = launch_all_obs(ctx, pl, q ? 0 : 2, pl.slot, G.n_out, q))) {
      return rc;
    }
    pl.slot += G.n_out;
    if (pl.slot == pl.chunk && (rc = flush_slots(ctx, pl))) return rc;
  }
  pl.phase("launch loop");
  return DSE_OK;
}

// the last flush, the timing events, every stream, the small engine's results, the hand-off error
// word, the sums of the registers partitioned over processes; then the context's record of the call
int finish_evolve(dse_ctx* ctx, EvolvePlan& pl) {
  int rc;
  if (pl.slot > 0 && (rc = flush_slots(ctx, pl))) return rc;
  for (size_t li = 0; li < ctx->lanes.size(); ++li)
    for (int pool = 0; pool < 2; ++pool)
      if ((rc = pl.timer.drain(ctx, ctx->lanes[li], li, pool))) return rc;
  if ((rc = sync_all(ctx))) return rc;
  if ((rc = small_gather(ctx, pl.n_t, pl.obs_out))) return rc;
  pl.phase("flush/drain");
  if (pl.persistent && pl.any_big) {
    int herr = 0;
    HIPC(hipMemcpy(&herr, pl.d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (herr) return kRcHandoffTimeout;
  }
  if (pl.any_dist) {  // sums over all shards of the register, then normalisation (finish_obs)
    if ((rc = xchg_allreduce_host(ctx, pl.dist_raw.data(), pl.dist_raw.size(), ctx->lanes[0].stream))) return rc;
    for (size_t pi = 0; pi < ctx->probs.size(); ++pi) {
      if (!ctx->probs[pi].dist) continue;
      for (int ti = 0; ti < pl.n_t; ++ti)
        finish_obs(ctx->probs[pi], pl.dist_raw.data() + (pi * (size_t)pl.n_t + ti) * 7,
                   pl.obs_out + pi * DSE_N_OBS * (size_t)pl.n_t + ti, (size_t)pl.n_t);
    }
  }
  pl.phase("tail");
  ctx->last_q = (int)pl.groups.size() & 1;
  for (auto& P : ctx->probs) P.final_bsel = P.side() ? 0 : (ctx->last_q ? 2 : 0);
  ctx->evolved = true;
  ctx->leap_problems = 0;
  for (const auto& P : ctx->probs) ctx->leap_problems += P.lp ? 1 : 0;
  for (ObsFamily f : kObsLaunchOrder) {
    ObsFamilyState& A = ctx->fam[f];
    if (!A.on) continue;
    A.nt = pl.n_t;  // the store is complete: the getter may read it
    A.problems = 0;
    for (const auto& P : ctx->probs) A.problems += obs_record(ctx, f, P) ? 1 : 0;
  }
  return DSE_OK;
}

int fill_stats(dse_ctx* ctx, const EvolvePlan& pl, dse_stats* stats) {
  const LaunchTimer& tm = pl.timer;
  double happl = pl.small_happl + pl.matrix_happl;
  int n_dense = 0, n_span = 0, n_real = 0, n_custom = 0, max_deg = pl.max_deg;
  for (const auto& P : ctx->probs) {
    if (!P.side()) happl += (double)P.degree * (int)pl.groups.size();
    n_dense += P.dn ? 1 : 0;
    n_span += P.span_s ? 1 : 0;
    n_real += (P.rl && !P.lp) ? 1 : 0;  // (the leap path's registers: dse_leap_problems)
    // a loopback partitioned register counts once (its shard 0)
    n_custom += (P.init_kind && (P.dist || P.shard_rank == 0)) ? 1 : 0;
    if (P.sm || P.mx) max_deg = std::max(max_deg, P.degree);
  }
  std::memset(stats, 0, sizeof(*stats));
  stats->h_applications = happl;
  stats->amplitude_updates = pl.amp_updates;
  stats->step_bytes = pl.all_bytes;
  stats->h_flops = pl.all_flops;
  stats->timed_flops = tm.flops;
  stats->timed_amp_terms = tm.amp_terms;
  stats->mode = pl.matrix_pi >= 0 ? 5 : (!pl.any_big ? (pl.any_dense ? 4 : 3) : (pl.persistent ? 1 : (pl.used_wht ? 2 : 0)));
  stats->dense_problems = n_dense;
  stats->span_problems = n_span;
  stats->real_problems = n_real;
  stats->eig_fallbacks = ctx->eig_fallbacks.load();
  stats->dense_ms = pl.dense_ms;
  stats->dense_eig_ms = pl.dense_eig_ms;
  stats->dense_nufft_problems = pl.any_dense ? ctx->nufft_problems : 0;
  stats->site_obs_problems = obs_family_problems(ctx, kSite);
  stats->dense_output_ms = pl.any_dense ? ctx->dense_out_ms : 0.0;
  stats->custom_init_problems = n_custom;
  stats->step_kernel_ms = tm.launches > 0 ? tm.step_ms : -1.0;
  stats->step_launches = pl.launches + pl.small_launches;
  stats->timed_launches = tm.launches;
  stats->timed_bytes = tm.bytes;
  stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - pl.wall0).count();
  stats->max_degree = max_deg;
  stats->n_intervals = pl.n_t - 1;
  stats->tile_bits = ctx->probs.empty() ? 0 : ctx->probs.front().L;
  stats->streams = pl.n_lanes;
  stats->outputs_per_launch = pl.M;
  stats->handoff_fallbacks = ctx->handoff_fallbacks;
  stats->exchange_bytes = ctx->xbytes;
  if (int rc = xt_sum(ctx)) return rc;
  stats->exchange_ms = ctx->xms;
  stats->lane0_kernel_ms = tm.lane0_ms;
  stats->lane0_launches = tm.lane0_launches;
  stats->lane0_amp_terms = tm.lane0_amp_terms;
  if (pl.matrix_pi >= 0) {
    stats->matrix_build_ms = ctx->mx_build_ms;
    stats->matrix_products_ms = ctx->mx_products_ms;
    stats->matrix_products = ctx->mx_products;
    stats->matrix_bytes_per_product = ctx->mx_bytes_per_product;
  }
  return DSE_OK;
}

int evolve_impl(dse_ctx* ctx, const double* t, int n_t, double tol, double* obs_out, dse_stats* stats) {
  EvolvePlan pl;
  pl.t = t, pl.n_t = n_t, pl.tol = tol, pl.obs_out = obs_out;
  pl.wall0 = pl.tmark = std::chrono::steady_clock::now();
  int rc;
  if ((rc = check_times(ctx, pl))) return rc;
  HIPC(hipSetDevice(ctx->device));
  // timing-event records of an earlier call that ended early (an error, or the hand-off timeout
  // dse_evolve re-runs) are dropped: their per-launch counters lived in that call
  for (auto& ln : ctx->lanes) ln.ev_used[0] = ln.ev_used[1] = 0;
  if ((rc = prepare(ctx))) return rc;
  ctx->xbytes = 0.0;
  ctx->xms = 0.0;
  ctx->xev_used = 0;
  pl.phase("prepare");
  if ((rc = set_unit_families_on(ctx, false)) || (rc = choose_engines(ctx, pl))) return rc;
  choose_span(ctx, pl);
  choose_real(ctx, pl);
  choose_leap(ctx, pl);
  if ((rc = choose_wht(ctx, pl))) return rc;
  choose_outputs_per_launch(ctx, pl);
  if ((rc = group_intervals(ctx, pl))) return rc;
  pl.phase("groups");
  if ((rc = build_coefficients(ctx, pl))) return rc;
  if ((rc = place_output_buffers(ctx, pl)) || (rc = place_handoff_buffers(ctx, pl))) return rc;
  if ((rc = assign_lanes(ctx, pl))) return rc;
  if (pl.persistent) {
    if ((rc = order_interval_items(ctx, pl)) || (rc = order_span_items(ctx, pl))) return rc;
    order_real_items(ctx, pl);
  }
  if ((rc = upload_items_and_flags(ctx, pl))) return rc;
  pl.phase("lanes/items");
  if ((rc = write_initial_states(ctx, pl)) || (rc = run_side_engines(ctx, pl))) return rc;
  pl.phase("psi0/small");
  if ((rc = size_obs_chunks(ctx, pl)) || (rc = run_intervals(ctx, pl)) || (rc = finish_evolve(ctx, pl))) return rc;
  return stats ? fill_stats(ctx, pl, stats) : DSE_OK;
}

}  // namespace

extern "C" {

int dse_evolve(dse_ctx* ctx, const double* t, int n_t, double tol, double* obs_out, dse_stats* stats) {
  if (!ctx) return DSE_ERR_ARG;
  ctx->handoff_fallbacks = 0;
  ctx->eig_fallbacks = 0;
  // the site and pair observables of an earlier evolve end here, whatever becomes of this call (an
  // argument error before any work, a failure half way): their getters are DSE_ERR_STATE until an
  // evolve with the option on has succeeded
  for (auto& A : ctx->fam) A.nt = 0;
  ctx->final_valid = false;
  int rc = evolve_impl(ctx, t, n_t, tol, obs_out, stats);
  int* const d_err = ctx->d_err_cur;
  ctx->d_err_cur = nullptr;
  if (rc != kRcHandoffTimeout) {
    ctx->final_valid = rc == DSE_OK;
    return rc;
  }
  // A workgroup pair of a 2-tile problem was not resident together within the spin limit (the
  // device shared with long-running work of another stream or process).  The first flush after
  // the timeout saw it (launches queued behind it return at once: k_interval checks the error
  // word on entry), so the call runs again on the per-term streaming kernels, which have no
  // inter-workgroup dependency.
  (void)sync_all(ctx);
  const int zero = 0;
  HIPC(hipMemcpy(d_err, &zero, sizeof(int), hipMemcpyHostToDevice));
  const int saved = ctx->persistent;
  ctx->persistent = 0;
  ctx->rerun = true;
  rc = evolve_impl(ctx, t, n_t, tol, obs_out, stats);
  ctx->rerun = false;
  ctx->persistent = saved;
  ctx->d_err_cur = nullptr;
  ctx->handoff_fallbacks = 1;
  if (stats) stats->handoff_fallbacks = 1;
  ctx->final_valid = rc == DSE_OK;
  return rc;
}

int dse_get_state(dse_ctx* ctx, int problem, double* psi_out) {
  if (!ctx) return DSE_ERR_ARG;
  if (problem < 0 || problem >= (int)ctx->probs.size()) return fail(ctx, DSE_ERR_ARG, "bad problem id");
  if (!psi_out) return fail(ctx, DSE_ERR_ARG, "null state");
  if (!ctx->evolved) return fail(ctx, DSE_ERR_STATE, "no evolved state (call dse_evolve first)");
  HIPC(hipSetDevice(ctx->device));
  int first = 0, count = 1;
  int rc = hook_members(ctx, problem, &first, &count);
  if (rc) return rc;
  double2* out = reinterpret_cast<double2*>(psi_out);
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    const size_t amps = size_t(1) << P.n_local;
    HIPC(hipMemcpy(out + i * amps, P.buf[P.final_bsel], amps * sizeof(double2), hipMemcpyDeviceToHost));
  }
  return DSE_OK;
}

}  // extern "C"

namespace {

// The members a custom-initial-state call on `problem` acts on (hook_members: the whole loopback
// register for its shard 0); registers partitioned over processes are not supported.
int init_members(dse_ctx* ctx, int problem, int* first, int* count, const char* who) {
  const int rc = hook_members(ctx, problem, first, count);
  if (rc) return rc;
  if (ctx->probs[*first].dist)
    return fail(ctx, DSE_ERR_ARG, std::string(who) + ": not available for a register partitioned over processes");
  return DSE_OK;
}

// Every member gets its stored-state buffer (kept if it has one).  On failure the buffers this call
// allocated are released and the members keep their previous initial state.
int ensure_init_state(dse_ctx* ctx, int first, int count) {
  std::vector<int> fresh;
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    if (P.init_state) continue;
    if (hipMalloc(&P.init_state, (size_t(1) << P.n_local) * sizeof(double2)) != hipSuccess) {
      (void)hipGetLastError();
      P.init_state = nullptr;
      for (int j : fresh) (void)hipFree(ctx->probs[j].init_state), ctx->probs[j].init_state = nullptr;
      return fail(ctx, DSE_ERR_OOM, "initial-state buffer allocation failed");
    }
    fresh.push_back(first + i);
  }
  return DSE_OK;
}

void set_init_stored(dse_ctx* ctx, int first, int count) {
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    if (P.d_init_amp) (void)hipFree(P.d_init_amp), P.d_init_amp = nullptr;
    P.init_amp.clear();
    P.init_kind = 1;
  }
}

}  // namespace

extern "C" {

int dse_set_initial_state(dse_ctx* ctx, int problem, const double* psi) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_set_initial_state");
  if (rc) return rc;
  HIPC(hipSetDevice(ctx->device));
  if (!psi) {  // back to the basis state psi0_index
    for (int i = 0; i < count; ++i) free_initial(ctx->probs[first + i]);
    return DSE_OK;
  }
  const size_t total = size_t(1) << ctx->probs[first].n;
  bool nonzero = false;
  for (size_t i = 0; i < 2 * total; ++i) {
    if (!std::isfinite(psi[i])) return fail(ctx, DSE_ERR_ARG, "dse_set_initial_state: non-finite amplitude");
    nonzero = nonzero || psi[i] != 0.0;
  }
  if (!nonzero) return fail(ctx, DSE_ERR_ARG, "dse_set_initial_state: the state is zero");
  if ((rc = ensure_init_state(ctx, first, count))) return rc;
  const double2* in = reinterpret_cast<const double2*>(psi);
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    const size_t amps = size_t(1) << P.n_local;
    HIPC(hipMemcpy(P.init_state, in + i * amps, amps * sizeof(double2), hipMemcpyHostToDevice));
  }
  set_init_stored(ctx, first, count);
  return DSE_OK;
}

int dse_set_overlap_refs(dse_ctx* ctx, int problem, int k, const double* refs) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_set_overlap_refs");
  if (rc) return rc;
  if (k < 0 || k > DSE_MAX_OVERLAP_REFS)
    return fail(ctx, DSE_ERR_ARG, "dse_set_overlap_refs: k must be in 0.." + std::to_string(DSE_MAX_OVERLAP_REFS));
  HIPC(hipSetDevice(ctx->device));
  if (k == 0 || !refs) {
    (void)sync_all(ctx);
    for (int i = 0; i < count; ++i) free_overlap_refs(ctx->probs[first + i]);
    return DSE_OK;
  }
  const size_t total = size_t(1) << ctx->probs[first].n;
  for (int r = 0; r < k; ++r) {
    bool nonzero = false;
    for (size_t i = 0; i < 2 * total; ++i) {
      const double a = refs[2 * total * r + i];
      if (!std::isfinite(a)) return fail(ctx, DSE_ERR_ARG, "dse_set_overlap_refs: non-finite amplitude");
      nonzero = nonzero || a != 0.0;
    }
    if (!nonzero) return fail(ctx, DSE_ERR_ARG, "dse_set_overlap_refs: reference " + std::to_string(r) + " is zero");
  }
  // the new set beside the old one: a failed allocation leaves the previous set in place
  std::vector<std::vector<double2*>> fresh(count);
  std::vector<const double2**> tabs(count, nullptr);
  bool ok = true;
  for (int i = 0; i < count && ok; ++i) {
    const size_t amps = size_t(1) << ctx->probs[first + i].n_local;
    for (int r = 0; r < k && ok; ++r) {
      double2* b = nullptr;
      ok = hipMalloc(&b, amps * sizeof(double2)) == hipSuccess;
      if (ok) fresh[i].push_back(b);
    }
    ok = ok && hipMalloc(&tabs[i], kMaxOverlapRefs * sizeof(double2*)) == hipSuccess;
  }
  const double2* in = reinterpret_cast<const double2*>(refs);
  hipError_t he = hipSuccess;
  for (int i = 0; i < count && ok && he == hipSuccess; ++i) {
    const size_t amps = size_t(1) << ctx->probs[first + i].n_local;
    for (int r = 0; r < k && he == hipSuccess; ++r)
      he = hipMemcpy(fresh[i][r], in + total * r + i * amps, amps * sizeof(double2), hipMemcpyHostToDevice);
    std::vector<const double2*> tab(kMaxOverlapRefs, nullptr);
    std::copy(fresh[i].begin(), fresh[i].end(), tab.begin());
    if (he == hipSuccess) he = hipMemcpy(tabs[i], tab.data(), tab.size() * sizeof(double2*), hipMemcpyHostToDevice);
  }
  if (!ok || he != hipSuccess) {
    (void)hipGetLastError();
    for (int i = 0; i < count; ++i) {
      for (double2* b : fresh[i]) (void)hipFree(b);
      if (tabs[i]) (void)hipFree(tabs[i]);
    }
    if (!ok) return fail(ctx, DSE_ERR_OOM, "overlap reference buffer allocation failed");
    return fail(ctx, DSE_ERR_HIP, std::string("dse_set_overlap_refs: ") + hipGetErrorString(he));
  }
  (void)sync_all(ctx);
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    free_overlap_refs(P);
    P.ovl_refs = fresh[i];
    P.d_ovl_tab = tabs[i];
  }
  return DSE_OK;
}

int dse_overlap_refs(const dse_ctx* ctx, int problem) {
  if (!ctx || problem < 0 || problem >= (int)ctx->probs.size()) return DSE_ERR_ARG;
  return ctx->probs[problem].ovl_k();
}

// One string, codes by register bit, into its masks and prefactor (include/dse.h: dse_site_op).  With
// bit value 0 = up: Ix = (|0><1| + |1><0|) / 2, Iy = (|0><1| - |1><0|) / 2i, Iz = diag(1, -1) / 2,
// I+ = |0><1|, I- = |1><0|.  <x|O|x ^ flip> of one bit: Ix 1/2; Iy -i/2 for x = 0 and +i/2 for
// x = 1, i.e. (-i/2) (-1)^x; Iz (1/2) (-1)^x; I+ only x = 0, I- only x = 1; Ea only x = 0, Eb only x = 1.
bool compile_op_string(int n, const uint8_t* ops, StringEntry* e) {
  StringEntry s{0, 0, 0, 0, 1.0, 0.0};
  int halves = 0, ny = 0;
  for (int b = 0; b < n; ++b) {
    const uint64_t m = uint64_t(1) << b;
    switch (ops[b]) {
      case DSE_OP_1: break;
      case DSE_OP_X: s.xm |= m, ++halves; break;
      case DSE_OP_Y: s.xm |= m, s.zm |= m, ++halves, ++ny; break;
      case DSE_OP_Z: s.zm |= m, ++halves; break;
      case DSE_OP_P: s.xm |= m, s.cm |= m; break;
      case DSE_OP_M: s.xm |= m, s.cm |= m, s.cv |= m; break;
      case DSE_OP_EA: s.cm |= m; break;
      case DSE_OP_EB: s.cm |= m, s.cv |= m; break;
      default: return false;
    }
  }
  const double mag = std::ldexp(1.0, -halves);
  static const double kRe[4] = {1, 0, -1, 0}, kIm[4] = {0, -1, 0, 1};  // (-i)^k
  s.pre_re = mag * kRe[ny & 3];
  s.pre_im = mag * kIm[ny & 3];
  *e = s;
  return true;
}

int dse_op_string_masks(int n, const uint8_t* ops, uint64_t* masks, double* pre) {
  if (n < 1 || n > DSE_MAX_QUBITS || !ops || !masks || !pre) return DSE_ERR_ARG;
  StringEntry e;
  if (!compile_op_string(n, ops, &e)) return DSE_ERR_ARG;
  masks[0] = e.xm, masks[1] = e.zm, masks[2] = e.cm, masks[3] = e.cv;
  pre[0] = e.pre_re, pre[1] = e.pre_im;
  return DSE_OK;
}

int dse_set_op_strings(dse_ctx* ctx, int problem, int k, const uint8_t* ops) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_set_op_strings");
  if (rc) return rc;
  if (k < 0 || k > DSE_MAX_OP_STRINGS)
    return fail(ctx, DSE_ERR_ARG, "dse_set_op_strings: k must be in 0.." + std::to_string(DSE_MAX_OP_STRINGS));
  HIPC(hipSetDevice(ctx->device));
  if (k == 0 || !ops) {
    (void)sync_all(ctx);
    for (int i = 0; i < count; ++i) free_op_strings(ctx->probs[first + i]);
    return DSE_OK;
  }
  const int n = ctx->probs[first].n;
  std::vector<StringEntry> tab(k);
  for (int s = 0; s < k; ++s)
    if (!compile_op_string(n, ops + (size_t)s * n, &tab[s]))
      return fail(ctx, DSE_ERR_ARG, "dse_set_op_strings: string " + std::to_string(s) + " holds a code above 7");
  // the new tables beside the old ones: a failed allocation leaves the previous set in place
  std::vector<StringEntry*> fresh(count, nullptr);
  hipError_t he = hipSuccess;
  for (int i = 0; i < count && he == hipSuccess; ++i) {
    he = hipMalloc(&fresh[i], tab.size() * sizeof(StringEntry));
    if (he != hipSuccess) fresh[i] = nullptr;
    if (he == hipSuccess) he = hipMemcpy(fresh[i], tab.data(), tab.size() * sizeof(StringEntry), hipMemcpyHostToDevice);
  }
  if (he != hipSuccess) {
    (void)hipGetLastError();
    for (StringEntry* b : fresh)
      if (b) (void)hipFree(b);
    return fail(ctx, he == hipErrorOutOfMemory ? DSE_ERR_OOM : DSE_ERR_HIP, std::string("dse_set_op_strings: ") + hipGetErrorString(he));
  }
  (void)sync_all(ctx);
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    free_op_strings(P);
    P.str_tab = tab;
    P.d_str_tab = fresh[i];
  }
  return DSE_OK;
}

int dse_op_strings(const dse_ctx* ctx, int problem) {
  if (!ctx || problem < 0 || problem >= (int)ctx->probs.size()) return DSE_ERR_ARG;
  return ctx->probs[problem].str_k();
}

// k sets of an n-bit register, masks[s] = {m, cm, cv}, into the table: validation and layout in one
// place (dse_sector_layout, dse_set_sectors).  The units U, or -1 for what the header refuses.
int compile_sectors(int n, int k, const uint64_t* masks, std::vector<SectorEntry>* tab) {
  if (n < 1 || n > DSE_MAX_QUBITS || k < 1 || k > DSE_MAX_SECTOR_SETS || !masks) return -1;
  const uint64_t all = n >= 64 ? ~uint64_t(0) : (uint64_t(1) << n) - 1;
  int off = 0;
  if (tab) tab->clear();
  for (int s = 0; s < k; ++s) {
    const uint64_t m = masks[3 * s], cm = masks[3 * s + 1], cv = masks[3 * s + 2];
    if (((m | cm | cv) & ~all) || (m & cm) || (cv & ~cm)) return -1;
    const int bins = __builtin_popcountll(m) + 1;
    if (tab) tab->push_back(SectorEntry{m, cm, cv, off, bins});
    off += bins;
  }
  return off;
}

int dse_sector_layout(int n, int k, const uint64_t* masks, int* offsets) {
  std::vector<SectorEntry> tab;
  const int U = compile_sectors(n, k, masks, &tab);
  if (U < 0) return DSE_ERR_ARG;
  if (offsets) {
    for (int s = 0; s < k; ++s) offsets[s] = tab[s].off;
    offsets[k] = U;
  }
  return U;
}

int dse_set_sectors(dse_ctx* ctx, int problem, int k, const uint64_t* masks) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_set_sectors");
  if (rc) return rc;
  if (k < 0 || k > DSE_MAX_SECTOR_SETS)
    return fail(ctx, DSE_ERR_ARG, "dse_set_sectors: k must be in 0.." + std::to_string(DSE_MAX_SECTOR_SETS));
  HIPC(hipSetDevice(ctx->device));
  if (k == 0) {
    (void)sync_all(ctx);
    for (int i = 0; i < count; ++i) free_sectors(ctx->probs[first + i]);
    return DSE_OK;
  }
  std::vector<SectorEntry> tab;
  if (compile_sectors(ctx->probs[first].n, k, masks, &tab) < 0)
    return fail(ctx, DSE_ERR_ARG, "dse_set_sectors: null masks, a bit at or above n, m & cm != 0 or cv & ~cm != 0");
  // the new tables beside the old ones: a failed allocation leaves the previous sets in place
  std::vector<SectorEntry*> fresh(count, nullptr);
  hipError_t he = hipSuccess;
  for (int i = 0; i < count && he == hipSuccess; ++i) {
    he = hipMalloc(&fresh[i], tab.size() * sizeof(SectorEntry));
    if (he != hipSuccess) fresh[i] = nullptr;
    if (he == hipSuccess) he = hipMemcpy(fresh[i], tab.data(), tab.size() * sizeof(SectorEntry), hipMemcpyHostToDevice);
  }
  if (he != hipSuccess) {
    (void)hipGetLastError();
    for (SectorEntry* b : fresh)
      if (b) (void)hipFree(b);
    return fail(ctx, he == hipErrorOutOfMemory ? DSE_ERR_OOM : DSE_ERR_HIP, std::string("dse_set_sectors: ") + hipGetErrorString(he));
  }
  (void)sync_all(ctx);
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    free_sectors(P);
    P.sec_tab = tab;
    P.d_sec_tab = fresh[i];
  }
  return DSE_OK;
}

int dse_sectors(const dse_ctx* ctx, int problem) {
  if (!ctx || problem < 0 || problem >= (int)ctx->probs.size()) return DSE_ERR_ARG;
  return ctx->probs[problem].sec_k();
}

int dse_sector_units(const dse_ctx* ctx, int problem) {
  if (!ctx || problem < 0 || problem >= (int)ctx->probs.size()) return DSE_ERR_ARG;
  return ctx->probs[problem].sec_units();
}

int dse_set_initial_product(dse_ctx* ctx, int problem, const double* amp) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_set_initial_product");
  if (rc) return rc;
  if (!amp) return fail(ctx, DSE_ERR_ARG, "dse_set_initial_product: null amplitudes");
  const int n = ctx->probs[first].n;
  for (int b = 0; b < n; ++b) {
    const double* a = amp + 4 * b;
    if (!(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]) && std::isfinite(a[3])))
      return fail(ctx, DSE_ERR_ARG, "dse_set_initial_product: non-finite amplitude");
    if (a[0] == 0.0 && a[1] == 0.0 && a[2] == 0.0 && a[3] == 0.0)
      return fail(ctx, DSE_ERR_ARG, "dse_set_initial_product: amplitude pair of bit " + std::to_string(b) + " is zero");
  }
  HIPC(hipSetDevice(ctx->device));
  std::vector<int> fresh;
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    if (P.d_init_amp) continue;
    if (hipMalloc(&P.d_init_amp, 4 * (size_t)n * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      P.d_init_amp = nullptr;
      for (int j : fresh) (void)hipFree(ctx->probs[j].d_init_amp), ctx->probs[j].d_init_amp = nullptr;
      return fail(ctx, DSE_ERR_OOM, "product-state table allocation failed");
    }
    fresh.push_back(first + i);
  }
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    HIPC(hipMemcpy(P.d_init_amp, amp, 4 * (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    if (P.init_state) (void)hipFree(P.init_state), P.init_state = nullptr;  // no state-sized buffer is kept
    P.init_amp.assign(amp, amp + 4 * (size_t)n);
    P.init_kind = 2;
  }
  return DSE_OK;
}

int dse_continue_from_final(dse_ctx* ctx, int problem) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_continue_from_final");
  if (rc) return rc;
  if (!ctx->evolved || !ctx->final_valid)
    return fail(ctx, DSE_ERR_STATE, "no final state (needs a successful dse_evolve before)");
  HIPC(hipSetDevice(ctx->device));
  if ((rc = ensure_init_state(ctx, first, count))) return rc;
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    HIPC(hipMemcpy(P.init_state, P.buf[P.final_bsel], (size_t(1) << P.n_local) * sizeof(double2),
                   hipMemcpyDeviceToDevice));
  }
  HIPC(hipDeviceSynchronize());
  set_init_stored(ctx, first, count);
  return DSE_OK;
}

int dse_get_initial_state(dse_ctx* ctx, int problem, double* psi_out) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_get_initial_state");
  if (rc) return rc;
  if (!psi_out) return fail(ctx, DSE_ERR_ARG, "null state");
  HIPC(hipSetDevice(ctx->device));
  double2* out = reinterpret_cast<double2*>(psi_out);
  for (int i = 0; i < count; ++i) {
    HostProblem& P = ctx->probs[first + i];
    const size_t amps = size_t(1) << P.n_local;
    double2* dst = out + i * amps;
    if (P.init_kind == 1) {
      HIPC(hipMemcpy(dst, P.init_state, amps * sizeof(double2), hipMemcpyDeviceToHost));
    } else if (P.init_kind == 2) {  // the kernel dse_evolve runs, into a buffer of the call's own
      double2* tmp = nullptr;
      if (hipMalloc(&tmp, amps * sizeof(double2)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, DSE_ERR_OOM, "dse_get_initial_state: allocation failed");
      }
      hipError_t e = launch_product_state(tmp, P.d_init_amp, P.n, P.n_local, (uint64_t)P.shard_rank, nullptr);
      if (e == hipSuccess) e = hipMemcpy(dst, tmp, amps * sizeof(double2), hipMemcpyDeviceToHost);
      (void)hipFree(tmp);
      HIPC(e);
    } else {
      std::memset(dst, 0, amps * sizeof(double2));
      if ((P.psi0 >> P.n_local) == (uint64_t)P.shard_rank)
        dst[P.psi0 & ((uint64_t(1) << P.n_local) - 1)] = make_double2(1.0, 0.0);
    }
  }
  return DSE_OK;
}

// ---- hard pulses and a new H for a problem (features "pulse", "set_hamiltonian") ------------------

int dse_apply_pulse(dse_ctx* ctx, int problem, const double* u) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_apply_pulse");
  if (rc) return rc;
  if (!u) return fail(ctx, DSE_ERR_ARG, "dse_apply_pulse: null matrices");
  const HostProblem& P0 = ctx->probs[first];
  const int n = P0.n;
  uint64_t active = 0, diag = 0;
  for (int b = 0; b < n; ++b) {
    const double* m = u + 8 * b;
    bool zero = true;
    for (int i = 0; i < 8; ++i) {
      if (!std::isfinite(m[i])) return fail(ctx, DSE_ERR_ARG, "dse_apply_pulse: non-finite matrix entry");
      zero = zero && m[i] == 0.0;
    }
    if (zero) return fail(ctx, DSE_ERR_ARG, "dse_apply_pulse: the matrix of bit " + std::to_string(b) + " is zero");
    const bool dg = m[2] == 0.0 && m[3] == 0.0 && m[4] == 0.0 && m[5] == 0.0;
    const bool id = dg && m[0] == 1.0 && m[1] == 0.0 && m[6] == 1.0 && m[7] == 0.0;
    if (!id) active |= uint64_t(1) << b;
    if (dg && !id) diag |= uint64_t(1) << b;
  }
  ctx->pulse_stats[0] = ctx->pulse_stats[1] = ctx->pulse_stats[2] = 0.0;
  if (!active) return DSE_OK;  // the identity: nothing changes, whatever the kind of start
  if (P0.init_kind != 1) {
    // a product state stays one: a_b <- U_b a_b; the basis state becomes the product of the columns
    // bit_b(psi0) of the U_b
    std::vector<double> amp(4 * (size_t)n);
    for (int b = 0; b < n; ++b) {
      const double* m = u + 8 * b;
      double a[4] = {1.0, 0.0, 0.0, 0.0};
      if (P0.init_kind == 2) std::copy(P0.init_amp.begin() + 4 * b, P0.init_amp.begin() + 4 * b + 4, a);
      else if ((P0.psi0 >> b) & 1) a[0] = 0.0, a[2] = 1.0;
      double* o = &amp[4 * (size_t)b];
      for (int v = 0; v < 2; ++v) {
        const double* r = m + 4 * v;  // row v: (re u_v0, im u_v0, re u_v1, im u_v1)
        o[2 * v] = (r[0] * a[0] - r[1] * a[1]) + (r[2] * a[2] - r[3] * a[3]);
        o[2 * v + 1] = (r[0] * a[1] + r[1] * a[0]) + (r[2] * a[3] + r[3] * a[2]);
      }
      if (!(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]) && std::isfinite(o[3])))
        return fail(ctx, DSE_ERR_ARG, "dse_apply_pulse: non-finite amplitude of bit " + std::to_string(b));
      if (o[0] == 0.0 && o[1] == 0.0 && o[2] == 0.0 && o[3] == 0.0)
        return fail(ctx, DSE_ERR_ARG, "dse_apply_pulse: the pulse maps the amplitude pair of bit " + std::to_string(b) + " to zero");
    }
    return dse_set_initial_product(ctx, problem, amp.data());
  }
  HIPC(hipSetDevice(ctx->device));
  if ((rc = ctx->d_pulse_tab.reserve(ctx, 1, "pulse table allocation failed"))) return rc;
  for (auto& e : ctx->pulse_ev)
    if (!e) HIPC(hipEventCreate(&e));
  double2* base[kMaxShards] = {};
  for (int i = 0; i < count; ++i) base[i] = ctx->probs[first + i].init_state;
  hipStream_t st = ctx->lanes[0].stream;
  int passes = 0;
  HIPC(hipEventRecord(ctx->pulse_ev[0], st));
  HIPC(launch_pulse(base, P0.n_local, count > 1 ? P0.shard_bits : 0, u, active, diag, ctx->d_pulse_tab.p, st, &passes));
  HIPC(hipEventRecord(ctx->pulse_ev[1], st));
  HIPC(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPC(hipEventElapsedTime(&ms, ctx->pulse_ev[0], ctx->pulse_ev[1]));
  ctx->pulse_stats[0] = passes;
  ctx->pulse_stats[1] = ms;
  ctx->pulse_stats[2] = 32.0 * (double)passes * std::ldexp(1.0, n);
  return DSE_OK;
}

int dse_pulse_stats(const dse_ctx* ctx, double* out) {
  if (!ctx || !out) return DSE_ERR_ARG;
  std::copy(ctx->pulse_stats, ctx->pulse_stats + 3, out);
  return DSE_OK;
}

int dse_set_hamiltonian(dse_ctx* ctx, int problem, const double* field, const double* zz, const double* pair,
                        const double* flip, double shift) {
  if (!ctx) return DSE_ERR_ARG;
  int first = 0, count = 1;
  int rc = init_members(ctx, problem, &first, &count, "dse_set_hamiltonian");
  if (rc) return rc;
  const HostProblem& P0 = ctx->probs[first];
  HostProblem q;  // validated as dse_add_problem validates; the old H stays on failure
  if ((rc = make_problem(ctx, q, P0.n, field, zz, pair, flip, shift, P0.psi0, P0.sea_mask, P0.rare_bit, P0.rare_z)))
    return rc;
  (void)hipSetDevice(ctx->device);
  (void)sync_all(ctx);
  free_device(ctx);  // the device layout is rebuilt lazily; the previous final state goes with it
  for (int i = 0; i < count; ++i) {
    // a problem as dse_add_problem(_sharded) makes it (free_device left no device pointer behind) that
    // takes over the shard layout and what belongs to the problem beyond its tables
    HostProblem& P = ctx->probs[first + i];
    HostProblem f = q;
    f.shard_bits = P.shard_bits, f.shard_rank = P.shard_rank, f.n_local = P.n_local;
    f.group_first = P.group_first, f.dist = P.dist;
    f.init_kind = P.init_kind, f.init_state = P.init_state, f.d_init_amp = P.d_init_amp;
    f.init_amp = std::move(P.init_amp);
    f.ovl_refs = std::move(P.ovl_refs), f.d_ovl_tab = P.d_ovl_tab;
    f.str_tab = std::move(P.str_tab), f.d_str_tab = P.d_str_tab;
    f.sec_tab = std::move(P.sec_tab), f.d_sec_tab = P.d_sec_tab;
    P = std::move(f);
  }
  return DSE_OK;
}

int dse_energy(dse_ctx* ctx, int problem, double* e_out) {
  if (!ctx) return DSE_ERR_ARG;
  if (!e_out) return fail(ctx, DSE_ERR_ARG, "null pointer");
  if (!ctx->evolved) return fail(ctx, DSE_ERR_STATE, "no evolved state (call dse_evolve first)");
  int first = 0, count = 1;
  int rc = hook_members(ctx, problem, &first, &count);
  if (rc) return rc;
  if (ctx->probs[first].dist) return fail(ctx, DSE_ERR_ARG, "dse_energy: not available for a dist shard");
  HIPC(hipSetDevice(ctx->device));
  hipStream_t st = ctx->lanes[0].stream;
  for (int i = 0; i < count; ++i) {  // H reads buf[0]: copy the state there (it stays in its buffer)
    HostProblem& P = ctx->probs[first + i];
    if (P.final_bsel != 0)
      HIPC(hipMemcpyAsync(P.buf[0], P.buf[P.final_bsel], (size_t(1) << P.n_local) * sizeof(double2),
                          hipMemcpyDeviceToDevice, st));
  }
  if ((rc = apply_members(ctx, first, count, st))) return rc;
  constexpr int kBlocks = 1024;
  double* d = nullptr;
  HIPC(hipMalloc(&d, (size_t)count * kBlocks * 2 * sizeof(double)));
  hipError_t e = hipSuccess;
  for (int i = 0; i < count && e == hipSuccess; ++i) {
    const HostProblem& P = ctx->probs[first + i];
    e = launch_dot(P.buf[0], P.buf[1], size_t(1) << P.n_local, d + (size_t)i * kBlocks * 2, kBlocks, st);
  }
  std::vector<double> h((size_t)count * kBlocks * 2);
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d);
  HIPC(e);
  double en = 0.0, n2 = 0.0;
  for (size_t b = 0; b < h.size(); b += 2) {
    en += h[b];
    n2 += h[b + 1];
  }
  e_out[0] = n2 > 0.0 ? en / n2 : 0.0;
  e_out[1] = n2;
  return DSE_OK;
}

int dse_time_step_kernel(dse_ctx* ctx, int reps, double* ms_per_launch, double* bytes_per_launch) {
  if (!ctx) return DSE_ERR_ARG;
  if (reps < 1 || !ms_per_launch || !bytes_per_launch) return fail(ctx, DSE_ERR_ARG, "bad arguments");
  if (!ctx->evolved) return fail(ctx, DSE_ERR_STATE, "call dse_evolve first (coefficients needed)");
  HIPC(hipSetDevice(ctx->device));
  Lane& ln = ctx->lanes[0];
  int rc = ensure_events(ctx, ln, (size_t)reps);
  if (rc) return rc;
  // one launch over every item of every lane: the whole batch at term k = 2
  std::vector<int2> items(ctx->total_items);
  HIPC(hipMemcpy(items.data(), ctx->d_items, items.size() * sizeof(int2), hipMemcpyDeviceToHost));
  std::map<int, std::vector<int2>> by_L;
  if (ctx->probe_items > 0 && (int64_t)items.size() > ctx->probe_items) items.resize(ctx->probe_items);
  for (auto& it : items) by_L[ctx->probs[it.x].L].push_back(it);
  int2* d_tmp = nullptr;
  HIPC(hipMalloc(&d_tmp, items.size() * sizeof(int2)));
  double bytes = 0.0, tot = 0.0;
  int64_t off = 0;
  std::vector<std::pair<int, int64_t>> segs;
  for (auto& kv : by_L) {
    HIPC(hipMemcpy(d_tmp + off, kv.second.data(), kv.second.size() * sizeof(int2), hipMemcpyHostToDevice));
    segs.push_back({kv.first, off});
    off += (int64_t)kv.second.size();
    bytes += 48.0 * (double)kv.second.size() * (double)(1 << kv.first);
  }
  for (int r = 0; r < reps; ++r) {
    HIPC(hipEventRecord(ln.ev[0][2 * r], ln.stream));
    for (size_t s = 0; s < segs.size(); ++s) {
      const int64_t cnt = (s + 1 < segs.size() ? segs[s + 1].second : off) - segs[s].second;
      HIPC(launch_step(segs[s].first, MODE_GEN, ctx->d_probs, d_tmp + segs[s].second, (int)cnt, 2, 0, 0, ln.stream));
    }
    HIPC(hipEventRecord(ln.ev[0][2 * r + 1], ln.stream));
  }
  HIPC(hipStreamSynchronize(ln.stream));
  for (int r = 0; r < reps; ++r) {
    float ms = 0.f;
    HIPC(hipEventElapsedTime(&ms, ln.ev[0][2 * r], ln.ev[0][2 * r + 1]));
    tot += ms;
  }
  (void)hipFree(d_tmp);
  *ms_per_launch = tot / reps;
  *bytes_per_launch = bytes;
  ctx->evolved = false;  // buffers now hold timing garbage
  return DSE_OK;
}

}  // extern "C"
