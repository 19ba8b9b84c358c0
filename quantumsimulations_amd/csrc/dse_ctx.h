// dse_ctx.h -- what the sources of the host runtime share (dse_runtime.hip, dse_rt_*.hip): the context and
// problem types, the error helpers, and the functions that cross from one source to another.  Private to the
// runtime: no kernel source includes it, and no function it declares is a dynamic symbol of the library.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <string>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <deque>
#include <vector>

#include <rccl/rccl.h>
#include <rocblas/rocblas.h>

#include "../../include/dse.h"
#include "dse_internal.h"
#include "dse_dense.h"
#include "dse_small.h"
#include "dse_wht.h"

#pragma GCC visibility push(hidden)

namespace dse::rt {

struct HostProblem {
  int n = 0;
  std::vector<double> field, zz, pair, flip;
  double shift = 0.0;
  uint64_t psi0 = 0, sea_mask = 0;
  int rare_bit = -1;
  double rare_z = 0.0;
  double e_min = 0.0, e_max = 0.0;
  // device state
  int L = 0;
  int64_t n_tiles = 0;
  double2* buf[3] = {nullptr, nullptr, nullptr};
  void* tables = nullptr;
  double2* coef = nullptr;   // into dse_ctx::d_coef (compact rows, coef_row)
  int degree = 1;
  double flops_per_amp = 0.0;  // algorithmic flops of one H application per amplitude
  int2* d_items = nullptr;  // this problem's tiles (apply_h / observables hooks)
  // partitioned register (dse_add_problem_sharded): shard `shard_rank` of 2^shard_bits
  int shard_bits = 0, shard_rank = 0;
  int n_local = 0;           // qubits held by this shard (n - shard_bits)
  int group_first = -1;      // loopback group: index of shard 0 (all shards in this context)
  bool dist = false;         // shard of a register partitioned over processes (RCCL exchange)
  uint32_t xmasks = 0;       // bit m set: terms or observables read shard rank ^ m
  double2* rbuf_own[kMaxShards] = {};  // dist: receive buffers of the exchange, per mask
  bool imag = false;         // every drive coefficient purely imaginary (drive phase pi/2)
  // Walsh-Hadamard engine (dse_wht.hip): X- and Y-branch vectors and the pair matrix
  double2* wvec[4] = {nullptr, nullptr, nullptr, nullptr};  // A, B (+ index-swapped A, B)
  double* d_cquad = nullptr;
  double* d_wtab = nullptr;  // ztab | xytab
  int wht_groups = 0;        // passes' tile-bit groups; 0: this problem uses the step kernels
  // small-register engine (dse_small.hip): n <= 9 qubits, whole evolution one wave per problem
  bool sm = false;           // this evolve runs the problem on that engine
  // dense eigen-propagator engine (dse_dense.hip): this evolve diagonalises the register instead
  bool dn = false;
  // propagator-matrix mode (matrix_run): the context's single register, U = exp(-iH dt) built
  // column by column, the outputs by repeated products
  bool mx = false;
  bool side() const { return sm || dn || mx; }  // not on the per-interval Chebyshev launches
  double2* sm_coef = nullptr;  // into dse_ctx::d_sm_coef
  int* sm_deg = nullptr;
  int final_bsel = 0;        // buffer holding the final state after dse_evolve
  // spanning register (dse_span.hip): this evolve runs the register over 2^span_s workgroups of
  // 2^(n - span_s) amplitudes (0: not spanned)
  int span_s = 0;
  // real-component mode (dse_real.hip): this evolve runs the register as two real recurrences
  bool rl = false;
  // the leap path (choose_leap; with rl): one real recurrence per launch, outputs by the time recurrence
  bool lp = false;
  int leap_k[kLeapMaxOut / kMaxOut] = {};  // the degree of each workgroup's pair of rows (build_coefficients)
  // custom psi(t0) (ABI 14.1; every shard of a loopback register alike): 0 the basis state psi0; 1 a
  // stored state in init_state (this shard's 2^n_local amplitudes: the one extra state-sized
  // buffer, held only while the problem has a stored state); 2 a product state, its 4 n amplitudes
  // in init_amp and on the device in d_init_amp.  They belong to the problem: kept over evolves and
  // over free_device, released by dse_clear / dse_destroy or when the kind changes
  int init_kind = 0;
  double2* init_state = nullptr;
  std::vector<double> init_amp;
  double* d_init_amp = nullptr;
  // reference states of the overlaps (dse_set_overlap_refs; every shard of a loopback register
  // alike): K device buffers of this shard's 2^n_local amplitudes and the device table of their
  // pointers the kernels read (kMaxOverlapRefs entries).  They belong to the problem like the
  // initial state: kept over evolves and over free_device, replaced as a set, released by dse_clear
  // / dse_destroy
  std::vector<double2*> ovl_refs;
  const double2** d_ovl_tab = nullptr;
  int ovl_k() const { return (int)ovl_refs.size(); }
  // operator strings (dse_set_op_strings; every shard of a loopback register alike): the compiled
  // table, masks by register bit, and its device copy the kernels read.  They belong to the problem
  // like the references: kept over evolves, over free_device and over dse_set_hamiltonian, replaced
  // as a set, released by dse_clear / dse_destroy
  std::vector<StringEntry> str_tab;
  StringEntry* d_str_tab = nullptr;
  int str_k() const { return (int)str_tab.size(); }
  // sector sets (dse_set_sectors; every shard of a loopback register alike): the table, masks by
  // register bit with each set's first unit, and its device copy.  They belong to the problem as the
  // strings do
  std::vector<SectorEntry> sec_tab;
  SectorEntry* d_sec_tab = nullptr;
  int sec_k() const { return (int)sec_tab.size(); }
  int sec_units() const { return sec_tab.empty() ? 0 : sec_tab.back().off + sec_tab.back().bins; }
};

inline int fail(dse_ctx* c, int code, const std::string& msg);

// One grow-only device buffer of cap elements.  reserve() keeps a buffer that is large enough and
// otherwise frees it before it allocates the larger one (the contents are not kept); after a failed
// allocation the buffer is empty, cap = 0.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // in elements
  void release() {
    if (p) (void)hipFree(p), p = nullptr;
    cap = 0;
  }
  // what: the message of DSE_ERR_OOM; with_bytes appends " (<size> bytes)"
  int reserve(dse_ctx* ctx, size_t n, const char* what, bool with_bytes = false) {
    if (n <= cap) return DSE_OK;
    release();
    if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) {
      p = nullptr;
      return fail(ctx, DSE_ERR_OOM, with_bytes ? std::string(what) + " (" + std::to_string(n * sizeof(T)) + " bytes)" : what);
    }
    cap = n;
    return DSE_OK;
  }
};
template <class... B>
void release_all(B&... b) { (b.release(), ...); }

// The observable families beside the seven aggregates: sums per unit (register bit, pair of bits,
// reference state, operator string, sector bin) of every output state, kept per register and read back after the evolve.
// kObsFamilies below describes each; the engines launch them in this order and read them back in the
// reverse one.
enum ObsFamily { kSite = 0, kPair = 1, kOverlap = 2, kString = 3, kSector = 4, kNumObsFamilies = 5 };
constexpr ObsFamily kObsLaunchOrder[kNumObsFamilies] = {kSite, kPair, kOverlap, kString, kSector};
constexpr ObsFamily kObsReadbackOrder[kNumObsFamilies] = {kSector, kString, kOverlap, kPair, kSite};

// What a context holds for one family: its option, a partial arena for the tile engine's kernel
// (S doubles per tile and slot: the family's stride of the context's widest register), and the
// results of the last evolve, per register [comps][units][n_t] (loopback group: shard 0's entry)
struct ObsFamilyState {
  int on = 0;              // the option's value; a family with per-problem units (kOverlap, kString, kSector):
                           // the context holds references / strings / sets (set_unit_families_on)
  int kmax = 0;            // such a family: the most units (references, strings, bins) any register of the context holds
  DevBuf<double> d_partial;
  size_t slots = 0;
  int S = 0;
  std::vector<std::vector<double>> store;
  int nt = 0;              // output times of store (0: none)
  int problems = 0;        // registers with sums in the last successful evolve
  DevBuf<double> d_small;  // small engine: [problem][n_t][small_stride] raw sums
  void release() {
    release_all(d_partial, d_small);
    slots = 0;
    store.clear();
    nt = problems = 0;
  }
};

// What a lane group launches.  Tiles: k_interval (persistent) or the step / Walsh-Hadamard kernels (streaming)
// over problems of `tiles` tiles each; Mixed: 1- and 2-tile problems in one k_interval launch; Span: k_span; Real: k_real
enum class GroupKind { Tiles, Mixed, Span, Real };

// One stream's share of the problems, grouped by tile size.
struct LaneGroup {
  int L = 0;
  GroupKind kind = GroupKind::Tiles;
  int tiles = 1;            // tiles per problem of kind Tiles (persistent mode: 1 or 2); else 0
  int wht_groups = 0;       // > 0: every problem of the group runs on the Walsh-Hadamard engine
  std::vector<std::pair<int, int>> wht_regs;  // partitioned registers: (first shard, degree)
  int64_t off = 0;          // first position in the global item array
  int64_t count = 0;        // items of this group
  std::vector<int> active;     // active[k] = items with degree >= k (prefix of the group)
  std::vector<double> bytes;   // bytes[k] = algorithmic HBM bytes of the term-k launch
  std::vector<double> flops;   // flops[k] = algorithmic flops of the term-k launch
  // spanning registers (kind Span): k_span<span_L, span_rb> over span_count launch items from
  // span_off in dse_ctx::d_span_items (tiles of one register 8 apart, padding items x = -1)
  int span_L = 0, span_rb = 0;
  int64_t span_off = 0, span_count = 0;
  // launch boundaries inside those items (relative to span_off, last = span_count): whole blocks of
  // 8 registers, each launch at most what the chip holds at once (every register's tiles resident
  // together: its hand-offs wait on each other)
  std::vector<int64_t> span_cuts;
  std::vector<double> span_am, span_fl;  // per launch: amplitudes x terms, algorithmic flops
  // real-component registers: k_real over real_count items (problem, component) from real_off in
  // dse_ctx::d_real_items, then k_real_combine over real_np items (problem, 0) from real_poff
  int64_t real_off = 0, real_count = 0, real_poff = 0, real_np = 0;
};
struct Lane {
  hipStream_t stream = nullptr;
  // persistent mode, option obs_overlap: the observables of interval group g run on obs_stream
  // behind ev_iv[g & 1] (its interval launches), and interval group g + 2, which rewrites the
  // buffers they read, waits for ev_obs[g & 1]
  hipStream_t obs_stream = nullptr;
  hipEvent_t ev_iv[2] = {nullptr, nullptr}, ev_obs[2] = {nullptr, nullptr};
  bool obs_pending[2] = {false, false};
  std::vector<LaneGroup> groups;
  std::vector<hipEvent_t> ev[2];
  size_t ev_used[2] = {0, 0};
  int max_deg = 0;
};

// internal return code of evolve_impl: a persistent hand-off timed out (dse_evolve falls back)
constexpr int kRcHandoffTimeout = 1000;

}  // namespace dse::rt

// The context: the type include/dse.h forward-declares, so it is global; not hidden (its destructor is a
// dynamic symbol of the library).
#pragma GCC visibility pop
struct dse_ctx {
  int device = 0;
  std::string err;
  std::vector<dse::rt::HostProblem> probs;
  dse::DevProb* d_probs = nullptr;
  std::vector<dse::DevProb> h_desc;
  std::vector<dse::rt::Lane> lanes;
  int2* d_items = nullptr;          // all items, lane-major, degree-sorted inside each group
  int2* d_items_iv = nullptr;       // the same, 2-tile groups reordered for the interval kernel
  std::vector<int64_t> item_pos;    // first item position of every problem (evolve layout)
  int64_t total_items = 0;
  dse::rt::DevBuf<double> d_partial;
  size_t partial_slots = 0;
  // site-resolved observables and two-spin correlators (kObsFamilies), indexed by ObsFamily
  dse::rt::ObsFamilyState fam[dse::rt::kNumObsFamilies];
  std::map<std::vector<double>, double*> zzlo_tables;  // identical in-tile ZZ tables are shared
  bool prepared = false;
  bool evolved = false;
  bool final_valid = false;         // the last dse_evolve returned DSE_OK (dse_continue_from_final)
  int last_q = 0;
  int tile_bits = 13;
  int n_streams = 4;
  int persistent = 1;               // use k_interval when every problem fits <= 2 tiles
  int wht = 1;                      // Walsh-Hadamard engine for registers of more tiles
  int wht_group_bits = 0;           // high bits per pass of that engine (0: tile bits - 2)
  int wht_tile_bits = 0;            // its tile: 12, 13 (0 = 13)
  int wht_persist = 0;              // bit 1: MID as a persistent launch (k_wht_mid_p), option wht_persist
  int wht_contiguous = 0;           // option wht_contiguous: hipDeviceMallocContiguous X/Y vectors
  int wht_fuse = 1;                 // option wht_fuse: FINAL of term k runs term k + 1's FIRST
  int wht_mid_inpage = 0;           // option wht_mid_inpage: in-page high bits of the MID group
  int wht_half = 7;                 // option wht_half: half-LDS passes (k_wht_h), bit 0 FIRST, 1 FWD/INV, 2 MID
  dse::WhtProb* d_wht = nullptr;         // per problem (zero entries: not on that engine)
  bool wht_ready = false;
  int xcd_pairs = 1;                // diagnostics: 0 keeps the two tiles of a problem adjacent
  int mixed_launch = 1;             // persistent: 1- and 2-tile problems of one tile size in one launch
  int span_partial = 1;             // option span_partial: the auto span policy's partial form
  int span_chunks = 2;              // option span_chunks: resident launches the auto policy allows (0-2)
  int span_partial_tile = 11;       // option span_partial_tile: the partial form's tile (10, 11)
  int obs_overlap = 0;              // persistent: observables off the interval launches' stream
  int n_cu = 256;                   // compute units of the device
  int coresident = 0;               // diagnostics: workgroups per 2-tile interval chunk (0: occupancy)
  int handoff_fallbacks = 0;        // this evolve call re-ran on the streaming kernels after a hand-off timeout (0/1)
  bool rerun = false;               // that re-run: the dense engine's results of the first pass are kept
  int* d_err_cur = nullptr;         // the hand-off error word of the running persistent evolve (else null)
  dse::rt::DevBuf<double> d_allreduce;       // RCCL all-reduce staging buffer of the observable sums
  dse::rt::DevBuf<int> d_flags;              // hand-off flags (2 tiles x kIvWaves per problem) + error word
  dse::rt::DevBuf<double2> d_xslots;         // hand-off slots of the interval kernel
  dse::rt::DevBuf<double2> d_xacc;           // intermediate outputs of multi-output launches
  // per-evolve uploads, one device arena each (one copy per evolve, not one per problem)
  dse::rt::DevBuf<unsigned char> d_coef;     // Chebyshev coefficient rows of every problem
  dse::rt::DevBuf<unsigned char> d_sm_coef;  // small-engine coefficients and degrees
  dse::rt::DevBuf<dse::BasisInit> d_init;         // psi(t0) list
  int outputs_per_launch = 2;       // M of the interval kernel (dse_evolve picks 1 on coarse grids)
  int span_outputs = 4;             // M when every register spans (k_span, staggered sums)
  int64_t probe_items = 0;          // 0: all items
  int time_every = 1;               // 0: no kernel timing; N: time intervals with m % N == 0
  double max_degree = 2e6;
  // partitioned registers over processes: one RCCL communicator, one rank per GPU
  ncclComm_t comm = nullptr;
  int dist_rank = 0, dist_world = 1;
  // or a host transport (dse_dist_init_exchange): device data staged through host buffers
  dse_exchange_fn xfn = nullptr;
  void* xuser = nullptr;
  std::vector<unsigned char> xsend, xrecv;
  double xbytes = 0.0;              // bytes this rank sent to other ranks (current evolve)
  // exchange timing (current evolve): HIP event pairs around RCCL calls (summed at the end of
  // dse_evolve) plus host wall time of host-transport exchanges
  std::vector<hipEvent_t> xev;
  size_t xev_used = 0;
  double xms = 0.0;
  // small-register engine
  int dbg = 0;                      // diagnostics switches (option "dbg")
  int small = 1;                    // registers of <= 9 qubits run on dse_small.hip
  int small_chunk = 64;             // output intervals per launch of that engine
  hipStream_t small_stream = nullptr;
  // partitioned registers on the Walsh-Hadamard engine: the index swaps run on swap_stream, one
  // vector's swap under the other vector's pass (option "swap_overlap"); swap_ev orders the two
  int swap_overlap = 1;
  hipStream_t swap_stream = nullptr;
  hipEvent_t swap_ev[8] = {};
  dse::rt::DevBuf<dse::SmallProb> d_small;        // descriptors
  dse::rt::DevBuf<double> d_small_out;       // [problem][n_t][8] raw observable sums
  dse::rt::DevBuf<int> d_small_aux;          // problem selections per register size, interval -> set map
  // dense eigen-propagator engine (dse_dense.h): option "dense" 0 off, 1 when cheaper than the
  // Chebyshev propagator by the cost model of dense_cheaper (default), 2 for every eligible register
  int dense = 1;
  // propagator-matrix mode for a context holding one register on a uniform grid: 0 off, 1 when
  // the model of matrix_cheaper says so (default), 2 whenever eligible
  int matrix = 1;
  // matrix mode's device buffers (U, the states, the products' partial sums, tables), kept across
  // evolves of the same register size (simulate_rare calls one register at a time; a 2^12 register
  // holds 256 MiB of U) and released by dse_destroy or when a larger register needs more
  dse::rt::DevBuf<unsigned char> d_mx;
  // option "symv_fused": each product's reduction inside the product's launch (agent-scope counters
  // with a release per workgroup): measured 22.9 vs 10.4 ms for config 2, so off by default
  int symv_fused = 0;
  double mx_build_ms = 0.0, mx_products_ms = 0.0, mx_products = 0.0, mx_bytes_per_product = 0.0;  // last matrix_run

  // spanning registers (dse_span.hip): option "span" 0 off; s = 1..4: every register that fits
  // runs over 2^s workgroups (one per CU) of 2^(n - s) amplitudes; "span_rb": amplitudes per
  // thread 2^span_rb (0: 512 threads per workgroup)
  int span = 0;
  int span_tile = -1;               // option "span_tile": L > 0 every register of n > L qubits spans 2^(n-L)
                                    // tiles; -1 (default) auto: L = 11 when all tiles fit the chip at once
  // real-component mode (dse_real.hip, option "real", default 0): registers of 13 or 14 qubits with
  // imaginary drives run as two real recurrences, one workgroup per component, no hand-off
  int real_mode = 0;
  // the leap path (option "leap": -1 automatic (default), 0 never, 1 whenever choose_leap's conditions hold)
  int leap = -1;
  int leap_fan = 2;                 // option "leap_fan": workgroups per register and launch on that path (1, 2)
  int leap_problems = 0;            // registers the last evolve ran on it (dse_leap_problems)
  dse::rt::DevBuf<double2> d_real;          // [a | b] inputs and propagator sums of the real-mode registers
  dse::rt::DevBuf<unsigned char> d_real_tab;
  dse::rt::DevBuf<int2> d_real_items;
  int span_rb = 0;
  dse::rt::DevBuf<dse::SpanDesc> d_span;          // per problem
  dse::rt::DevBuf<unsigned char> d_span_tab;
  dse::rt::DevBuf<double2> d_span_slots;     // hand-off slots of the spanned registers
  dse::rt::DevBuf<int> d_span_flags;
  dse::rt::DevBuf<int2> d_span_items;

  hipStream_t dense_stream = nullptr;
  rocblas_handle blas = nullptr;
  // dense engine: registers of >= 2^10 amplitudes are diagonalised up to eig_streams at a time (one
  // host thread, stream and rocBLAS handle each; option "eig_streams", default 3: one N = 14 point
  // of the 30 s grid (two 2^14 registers through the two-stage solver, one 2^13) 4.54 / 4.00 / 3.75 /
  // 3.87 s with 1 / 2 / 3 / 4 streams, profiles/r04/eig_streams_point_2stage.jsonl)
  int eig_streams = 3;
  // dense engine eigensolver: 0 rocSOLVER dsyevd at every size; 1 eig_sym_lower (dse_sytrd.hip: the
  // half-matrix tridiagonalisation from 2^13, rocSOLVER dstedc, the blocked back-transformation)
  // from kEigHalfMinDim amplitudes, dsyevd below; 2 eig_sym_lower from 2^10 (tests)
  int eig_impl = 1;
  // the two-stage eigensolver's cross-workgroup polls give up after this many rounds (option
  // eig_spin_limit; < 0: at once, tests); a give-up re-solves that register with dsyevd
  int eig_spin = dse::kEig2DefaultSpin;
  dse::HandoffKnobs hk;  // options spin_limit, handoff_fences: every persistent launch of this context
  std::atomic<int> eig_fallbacks{0};  // registers re-solved that way in the last evolve
  // dense engine: eigenvalues refined by double-double Rayleigh quotients and output phases reduced
  // in double-double (option "dense_refine", default 1; 0: the eigensolver's eigenvalues and fp64
  // phases, whose error grows like eps |lambda| t: ~1e-8 at the reference grid's 30 s)
  int dense_refine = 1;
  // dense engine: output times of registers of >= kNufftMinDim amplitudes by a type-1 non-uniform
  // FFT on uniform grids (option "dense_nufft": 1 default, from kNufftMinOutputs outputs; 2 every
  // register from two outputs (tests); 0 the [cos | -sin] GEMM for every output), dse_nufft.hip;
  // its rocFFT plans
  int dense_nufft = 1;
  dse::NufftCache* nufft = nullptr;
  int nufft_problems = 0;     // last evolve: registers whose outputs came from the transform
  double dense_out_ms = 0.0;  // last evolve: host wall time of the dense engine's output stage
  std::vector<hipStream_t> eig_st;
  std::vector<rocblas_handle> eig_h;
  // hard pulses (dse_pulse.hip): the table a call's passes read, the events around them, and the last
  // call's passes, HIP-event ms and bytes (dse_pulse_stats); released by dse_destroy
  dse::rt::DevBuf<dse::PulseTab> d_pulse_tab;
  hipEvent_t pulse_ev[2] = {nullptr, nullptr};
  double pulse_stats[3] = {0.0, 0.0, 0.0};
};

#pragma GCC visibility push(hidden)

namespace dse::rt {

inline int fail(dse_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIPC(expr)                                                                      \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return fail(ctx, DSE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Host bytes gathered for one upload: pieces 64-B aligned, offsets into the device arena.
struct Arena {
  std::vector<unsigned char> host;
  size_t add(const void* src, size_t bytes) {
    const size_t off = place(bytes);
    if (bytes) std::memcpy(host.data() + off, src, bytes);
    return off;
  }
  size_t place(size_t bytes) {  // room for a piece filled later
    const size_t off = align_up(host.size(), 64);
    host.resize(off + bytes);
    return off;
  }
};

// One family: raw sums v of a register, comps per unit at v[comps * u + c] and ||psi||^2 at
// v[family_norm_at], `stride` doubles per state; results normalised by that norm (site, pair:
// expectation values, sums / ||psi||^2) or by its square root (overlap: linear in psi).
// The units of site and pair follow from the register's size; the overlap's, the string's and the
// sector's belong to the problem (its K references, its K strings, the U bins of its sets) and their
// strides to the context (K_max, U_max), so both are asked of those.
struct ObsFamilyDesc {
  const char *option, *hook, *noun;  // the option's and the hook's names, the family's word in messages
  int comps;  // site: X Y Z of a bit; pair: ZZ, Re ZQ, Im ZQ, Re DQ, Im DQ of a pair (pair_index);
              // overlap: Re, Im of <phi_k|psi>; string: Re, Im of the string's sum; sector: the bin
  int (*units)(const HostProblem& P);
  int (*stride)(const dse_ctx* ctx, int n);  // of an n-qubit register of ctx
  bool per_problem_units;  // the units are the problem's own count (0: no record) and ||psi||^2 is at
                           // [stride - 2], where every register of the context finds it; else at [comps * units]
  bool amplitude;   // results are sums / ||psi|| instead of sums / ||psi||^2
  int small_stride;                                        // the small engine's stride (its widest register's)
  decltype(&launch_obs_sites) launch;                      // tile engine: S >= stride(n) doubles per tile
  decltype(&launch_dense_obs_sites) launch_dense;          // dense engine and matrix mode: the columns of a DenseCols
  double* DenseProb::*dense_out;                           // where that one writes
  // Where the twins differ.  The site hook refuses only its own register when that is a dist shard,
  // before prepare; the pair hook refuses as the option does (obs_family_refusal), after it
  bool hook_refuses_shard_early;
  // refusal when one output slot of the arena exceeds kPartialCapBytes (pair: up to 2806 doubles per
  // tile; the site arena, at most 104 per tile, takes one slot per flush then)
  bool slot_cap;
  bool get_needs_option;  // the getter refuses once the option is back at 0 (site: serves the last record)
};
inline const ObsFamilyDesc kObsFamilies[kNumObsFamilies] = {
    {"site_obs", "dse_site_observables", "site", 3, [](const HostProblem& P) { return P.n; },
     [](const dse_ctx*, int n) { return site_stride(n); }, false, false,
     kSmallSiteStride, launch_obs_sites, launch_dense_obs_sites, &DenseProb::sites, true, false, false},
    {"pair_obs", "dse_pair_observables", "pair", 5, [](const HostProblem& P) { return P.n * (P.n - 1) / 2; },
     [](const dse_ctx*, int n) { return pair_stride(n); }, false, false, kSmallPairStride, launch_obs_pairs,
     launch_dense_obs_pairs, &DenseProb::pairs, false, true, true},
    // no option: on while the context holds references (dse_set_overlap_refs)
    {"overlap references", "dse_overlaps", "overlap", 2, [](const HostProblem& P) { return P.ovl_k(); },
     [](const dse_ctx* ctx, int) { return overlap_stride(ctx->fam[kOverlap].kmax); }, true, true, kSmallOverlapStride,
     launch_obs_overlap, launch_dense_obs_overlap, &DenseProb::ovl, false, false, true},
    // no option: on while the context holds strings (dse_set_op_strings)
    {"operator strings", "dse_op_string_values", "string", 2, [](const HostProblem& P) { return P.str_k(); },
     [](const dse_ctx* ctx, int) { return string_stride(ctx->fam[kString].kmax); }, true, false, kSmallStringStride,
     launch_obs_strings, launch_dense_obs_strings, &DenseProb::strs, false, false, true},
    // no option: on while the context holds sector sets (dse_set_sectors); a unit is one bin
    {"sector sets", "dse_sector_values", "sector", 1, [](const HostProblem& P) { return P.sec_units(); },
     [](const dse_ctx* ctx, int) { return sector_stride(ctx->fam[kSector].kmax); }, true, false, kSmallSectorStride,
     launch_obs_sectors, launch_dense_obs_sectors, &DenseProb::secs, false, false, true},
};
inline int family_norm_at(const ObsFamilyDesc& F, int units, size_t stride) {
  return F.per_problem_units ? (int)stride - 2 : F.comps * units;
}

// ---- the functions that cross sources, by the source that defines them ---------------------------

// dse_runtime.hip
int upload_arena(dse_ctx* ctx, const Arena& a, DevBuf<unsigned char>& dev, hipStream_t st);
void finish_family_outputs(dse_ctx* ctx, ObsFamily f, size_t pi, const double* raw, size_t stride, int n_t);
void finish_obs(const HostProblem& P, const double* v, double* o, size_t stride);

// dse_rt_small.hip
int small_launch(dse_ctx* ctx, const double* t, int n_t, double tol, double* h_applications, double* launches);
int small_gather(dse_ctx* ctx, int n_t, double* obs_out);

}  // namespace dse::rt

#pragma GCC visibility pop
