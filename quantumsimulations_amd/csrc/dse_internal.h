// dse_internal.h -- device-side data structures shared by the kernels and the runtime.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

namespace dse {

// Chebyshev rows of one register (dse_host.cpp, host only): the series of exp(-i (alpha x + beta) tau)
// on x in [-1, 1] for every offset set_tau[set][j], truncated where dse_bessel_j drops below tol.
// rows: [set][j < M] x (deg + 2) pairs (re, im), [0].re the row's degree, [1 + k] the coefficient
// a_k, zero past the degree and for j >= set_tau[set].size(); *deg the largest row degree (>= 1).
// DSE_ERR_CONVERGENCE when an offset needs more than max_degree terms (*kmax_over: how many),
// DSE_ERR_ARG when dse_bessel_j fails.  Internal to the library (hidden: not an exported symbol).
__attribute__((visibility("hidden"))) int cheb_rows(double alpha, double beta, const std::vector<std::vector<double>>& set_tau, int M, double tol,
              double max_degree, int* deg, std::vector<std::pair<double, double>>* rows, int* kmax_over);
// The series of one offset tau, which cheb_rows, the small-register engine and the propagator-matrix
// mode are built on: a[k] = a_k for k <= *deg (>= 1), the same codes and *kmax_over.  J, if given:
// dse_bessel_j's J_k(alpha tau), k <= *deg, that the a_k were made of.
__attribute__((visibility("hidden"))) int cheb_series(double alpha, double beta, double tau, double tol, double max_degree, int* deg,
                std::vector<std::pair<double, double>>* a, int* kmax_over, std::vector<double>* J = nullptr);

enum { MODE_APPLY = 0, MODE_FIRST = 1, MODE_GEN = 2 };

constexpr int kMinTile = 1;
constexpr int kMaxTile = 13;
constexpr int kRegBits = 4;                       // amplitudes per thread = 2^kRegBits in that kernel
constexpr int kRegAmps = 1 << kRegBits;
constexpr int kRegPairs = kRegBits * (kRegBits - 1) / 2;
constexpr int kRegBlockMinTile = 6 + kRegBits;    // tiles >= 2^10 (>= one wave) use it
// index of the register-bit pair (a, b), a < b, in DevProb::rr_g: (0,1) (0,2) (0,3) (1,2) ...
__host__ __device__ constexpr int rr_index(int a, int b) {
  return a * (2 * kRegBits - a - 1) / 2 + (b - a - 1);
}
constexpr int kXSlots = 4;                        // hand-off ring of the interval kernel
constexpr int kIvWaves = 8;                       // hand-off flags per tile (one per wave of a 2^13 tile)
#ifndef DSE_PIPE
#define DSE_PIPE 1  // interval kernel: software-pipelined partner reads in the fused loop
#endif
constexpr int kMaxOut = 2;      // output times per launch of k_interval / k_real (sums in registers)
constexpr int kSpanMaxOut = 4;  // output times per k_span launch (staggered sums, coef_nterm)
constexpr int kMaxQubits = 34;                    // DSE_MAX_QUBITS
// Site-resolved observables: sums per register and state, X_b Y_b Z_b at [3 b + c] for b < n and
// ||psi||^2 at [3 n], padded to an even count (16-byte records)
__host__ __device__ constexpr int site_stride(int n) { return (3 * n + 2) & ~1; }
// Two-spin correlators: sums per register and state, ZZ, Re ZQ, Im ZQ, Re DQ, Im DQ of the pair
// (i, j), i < j, at [5 pair_index(i, j) + c] and ||psi||^2 at [5 NP], NP = n (n - 1) / 2, padded even
__host__ __device__ constexpr int pair_index(int i, int j) { return j * (j - 1) / 2 + i; }
__host__ __device__ constexpr int pair_stride(int n) { return (5 * (n * (n - 1) / 2) + 2) & ~1; }
// Overlaps with stored reference states: sums per register and state, Re, Im of <phi_k|psi> at [2 k],
// [2 k + 1] for k < K and ||psi||^2 at [S - 2], S = overlap_stride(K_max) doubles per record (K_max: the
// most references any register of the context holds), zero elsewhere
constexpr int kMaxOverlapRefs = 16;               // DSE_MAX_OVERLAP_REFS
__host__ __device__ constexpr int overlap_stride(int kmax) { return 2 * kmax + 2; }
// Operator strings (dse_strings.hip): a product of one-spin operators, one factor per register bit,
// compiled on the host (dse_op_string_masks) into the masks of
//   S = pre * sum_{x : (x & cm) == cv} (-1)^popcount(x & zm) conj(psi_x) psi_{x ^ xm}
// Sums per register and state: Re, Im of S_k at [2 k], [2 k + 1] for k < K and ||psi||^2 at [S - 2],
// S = string_stride(K_max) doubles per record, zero elsewhere
constexpr int kMaxOpStrings = 64;                 // DSE_MAX_OP_STRINGS
__host__ __device__ constexpr int string_stride(int kmax) { return 2 * kmax + 2; }
struct StringEntry {
  uint64_t xm, zm, cm, cv;  // flips, signs, selected bits and their required values in the row x
  double pre_re, pre_im;
};
// Magnetisation-sector populations (dse_sectors.hip): a set is three masks over register bits, m the
// counted bits, cm / cv the selecting bits and their values; its B = popcount(m) + 1 bins are
//   bin_j = sum_{x : (x & cm) == cv, popcount(x & m) == j} |psi_x|^2.
// Sums per register and state: the bins of set 0, then set 1, ... (set k's at [off_k + j]), U = sum_k B_k
// in all, and ||psi||^2 at [S - 2], S = sector_stride(U_max) doubles per record, zero elsewhere
constexpr int kMaxSectorSets = 16;                // DSE_MAX_SECTOR_SETS
__host__ __device__ constexpr int sector_stride(int umax) { return umax + 2; }
struct SectorEntry {
  uint64_t m, cm, cv;  // counted bits, selecting bits and their required values
  int off, bins;       // the set's first unit in the record, popcount(m) + 1
};
constexpr int kMaxShardBits = 3;                  // partitioned registers: up to 8 shards
constexpr int kMaxShards = 1 << kMaxShardBits;
// bits above an L-bit tile for the largest register (34 qubits), at least the 32-bit tile index
#define DSE_MAX_HIGH_BITS(L) ((34 - (L)) < 0 ? 0 : (34 - (L)))

// A pair flip or a drive flip, split into its in-tile mask and its tile-index mask.
//   pair : applies iff bit_i(x) == bit_j(x) <=> popc(x_lo & mask_lo) + popc(h & tile_xor) even
//   flip : coefficient index v = parity(x_lo & mask_lo) ^ parity(h & tile_xor) (output bit value)
struct alignas(16) DPair {
  uint32_t mask_lo;
  uint32_t tile_xor;
  double g;
};
struct alignas(16) DFlip {
  uint32_t mask_lo;
  uint32_t tile_xor;
  double re0, im0, re1, im1;
  double pad;
};

// Register-block kernel: one thread owns the 16 amplitudes x = rho * NT + tid (rho = 0..15),
// i.e. the four top tile bits are "register bits".  For every thread bit j a sweep reads the
// partner thread's 16 amplitudes once from LDS and applies (a) the drive flip of bit j and
// (b) the pair flips (j, register bit i) for i = 0..3.
struct alignas(16) DSweep {
  double re0, im0, re1, im1;  // drive flip on thread bit j (zero when absent)
  double g[kRegBits];         // pair coefficient with register bit i
  uint32_t has_flip;
  uint32_t has_pair;
};

// Chebyshev coefficients of one term k for one interval length.  The propagator sum
// acc = sum_k a_k w_k is accumulated every third term (and at the last term) from the three
// vectors the step kernel holds anyway: acc += c[0] w_{k-2} + c[1] w_{k-1} + c[2] w_k.
// MODE_FIRST (k = 1) writes acc = c[1] w_0 + c[2] w_1.
struct alignas(16) CoefK {
  double2 c[3];
  int upd;
  int pad[3];
};

struct RealTab;

struct DevProb {
  double2* buf[3];
  const double* zzlo;     // [2^L]  sum_{i<j<L} zz_ij s_i s_j
  const double* field;    // [n]
  const double* zz;       // [n*n]
  const DPair* pairs_lo;  // generic kernel: both bits inside the tile
  const DPair* pairs_hi;  // at least one bit above the tile (both kernels)
  const DFlip* flips_lo;  // generic kernel
  const DFlip* flips_hi;  // both kernels
  const DSweep* sweeps;   // register-block kernel: [L-kRegBits] thread-bit sweeps
  const DPair* pairs_tt;  // register-block kernel: pairs between two thread bits
  const double2* coef;    // compact Chebyshev rows, see coef_row / coef_at
  uint64_t sea_mask;
  double shift;
  double beta;            // spectral centre
  double s1;              // 1/alpha
  double rr_g[kRegPairs]; // register-block kernel: pairs among register bits (rr_index order)
  double rflip[kRegBits][4];  // register-block kernel: drive flips on register bits (re0 im0 re1 im1)
  int n, L;
  int n_pairs_lo, n_pairs_hi, n_flips_lo, n_flips_hi, n_pairs_tt;
  int kcap1;
  int degree;             // Chebyshev degree K of the current evolve (terms k = 1..K)
  int rare_bit;
  int n_sea;
  int rflip_mask;         // bit i set: register bit i has a drive flip
  // Partitioned registers (dse_add_problem_sharded): this problem holds shard `rank` of a
  // register whose top `shard_bits` qubits are global.  Tile indices in the kernels are global
  // (hg = h_base | h for local tile h); a tile of shard rank ^ m is read through rbuf[m][role]
  // (the partner's own buffers on the same device, or receive buffers filled by an exchange).
  uint32_t h_base;        // rank << tbl (0 for an ordinary problem)
  int tbl;                // local tile-index bits: log2(tiles of this shard)
  double2* rbuf[kMaxShards][3];
  double2* xslots;        // interval kernel, 2-tile problems: [2][kXSlots][2^L] hand-off slots
  // Multi-output launches: one interval-kernel launch propagates n_out <= n_acc consecutive output
  // times from a shared Chebyshev series.  Output j < n_out - 1 is accumulated in
  // xacc[j << n_local], the last in the next psi buffer.  With the observables overlapped
  // (option obs_overlap) the launches of odd groups (q = 1) use the second set,
  // xacc[(xacc_q + j) << n_local], so group g + 1 never writes what group g's observables read.
  double2* xacc;
  int n_acc;
  int xacc_q;             // 0, or n_acc - 1: intermediate outputs per launch-parity set
  // real-component mode (dse_real.hip): the register's tables, its [a | b] input and the
  // per-output, per-component propagator sums
  const struct RealTab* rtab;
  double* rin;
  double2* racc;
  // the leap path (null otherwise): e^{-i beta (t_m - t0)} of every output m of the evolve, and the
  // history ring of kLeapRing entries of 2^n (p, q)
  const double2* lphase;
  double2* lhist;
  // overlaps with reference states (dse_overlap.hip): the register's (shard's) ovl_k references,
  // 2^n_local amplitudes each (null, 0: none)
  const double2* const* ovl_refs;
  int ovl_k;
  // operator strings (dse_strings.hip): the register's compiled table of str_k entries, masks by
  // register bit (every shard of a loopback register the same table; null, 0: none)
  const StringEntry* str_tab;
  int str_k;
  // sector sets (dse_sectors.hip): the register's table of sec_k entries, masks by register bit
  // (every shard of a loopback register the same table; null, 0: none)
  const SectorEntry* sec_tab;
  int sec_k;
};

// ---- spanning registers (dse_span.hip): one register over 2^s cooperating workgroups ----------
// A register of n qubits is cut into 2^s tiles of L = n - s bits (the top s qubits index the
// tile), one workgroup per tile and compute unit, so one register's Chebyshev chain runs on 2^s
// CUs.  In a tile, thread t of NT = 2^(L - RB) owns the R = 2^RB amplitudes x = r * NT + t.
constexpr int kSpanMaxTop = 4;   // top (tile-index) bits: up to 16 workgroups per register
constexpr int kSpanWaves = 16;   // hand-off flags per tile: one per wave (<= 1024 threads)
constexpr int kSpanMaxIt = 160;  // fused-loop iteration rows (dv2): TB x (4 + pairs per iteration)
constexpr int kSpanMaxOps = kSpanMaxTop + kSpanMaxTop * (kSpanMaxTop - 1) / 2;
// One cross-tile operand of every tile's H application (phase 4 of k_span):
//   kind 0  u_b of the partner h ^ e_b (its slot b): flip_b w + sum_j g_jb [x_j == h_b] w(x ^ e_j)
//   kind 1  the partner's raw w_{k-1} under the drive flip of top bit b (no crossing pairs)
//   kind 2  the raw w_{k-1} of the partner h ^ e_b ^ e_b2: pair (b, b2), applies iff h_b == h_b2
struct alignas(16) SpanOp {
  int kind, b, b2;
  uint32_t pmask;  // partner tile = h ^ pmask
  double c[4];     // kind 1: re0 im0 re1 im1 (by this tile's bit b); kind 2: c[0] = g
};
struct alignas(16) SpanTab {
  double rr_g[6];                   // pairs among register bits (rr_index order)
  double rflip[4][4];               // drive flips on register bits (re0 im0 re1 im1)
  double ug[kSpanMaxTop][16];       // u pre-pass: g_{j,b} for tile bits j < L
  double uflip[kSpanMaxTop][4];     // drive flip of top bit b
  SpanOp ops[kSpanMaxOps];
  int rflip_mask, u_mask, n_ops, need_raw;  // need_raw: some operand reads a partner's raw w
  int n_it, pad[3];
  // iteration j (thread bit j): [0] re0 im0, [1] re1 im1 (drive of j by output value t_j),
  // [2] [3] pairs (j, register bit 0..3), [4 + q] thread pair q of the iteration (mask bits, g)
  double2 it[kSpanMaxIt];
};
// Per-context options of the persistent kernels' cross-workgroup hand-offs, passed with every launch
// (kernel arguments: distinct contexts on one process stay independent)
struct HandoffKnobs {
  int spin_limit = 1 << 22;  // polls of a partner's flag before the hand-off is declared failed
                             // (s_sleep 1 between polls; rounds, not time: include/dse.h); < 0: every wait fails at once
                             // (tests: exercises the fallback to the streaming kernels)
  int fences = 0;            // k_interval: 1 adds an agent release / acquire around each flag
};
struct SpanDesc {
  const SpanTab* tab;
  double2* slots;  // [2^s tiles][s + 1 operand kinds: u_0..u_{s-1}, raw][kXSlots][2^L]
  int* flags;      // [2^s tiles][kSpanWaves]: last term each wave of the tile published
  int s, L;
};
hipError_t launch_span(int L, int RB, bool imag, const DevProb* probs, const SpanDesc* sdesc,
                       const int2* items, int n_items, int q, int set, int n_out, int* err,
                       HandoffKnobs hk, hipStream_t st);
bool span_supported(int L, int RB);
hipError_t set_span_ablate(int mask);
hipError_t set_real_ablate(int mask);
hipError_t span_occupancy(int L, int RB, bool imag, int* blocks_per_cu);

// ---- real-component registers (dse_real.hip) ------------------------------------------------
// With every drive purely imaginary (the sweep's phase pi/2) H' = D H D^dagger, D|x> = i^|x| |x>, is
// REAL symmetric, so T_k(H') maps real vectors to real vectors: the rotated state phi = a + i b
// evolves as two independent real Chebyshev recurrences, T_k(H~') a and T_k(H~') b, whose complex
// propagator sums acc_c = sum_k c_k T_k c give phi(t + tau) = acc_a + i acc_b.  One workgroup per
// real component holds the WHOLE register in LDS (2^14 x 8 B = 128 KiB): no cross-workgroup
// hand-off inside a launch.  Thread t of 512 owns rows x = r * 512 + t, r < R = 2^(n - 9).
constexpr int kRealRB = 5;                  // register bits at n = 14 (R = 32 rows per thread)
constexpr int kRealRegPairs = kRealRB * (kRealRB - 1) / 2;
__host__ __device__ constexpr int real_rr_index(int a, int b) {  // a < b < kRealRB
  return a * (2 * kRealRB - a - 1) / 2 + (b - a - 1);
}
constexpr uint64_t kRealFromBuffer = ~uint64_t(0);
struct alignas(16) RealTab {
  double rr_g[kRealRegPairs];  // rotated pair coefficients (-g) among register bits
  double rflip[kRealRB][2];    // rotated drive of register bit i, by output value (0, 1)
  uint64_t x0;                 // psi(t0) = e_x0; kRealFromBuffer: a custom psi(t0), split from the
                               // state buffer by k_real_split (phi0_x = i^|x| psi0_x)
  int x0pop;                   // popcount(x0): psi = i^{|x0| - |x|} phi (0 with a custom psi(t0))
  int rflip_mask;
  // coefficient row of iteration j (thread bit j), as doubles: the rotated drive of j by output
  // value (2), the rotated pairs (j, register bit 0..5) (6), the iteration's 4 thread pairs in the
  // canonical schedule (span_pair_mask) (4)
  double2 it[9 * 6];
};
// real_c (per problem, real mode): rin = [a | b] (2 x 2^n doubles), racc = [output j][component c]
// blocks of 2^n complex propagator sums
// leap != 0: the leap path's launch (item.y = the workgroup's pair of outputs, below)
hipError_t launch_real(const DevProb* probs, const int2* items, int n_items, int set, int n_out, int leap,
                       hipStream_t st);
// psi = i^{|x0| - |x|} (acc_a + i acc_b) of every output (into the state buffer / intermediate
// outputs k_obs reads) and, from the last output, the next interval's [a | b]
hipError_t launch_real_combine(const DevProb* probs, const int2* items, int n_items, int q, int n_out,
                               hipStream_t st);
hipError_t real_occupancy(int* blocks_per_cu);
hipError_t launch_real_init(const DevProb* probs, const int2* items, int n_items, hipStream_t st);
// after launch_real_init, for the listed registers with a custom psi(t0) (RealTab::x0 ==
// kRealFromBuffer): [a | b] = [Re phi0 | Im phi0] from the state buffer buf[0] (dse_init.hip)
hipError_t launch_real_split(const DevProb* probs, const int2* items, int n_items, hipStream_t st);
// The leap path (uniform grids, basis-state starts; dse_real.hip at k_leap_combine): k_real runs component 0
// alone, rin = p_m, rows without e^{-i beta tau}.  History ring DevProb::lhist: (p, q) of output m in entry
// m % kLeapRing.  A launch at output m0 of n <= kLeapMaxOut outputs reads outputs m0 - 1 .. m0 - n and writes
// m0 + 1 .. m0 + n while output m0 stays for the next launch: 2 n + 1 distinct entries unless m0 + j and
// m0 - j share one (2 j a multiple of the ring), which is j = n = 4 in a ring of eight: read, then
// written, by the same thread.
constexpr int kLeapMaxOut = 4;  // two workgroups per register (option leap_fan = 2), kMaxOut sums each
constexpr int kLeapRing = 8;
constexpr int kLeapKShift = 4;  // a launch item's y: the workgroup's pair of outputs | its degree << kLeapKShift
// p_0 = e_x0 into rin, (e_x0, 0) into history entry 0
hipError_t launch_leap_init(const DevProb* probs, const int2* items, int n_items, hipStream_t st);
// the launch at output m0: outputs m0 + 1 .. m0 + n_out from racc blocks 2 j and the history, psi where
// launch_real_combine writes it, p of the last output into rin
hipError_t launch_leap_combine(const DevProb* probs, const int2* items, int n_items, int q, int n_out, int m0,
                               hipStream_t st);

// Coefficient row of output j of offset set `set`: kcap1 + 1 entries, row[0].x = the degree d of
// that output's series, row[1 + k] = a_k for k = 0..d (zero beyond): 16 B per term.
__host__ __device__ __forceinline__ const double2* coef_row(const DevProb& P, int set, int j) {
  return P.coef + ((size_t)set * P.n_acc + j) * (size_t)(P.kcap1 + 1);
}
// Terms accumulated into a propagator sum at term k (see CoefK), for the update phase ph (0..2):
// 2 at k = 1 (a_0 w_0 + a_1 w_1); then at every k >= 2 with (k - 1 - ph) = 0 mod 3 the terms since
// the previous update (3; at the first update of phase 1 / 2 one / two), and the terms left over at
// k = d; else 0.  A term can reach w_{k-2}, w_{k-1}, w_k, so no gap exceeds 3.  Phase 0 is the
// original schedule (updates at k = 1, 4, 7, ...); k_span staggers output j to phase j % 3, so at
// most ceil(M / 3) of its M sums are read-modify-written in one term.
__host__ __device__ __forceinline__ int coef_nterm(int k, int d, int ph = 0) {
  if (k > d) return 0;
  if (k == 1) return 2;
  const int t = ((k - 1 - ph) % 3 + 3) % 3;
  int last = t == 0 ? k - 3 : k - t;  // the previous update of phase ph at k' >= 2, else 1
  if (last < 2) last = 1;
  return (t == 0 || k == d) ? k - last : 0;
}
// (scalar loads: the row is read-only during a launch and uniform across the workgroup)
__device__ __forceinline__ CoefK coef_at(const double2* row, int k) {
  typedef const __attribute__((address_space(4))) double* kptr;
  const kptr r = (kptr)row;
  const int nt = coef_nterm(k, (int)r[0]);
  CoefK C = {};
  C.upd = nt > 0;
  const size_t o = 2 * (size_t)(k - 1);  // a_{k-2} at row[k - 1]
  C.c[0] = nt >= 3 ? make_double2(r[o], r[o + 1]) : make_double2(0.0, 0.0);
  C.c[1] = nt >= 2 ? make_double2(r[o + 2], r[o + 3]) : make_double2(0.0, 0.0);
  C.c[2] = nt >= 1 ? make_double2(r[o + 4], r[o + 5]) : make_double2(0.0, 0.0);
  return C;
}

// Global tile hp of the role-`role` vector: local buffer or a partner shard's.
__device__ __forceinline__ const double2* tile_ptr(const DevProb& P, int role, uint32_t hp) {
  const uint32_t gm = (hp ^ P.h_base) >> P.tbl;
  const double2* b = gm ? P.rbuf[gm][role] : P.buf[role];
  return b + ((size_t)(hp & ((1u << P.tbl) - 1u)) << P.L);
}

hipError_t launch_step(int L, int mode, const DevProb* probs, const int2* items, int n_items,
                       int k, int q, int set, hipStream_t st);
// diagnostics builds only (-DDSE_DIAG, e.g. DSE_EXTRA_FLAGS for a tools/ variant library): kernel
// section ablation masks; the product library returns hipErrorNotSupported
hipError_t set_ablate(int mask);
hipError_t set_ablate_interval(int mask);
bool interval_supported(int L);
// resident workgroups of k_interval<L> per compute unit (occupancy query)
hipError_t interval_occupancy(int L, bool imag, int* blocks_per_cu);
// imag: every drive coefficient of the launched problems is purely imaginary (HostProblem::imag)
// colstride > 0: column mode (one-tile register, item.y = column, buffers offset by column *
// colstride amplitudes): every column propagated over the interval of coefficient set `set`
hipError_t launch_interval(int L, bool imag, const DevProb* probs, const int2* items, int n_items, int q,
                           int set, int n_out, int* flags, int* err, HandoffKnobs hk, hipStream_t st,
                           long colstride = 0);
// zeroes the interval kernel's hand-off flags of the given items (before a 2-tile launch)
hipError_t zero_flags(const int2* items, int n_items, int* flags, hipStream_t st);
// psi(t0) of many registers in one launch: entry i zeroes ptr[0 .. n) and sets ptr[one_at] = 1
// (one_at < 0: the basis state lies in another shard)
struct BasisInit {
  double2* ptr;
  uint64_t n;
  int64_t one_at;
};
hipError_t launch_basis_init(const BasisInit* list, int n_entries, uint64_t max_amps, hipStream_t st);
// product state psi(g) = prod_b a_b[bit_b(g)] of an n-qubit register into one shard's 2^n_local
// amplitudes (global index g = (shard << n_local) | x); amp: device, [4 n] (re a_b0, im a_b0,
// re a_b1, im a_b1) (dse_init.hip)
hipError_t launch_product_state(double2* out, const double* amp, int n, int n_local, uint64_t shard,
                                hipStream_t st);
// observables of n_out outputs of a group (grid.y): output j < n_out - 1 from intermediate
// accumulator j, the last from state buffer role bsel; output j's partials at partial + j * out_stride.
// This launcher and the five below share their arguments and the kernels' addressing (ObsTile,
// dse_device.h) and dispatch over L through for_tile_bits; each checks its own bounds on S.
hipError_t launch_obs(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                      double* partial, hipStream_t st, int n_out = 1, size_t out_stride = 0,
                      int xq = 0);  // xq: launch parity of the intermediate outputs (xacc_q set)
// site-resolved sums of the same outputs (k_obs_sites): S >= site_stride(n) doubles per tile, output
// j's partials at partial + j * out_stride
hipError_t launch_obs_sites(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                            double* partial, int S, hipStream_t st, int n_out = 1, size_t out_stride = 0,
                            int xq = 0);
// the two-spin sums of the same outputs (k_obs_pairs, dse_pairs.hip): S >= pair_stride(n) doubles per
// tile, output j's partials at partial + j * out_stride
hipError_t launch_obs_pairs(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                            double* partial, int S, hipStream_t st, int n_out = 1, size_t out_stride = 0,
                            int xq = 0);
// the overlaps with the registers' reference states of the same outputs (k_obs_overlap,
// dse_overlap.hip): S = overlap_stride(K_max) doubles per tile, output j's partials at partial + j *
// out_stride; the tiles of a register without references are left unwritten
hipError_t launch_obs_overlap(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                              double* partial, int S, hipStream_t st, int n_out = 1, size_t out_stride = 0,
                              int xq = 0);
// the operator strings of the registers' tables on the same outputs (k_obs_strings, dse_strings.hip):
// S = string_stride(K_max) doubles per tile, output j's partials at partial + j * out_stride; the
// tiles of a register without strings are left unwritten
hipError_t launch_obs_strings(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                              double* partial, int S, hipStream_t st, int n_out = 1, size_t out_stride = 0,
                              int xq = 0);
// the sector populations of the registers' sets on the same outputs (k_obs_sectors, dse_sectors.hip):
// S = sector_stride(U_max) doubles per tile, output j's partials at partial + j * out_stride; the
// tiles of a register without sets are left unwritten
hipError_t launch_obs_sectors(int L, const DevProb* probs, const int2* items, int n_items, int bsel,
                              double* partial, int S, hipStream_t st, int n_out = 1, size_t out_stride = 0,
                              int xq = 0);
// partial[2 * block + {0, 1}] = block sums of Re(conj(a) b) and |a|^2 over n amplitudes
hipError_t launch_dot(const double2* a, const double2* b, size_t n, double* partial, int blocks,
                      hipStream_t st);

// ---- hard pulses (dse_pulse.hip): U = (x)_b U_b in place on a state ------------------------------
constexpr int kPulseTB = 12;          // tile bits of a pass: 2^12 amplitudes, 64 KiB of LDS per workgroup
constexpr int kPulseTile = 1 << kPulseTB;
constexpr int kPulseMinCarry = 2;     // a group of high bits carries at least this many low bits (64-B runs)
constexpr int kPulseMaxGroups = 4;    // group 0 and ceil((34 - 12) / 10) groups of high bits
// what every pass of one call reads from device memory (the parts indexed at run time)
struct PulseTab {
  double2* base[kMaxShards];  // the shards' buffers
  double d[kMaxQubits][4];    // (re u00, im u00, re u11, im u11) of every bit: the diagonal matrices' phase
  double u[kMaxQubits][8];    // every bit's matrix (k_pulse_small)
};
// one pass: the kernel's argument
struct PulsePass {
  int pos[kPulseTB];          // register bit of tile bit q
  double u[kPulseTB][8];      // its matrix
  double2* base0;             // the buffer of an unpartitioned register
  uint64_t outer;             // the register bits outside the tile (the workgroup index is spread over them)
  uint64_t diag;              // the bits whose diagonal matrix this pass applies (0: another pass does)
  uint32_t bfly;              // the tile bits this pass transforms
  int n_local, shard_bits;
};
struct PulseGroup {
  int c;                      // carried low bits (0: group 0 and the small path)
  int pos[kPulseTB];          // register bit of tile bit q (-1: none, registers of fewer than 12 bits)
  uint32_t bfly;              // the tile bits the pass transforms
  uint64_t active;            // the register bits it is launched for
};
struct PulsePlan {
  int passes;
  bool small;                 // the whole register in one workgroup (k_pulse_small)
  PulseGroup grp[kPulseMaxGroups];
};
int pulse_plan(int n_local, int shard_bits, uint64_t active, uint64_t diag, PulsePlan& plan);
hipError_t launch_pulse(double2* const* base, int n_local, int shard_bits, const double* u, uint64_t active,
                        uint64_t diag, PulseTab* tab, hipStream_t st, int* passes);

}  // namespace dse
