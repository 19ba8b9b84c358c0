/*
 * dse.h -- C ABI of the MI355X dipolar spin-ensemble state-vector engine (libdse.so).
 *
 * The reference has no native boundary: its only solver entry is the Python call
 *   simulate_rare(params) -> (t, obs)          dipolar_ensemble_with_rare.py:611-680
 * which builds H with QuTiP (:453-588), prepares psi0 (:591-606) and hands both to
 *   qt.sesolve(H, psi0, t, e_ops=[6 ops], options)   dipolar_ensemble_with_rare.py:653-666
 * The functions below replace that sesolve call (and the operator algebra feeding it)
 * for any number of independent evolutions per device.  The Python host
 * (quantumsimulations_amd/dipolar_ensemble_with_rare.py) reduces a DipolarRareParams to the
 * coefficient tables taken by dse_add_problem and calls dse_evolve; INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - A problem is an n-qubit register, state = 2^n complex doubles, interleaved (re, im).
 *   - s_b(x) = 1/2 - bit_b(x); bit value 0 = spin up (QuTiP basis(2, 0)).
 *   - H x-th row:  D(x) psi[x]
 *                + sum_b flip(b, bit_b(x)) psi[x ^ e_b]
 *                + sum_{i<j, bit_i(x)==bit_j(x)} pair[i][j] psi[x ^ e_i ^ e_j]
 *     D(x) = shift + sum_b field[b] s_b(x) + sum_{i<j} zz[i][j] s_i(x) s_j(x).
 *     flip is given as 4 doubles per bit: (re0, im0, re1, im1) where index v = bit_b(x) is the
 *     bit value of the OUTPUT row; H must be Hermitian: (re1, im1) = conj(re0, im0).
 *   - Observables (dse_obs order = the key order of simulate_rare's dict, :671-679):
 *       Ix_sea, Iy_sea, Iz_sea: sums over the bits of sea_mask;  Iz_R, Ix_R, Iy_R on rare_bit
 *       (rare_bit < 0: the rare spin is not in the register; Iz_R = rare_z_const, Ix_R = Iy_R = 0);
 *       state_norm = ||psi||.  Expectations are of the normalised state (QuTiP 5 normalize_output).
 *   - Status: 0 = ok, negative = error; dse_last_error(ctx) has the message.  No C++ exception
 *     crosses this boundary.
 *   - Threading: a context is bound to one device and is not thread-safe; distinct contexts are.
 *     Calls block until results are in host memory.
 */
#ifndef DSE_H
#define DSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSE_ABI_VERSION 14
/* Additions that leave every existing entry as it is (new functions, fields appended to dse_stats)
 * raise the minor number; a caller checks dse_abi_version() == DSE_ABI_VERSION and
 * dse_abi_minor() >= the DSE_ABI_MINOR it was built against.  14.1: initial states other than a
 * basis state (dse_set_initial_state, ...; dse_stats.custom_init_problems).
 * Later additions leave both numbers and dse_stats alone (custom_init_problems stays its last field):
 * a caller discovers them by name with dse_has_feature, and what would have been a stats counter is
 * a getter (the two-spin correlators: option "pair_obs", dse_pair_obs_problems; the overlaps with
 * reference states: feature "overlap_obs", dse_overlap_problems; the operator strings: feature
 * "op_strings", dse_op_string_problems; the sector populations: feature "sector_obs",
 * dse_sector_problems; the leap path on uniform grids: feature "leap", options "leap" and "leap_fan",
 * dse_leap_problems, and the host-only dse_uniform_spacing). */
#define DSE_ABI_MINOR 1
#define DSE_MAX_QUBITS 34
#define DSE_N_OBS 7
#define DSE_MAX_OVERLAP_REFS 16 /* reference states per problem (dse_set_overlap_refs) */
#define DSE_MAX_OP_STRINGS 64   /* operator strings per problem (dse_set_op_strings) */
#define DSE_MAX_SECTOR_SETS 16  /* sector sets per problem (dse_set_sectors) */

enum dse_status {
  DSE_OK = 0,
  DSE_ERR_ARG = -1,         /* invalid argument (reference: ValueError, :620-621)           */
  DSE_ERR_OOM = -2,         /* device or host allocation failed                             */
  DSE_ERR_HIP = -3,         /* HIP runtime error                                             */
  DSE_ERR_CONVERGENCE = -4, /* Chebyshev degree cap exceeded (reference: sesolve failure)    */
  DSE_ERR_STATE = -5,       /* call order (e.g. dse_get_state before dse_evolve)             */
  DSE_ERR_NODEVICE = -6     /* no HIP device / bad device index                             */
};

enum dse_obs {
  DSE_OBS_IX_SEA = 0,
  DSE_OBS_IY_SEA = 1,
  DSE_OBS_IZ_SEA = 2,
  DSE_OBS_IZ_R = 3,
  DSE_OBS_IX_R = 4,
  DSE_OBS_IY_R = 5,
  DSE_OBS_NORM = 6
};

typedef struct dse_ctx dse_ctx;

/* Per-call counters filled by dse_evolve (all sums over every problem of the context). */
typedef struct dse_stats {
  double h_applications;      /* Chebyshev terms = applications of H, summed over problems     */
  double amplitude_updates;   /* sum over step launches of the amplitudes they updated          */
  double step_bytes;          /* algorithmic HBM bytes of all step launches (80 B / amplitude)  */
  double step_kernel_ms;      /* summed HIP-event time of the timed launches of the dominant    */
                              /* kernel (streaming: k_step_rb, k >= 2; persistent: k_interval)  */
  double step_launches;       /* launches of the dominant kernel                                */
  double timed_launches;      /* dominant-kernel launches bracketed by HIP events               */
  double timed_bytes;         /* algorithmic bytes of the timed launches                        */
  double wall_ms;             /* host wall time of the call                                     */
  double h_flops;             /* algorithmic flops of all H applications (4 + 8/drive + 2/pair  */
                              /* per amplitude)                                                 */
  double timed_flops;         /* algorithmic flops of the timed launches                        */
  double timed_amp_terms;     /* amplitudes x Chebyshev terms of the timed launches (SURVEY.md  */
                              /* §8(d) prices a fused Chebyshev term at 80 B per amplitude)     */
  double exchange_bytes;      /* partitioned registers over processes: bytes this rank sent to  */
                              /* other ranks (index swaps / shard exchanges)                     */
  int32_t max_degree;         /* largest Chebyshev degree of any problem / interval             */
  int32_t n_intervals;        /* output intervals propagated                                    */
  int32_t tile_bits;          /* LDS tile of the first problem (log2 amplitudes per workgroup)  */
  int32_t streams;            /* HIP streams ("lanes") the problems were spread over            */
  int32_t mode;               /* 0: per-term streaming kernels, 1: persistent interval kernel, 
                                 2: streaming with the Walsh-Hadamard engine, 3: every problem on
                                 the small-register engine, 4: every problem on the dense
                                 engine (or small and dense), 5: the context's register in
                                 propagator-matrix mode (U = exp(-iH dt) built column-parallel,
                                 outputs by repeated products; option "matrix")                 */
  int32_t outputs_per_launch; /* persistent mode: output times per launch (shared series)   */
  int32_t handoff_fallbacks;  /* 1: this call re-ran on the streaming kernels after a          */
                              /* cross-tile hand-off timed out (device shared with other work)  */
  int32_t dense_problems;     /* problems this call ran on the dense eigen-propagator engine    */
                              /* (option "dense")                           */
  int32_t span_problems;      /* registers this call ran spread over 2^s workgroups (k_span,  */
                              /* option "span"; ABI 9)                                          */
  double dense_ms;            /* host wall time of the dense engine (all of its device work)    */
  double dense_eig_ms;        /* of which the eigendecompositions (rocSOLVER dsyevd)            */
  double exchange_ms;         /* partitioned registers over processes: time of the exchanges    */
                              /* (HIP events around each RCCL call on its stream; host wall     */
                              /* time of each host-transport exchange)                           */
  double lane0_kernel_ms;     /* the timed launches of stream ("lane") 0 alone: summed HIP-event */
  double lane0_launches;      /* time, their count and their amplitudes x terms -- in persistent */
  double lane0_amp_terms;     /* mode lane 0 holds the 2-tile registers (the critical stream)    */
  double matrix_build_ms;     /* propagator-matrix mode (mode 5): HIP-event time of the column   */
  double matrix_products_ms;  /* build of U (k_ucols) and of all products psi_{j+1} = U psi_j    */
  double matrix_products;     /* (k_symv + k_symv_reduce, or zgemv), their count, and the        */
  double matrix_bytes_per_product; /* bytes one product reads (U's stored tiles + x; ABI 10)     */
  int32_t real_problems;      /* registers run as two real recurrences in the rotated frame      */
                              /* (k_real, option "real"; ABI 11)                                 */
  int32_t eig_fallbacks;      /* dense registers whose two-stage eigensolve gave up a bounded     */
                              /* cross-workgroup poll and were re-solved by rocSOLVER dsyevd     */
                              /* (option "eig_spin_limit"; ABI 12)                                */
  int32_t dense_nufft_problems; /* dense registers whose output times came from the non-uniform  */
                              /* FFT instead of the GEMM (option "dense_nufft"; ABI 13)           */
  int32_t site_obs_problems;  /* registers whose site-resolved sums this call produced (option  */
                              /* "site_obs"; a loopback partitioned register counts once; ABI 14) */
  double dense_output_ms;     /* host wall time of the dense engine's output stage (refinement,   */
                              /* transform or GEMM, observables)                                   */
  int32_t custom_init_problems; /* registers this call started from anything other than the basis  */
                              /* state psi0_index (dse_set_initial_state / _product /              */
                              /* dse_continue_from_final; a loopback partitioned register counts   */
                              /* once; ABI 14.1)                                                   */
} dse_stats;

/* ---- library / device ------------------------------------------------------------------- */
int dse_abi_version(void);
int dse_abi_minor(void);
int dse_device_count(void);                 /* number of HIP devices, 0 if none              */
/* free_total[0] = free, free_total[1] = total device memory in bytes (hipMemGetInfo), so a caller
 * can batch evolutions to fit HBM. */
int dse_device_memory(int device, double* free_total /* [2] */);

/* ---- host-only helpers (no device needed; also used by the tests) ------------------------- */
/* Rigorous spectral bounds of the H defined by the tables (Weyl's inequality over the 1- and
 * 2-qubit pieces; exact for the non-interacting part).  Arrays as in dse_add_problem. */
int dse_spectral_bounds(int n_qubits, const double* field, const double* zz, const double* pair,
                        const double* flip, double shift, double* e_min, double* e_max);
/* Bessel J_k(z), k = 0..kmax (Miller's backward recurrence, normalised by
 * J_0 + 2 sum J_2k = 1).  *degree = the Chebyshev truncation degree for tolerance tol
 * (largest k with |J_k(z)| > tol, at least 1). */
int dse_bessel_j(double z, int kmax, double* out, double tol, int* degree);

/* ---- context ------------------------------------------------------------------------------ */
dse_ctx* dse_create(int device);            /* NULL on failure, see dse_create_error()       */
const char* dse_create_error(void);
void dse_destroy(dse_ctx* ctx);
const char* dse_last_error(const dse_ctx* ctx);
/* Options: "tile_bits"    LDS tile, log2 amplitudes per workgroup, 1..13 (default 13)
 *          "streams"      HIP streams the problems are spread over, 1..16 (default 4)
 *          "persistent"   1 (default): one persistent launch per group of output intervals
 *                         when every problem fits one or two LDS tiles (n <= tile_bits + 1);
 *                         0: per-term streaming launches
 *          "outputs_per_launch"  persistent mode: up to this many (1..2) consecutive output
 *                         times from one Chebyshev series (default 2; 1 on coarse grids,
 *                         alpha dt >= 400)
 *          "wht"          1 (default): streaming registers of more than one tile apply H as
 *                         D_Z + W D_X W + V D_Y V^+ (Walsh-Hadamard passes, two extra state-sized
 *                         vectors per problem, four per shard of a partitioned register; a problem
 *                         whose vectors do not fit in HBM keeps the step kernels); 0: step kernels
 *          "wht_tile_bits"   tile of that engine: 12 (two workgroups per CU), 13, or 0 (default:
 *                         13)
 *          "wht_group_bits"  high qubits transformed per pass of that engine, 2..11, or 0
 *                         (default: tile bits - 2)
 *          "swap_overlap" partitioned registers on that engine: 1 (default) the X- and Y-branch
 *                         vectors take separate passes and each one's index swap runs on a
 *                         second stream under the other's pass; 0: both swapped between passes
 *          "time_kernels" 0 = off, N = bracket the step launches of every N-th interval with
 *                         HIP events (default 1)
 *          "max_degree"   Chebyshev degree cap per interval (default 2e6)
 *          "obs_overlap"  persistent mode: 1 runs each interval group's observables on a second
 *                         stream per lane (lowest priority) while the next group's launches run,
 *                         with two sets of intermediate-output accumulators; 0 (default) in line
 *          "mixed_launch" persistent mode: 1 (default) puts the 1- and 2-tile problems of one tile
 *                         size in one interval launch (stiffest pairs, 1-tile problems, remaining
 *                         pairs) when all 2-tile workgroups fit at once; 0 one stream each
 *          "handoff_fences"  persistent mode, 2-tile registers: 0 (default) the sc1 hand-off
 *                         (write-through payload, per-wave vmcnt(0) + barrier, sc1 flag and
 *                         poll); 1 adds an agent-scope release before every flag store and an
 *                         acquire after every poll
 *          "wht_persist"  Walsh-Hadamard engine: bit 1 runs MID as a persistent launch (one
 *                         workgroup per CU looping over tiles, next tile's loads under the other
 *                         vector's transposes); 0 (default).  The half-LDS MID ("wht_half" bit 2,
 *                         on by default) takes precedence: bit 1 here has an effect only with
 *                         "wht_half" bit 2 cleared
 *          "wht_fuse"     Walsh-Hadamard engine, unpartitioned registers: 1 (default) the FINAL pass
 *                         of term k also runs term k + 1's FIRST on the new vector while it is in
 *                         registers (one read of it and one launch less per term; the group-0
 *                         butterflies in another order: results agree to rounding); 0 separate
 *                         passes.  Decided once per lane group for a whole evolve: a group that
 *                         contains any partitioned register runs unfused on every term, its
 *                         unpartitioned registers included
 *          "wht_mid_inpage"  Walsh-Hadamard plan: the MID group's high bits below the 2-MiB page
 *                         (0 default; measured slower, kept for experiments)
 *          "wht_half"     Walsh-Hadamard engine, 13-bit tiles: passes with one vector in registers
 *                         and the LDS transposes in halves (real, then imaginary parts), two
 *                         workgroups per CU: bit 0 FIRST, bit 1 FWD / INV, bit 2 MID (default 7;
 *                         0 the one-workgroup-per-CU passes); results bitwise identical.  Bit 2
 *                         takes precedence over "wht_persist" bit 1: while it is set, MID is never
 *                         the persistent launch
 *          "dense"        dense eigen-propagator: 0 off, 1 by cost model (default), 2 always
 *          "eig_streams"  dense engine: eigendecompositions of registers of >= 2^10 amplitudes
 *                         run this many at a time, one stream and rocBLAS handle each, 1..8
 *                         (default 3)
 *          "eig_impl"     dense engine eigensolver: 0 rocSOLVER dsyevd; 1 (default) for
 *                         registers of >= 2^11 amplitudes a tridiagonalisation (the half-matrix
 *                         one of dse_sytrd.hip from 2^13, rocSOLVER's below), rocSOLVER dstedc
 *                         and a blocked back-transformation, dsyevd below 2^11, and from 2^13
 *                         the two-stage solver of dse_eig2.hip (dense -> band 32 -> tridiagonal
 *                         by bulge chasing, dstedc, both back-transformations); 2 the half-matrix
 *                         path from 2^10; 3 the two-stage solver from 2^10.  Costs one extra
 *                         dim x dim matrix per solver stream (two-stage: two, plus ~n^2 / 2 for
 *                         the chase's reflectors)
 *          "matrix"       propagator-matrix mode for a lone register: 0 off, 1 by model
 *                         (default), 2 whenever eligible
 *          "symv_fused"   propagator-matrix mode: 1 sums each product's partials inside the
 *                         product's launch (agent-scope counters); 0 (default) a second launch
 *          "real"         1: registers of 13 / 14 qubits whose drives are all imaginary
 *                         (the sweep's phase pi/2) run in the rotated frame, where H is real: two
 *                         real Chebyshev recurrences, one workgroup each holding the whole
 *                         register in LDS (k_real, dse_real.hip); 2: only the 2-tile (14-qubit)
 *                         registers real, beside the 13-qubit ones on the 1-tile k_interval;
 *                         0 (default): the complex kernels (k_real measured at the 2-tile
 *                         k_interval's CU cost: slower on the bench's mix, 1 and 2 alike)
 *          "leap"         the leap path (feature "leap"): on a uniform output grid, from basis states, with
 *                         imaginary drives, the rotated state is chi = p + i q with p = cos(H' (t - t0)) e_x0
 *                         and q = -sin(H' (t - t0)) e_x0 real, and p_{m+j} = 2 C_j p_m - p_{m-j},
 *                         q_{m+j} = q_{m-j} - 2 S_j p_m: a launch runs ONE real Chebyshev recurrence per
 *                         register (k_real's kernel on p_m alone, no cross-workgroup hand-off) and
 *                         k_leap_combine forms the outputs from a ring of earlier ones.  1: whenever the
 *                         evolve is persistent without obs_overlap, every Chebyshev register has 13 or
 *                         14 qubits, imaginary drives and its basis state as psi(t0), outputs_per_launch
 *                         is 2 (one output per series doubles the launches the recurrence's rounding
 *                         grows over), alpha dt leap_fan < 400 and
 *                         max_m |t_m - (t_0 + m dt)| <= 2 ulp(|t_last|), dt = (t_last - t_0) / (n_t - 1);
 *                         otherwise, and with 0, the other options' choice runs unchanged, bitwise.
 *                         -1 (default): as 1, but only where the automatic layout policy decides, i.e.
 *                         with span_tile = -1, real = 0 and spin_limit, handoff_fences, xcd_pairs,
 *                         coresident at their defaults.  dse_leap_problems counts its registers
 *          "leap_fan"     the leap path: 1 one workgroup per register and launch, two outputs; 2
 *                         (default) a second workgroup for the offsets 3 dt, 4 dt from the same p_m:
 *                         four outputs per launch (stats outputs_per_launch = 4), a chain of
 *                         K(4 dt) instead of 2 K(2 dt) terms per four outputs on twice the
 *                         workgroups, and half the launches for the recurrence's rounding to grow
 *                         over (0.4 to 0.9 % faster than 1 on the bench's 192 registers); the
 *                         path's condition is then alpha dt < 200
 *          "spin_limit"   persistent kernels: polls of a partner workgroup's flag before a
 *                         cross-tile hand-off is declared failed (default 2^22 poll rounds, each an s_sleep 1 and
 *                         one flag load, so its wall time is set by that load's latency; the call
 *                         then re-runs on the streaming kernels, stats handoff_fallbacks);
 *                         -1: every hand-off fails at once (tests)
 *          "ablate", "span_ablate", "real_ablate"  diagnostics builds only (-DDSE_DIAG): skip
 *                         kernel sections for timing (results become wrong); DSE_ERR_ARG here
 *          "span_tile"    L > 0 (10 or 11): every register of n > L qubits runs over 2^(n - L)
 *                         cooperating workgroups, one per CU, with per-term cross-tile hand-offs
 *                         (k_span, dse_span.hip): a shorter chain per register for few registers
 *                         (one simulate_rare call, one GPU's share of a strong split); -1
 *                         (default): when every Chebyshev register of the evolve is 12..15 qubits,
 *                         L = 10 if all their tiles fit one per CU, else L = 11 if they fit the
 *                         chip at once; else the partial form (option span_partial); else L = 11
 *                         in two resident launches per interval; else none; 0 never
 *          "span_partial" 1 (default): the auto policy's partial form -- when not every register
 *                         fits spanned in one launch, the registers with the longest predicted
 *                         chains (spectral half-width x measured term time) span over
 *                         2^span_partial_tile-amplitude tiles on a stream of their own beside
 *                         k_interval, as long as every workgroup of both launches fits the chip
 *                         and the longest chain shrinks by 10% (one GPU's share of a 2- or 4-GPU
 *                         strong split); 0 off
 *          "span_chunks"  resident launches per interval the auto policy allows for every
 *                         register spanned (0, 1, 2; default 2)
 *          "span_partial_tile"  log2 tile of the partial form (10 or 11, default 11)
 *          "span"         the same with a fixed number s = 1..4 of top bits per register
 *          "span_rb"      k_span's rows per thread 2^span_rb (0: 512 threads per workgroup)
 *          "span_outputs" outputs per launch (1..4, default 4) of an evolve whose registers all
 *                         span: k_span staggers the outputs' sums over the terms, so more
 *                         outputs per Chebyshev series cost no extra registers
 *          "eig_spin_limit"  two-stage eigensolver: rounds a poll of another workgroup's result
 *                         waits before it gives up (default 2^22 poll rounds, each one buffer load of the
 *                         polled value; counted in rounds, not time, as spin_limit); a give-up voids that
 *                         solve and the register is re-solved by rocSOLVER dsyevd (stats
 *                         eig_fallbacks); -1: every solve gives up at once (tests)
 *          "dense_nufft"  dense engine: output times of registers of >= 2^10 amplitudes on a
 *                         uniform grid (np.linspace: tau_j = j s + delta_j, |delta_j| an ulp) by a
 *                         type-1 non-uniform FFT of the eigenvalue phases (spreading, rocFFT,
 *                         deconvolution; ~1e11 flops per 2^14 register) instead of the
 *                         [cos | -sin] GEMM (4 dim^2 T flops): 1 (default) from 2048 outputs, 2
 *                         every register from two outputs (tests), 0 never (stats
 *                         dense_nufft_problems; ABI 13)
 *          "dense_refine" dense engine: 1 (default) eigenvalues refined by double-double
 *                         Rayleigh quotients (exact diagonal) and output phases reduced modulo
 *                         2 pi in double-double; 0 the eigensolver's values and fp64 phases
 *          "site_obs"     0 (default): the seven aggregates only; 1: dse_evolve also keeps, for every
 *                         register and output time, <Ix_b>, <Iy_b>, <Iz_b> of every register bit b
 *                         (the definitions above, of the normalised state), read back with
 *                         dse_get_site_obs.  The aggregates are bitwise what they are with 0, and
 *                         the option does not influence which engine a register runs on.  Costs one
 *                         more read of the state per output (plus n - L partner-tile reads per tile)
 *                         and a second partial arena of 3 n_max + 1 doubles per tile and output
 *                         slot (capped at 256 MiB like the first).  Not available for a register
 *                         partitioned over processes (shard_rank >= 0): dse_evolve returns
 *                         DSE_ERR_ARG; any value but 0 or 1 is DSE_ERR_ARG (ABI 14)
 *          "pair_obs"     0 (default); 1: dse_evolve also keeps, for every register and output time,
 *                         the two-spin correlators of every pair of register bits i < j (5 sums per
 *                         pair, see dse_pair_observables), read back with dse_get_pair_obs.  The
 *                         aggregates and the "site_obs" traces are bitwise what they are with 0,
 *                         and the option does not influence which engine a register runs on; with
 *                         0 nothing is allocated and no kernel is added.  Costs one partner read per
 *                         amplitude with bit_i = 0 and pair, and a third partial arena of
 *                         5 n_max (n_max - 1) / 2 + 1 doubles (padded even) per tile and output
 *                         slot.  dse_evolve returns DSE_ERR_ARG for a context holding a register
 *                         partitioned over processes (shard_rank >= 0) and for one whose arena
 *                         would exceed 256 MiB for a single output slot (at 2^13-amplitude tiles:
 *                         registers above about 27 qubits); any value but 0 or 1 is DSE_ERR_ARG
 *                         (feature "pair_obs") */
int dse_set_option(dse_ctx* ctx, const char* key, double value);

/* ---- problems ----------------------------------------------------------------------------- */
/* Adds an evolution to the context.  field[n], zz[n*n] and pair[n*n] (row-major, upper
 * triangle i<j read), flip[4n].  Returns the problem id (>= 0) or a negative status. */
int dse_add_problem(dse_ctx* ctx, int n_qubits, const double* field, const double* zz,
                    const double* pair, const double* flip, double shift, uint64_t psi0_index,
                    uint64_t sea_mask, int rare_bit, double rare_z_const);
int dse_num_problems(const dse_ctx* ctx);
int dse_clear(dse_ctx* ctx);

/* ---- partitioned registers (SURVEY.md §8(e), configs with N >= 28) ----------------------------
 * A register whose top shard_bits (1..3) qubits are "global": shard r holds the 2^(n-shard_bits)
 * amplitudes whose global bits equal r.  Same tables as dse_add_problem.
 *   shard_rank = -1  all 2^shard_bits shards in this context (one device); terms that cross
 *                    shards read the partner shard's buffers directly.  Returns the id of shard 0;
 *                    the other shards take the next ids.  Every shard's row of obs_out holds the
 *                    observables of the whole register; dse_apply_h / dse_observables /
 *                    dse_get_state on shard 0 take and return the whole 2^n state.
 *   shard_rank >= 0  this context holds shard shard_rank of a register partitioned over
 *                    processes (one per GPU, rank = shard_rank, world = 2^shard_bits) joined by
 *                    dse_dist_init; before every Chebyshev term the shards that terms couple
 *                    exchange their current vector with RCCL send/recv, and the observable sums
 *                    are all-reduced.  dse_get_state returns the local shard (2^(n-shard_bits)).
 * No reference counterpart: replaces QuTiP's single-process CSR product at sizes it cannot hold. */
int dse_add_problem_sharded(dse_ctx* ctx, int n_qubits, const double* field, const double* zz,
                            const double* pair, const double* flip, double shift,
                            uint64_t psi0_index, uint64_t sea_mask, int rare_bit,
                            double rare_z_const, int shard_bits, int shard_rank);
/* RCCL bootstrap: rank 0 creates the id (DSE_DIST_ID_BYTES bytes), every rank passes it to
 * dse_dist_init with its rank and the world size (out-of-band broadcast, e.g. torch.distributed). */
#define DSE_DIST_ID_BYTES 128
int dse_dist_unique_id(unsigned char* id_out);
int dse_dist_init(dse_ctx* ctx, int rank, int world, const unsigned char* id);
/* The same with a host transport instead of RCCL (tests, or a deployment without RCCL between
 * the devices): every exchange is handed to fn on the calling host thread with HOST buffers (the
 * library stages device data through them; fn must not call back into libdse):
 *   DSE_XCHG_ALLTOALL      send/recv hold world chunks of `bytes` each, chunk p goes to rank p
 *   DSE_XCHG_SENDRECV      send `bytes` to rank `peer` and receive `bytes` from it into recv
 *   DSE_XCHG_ALLREDUCE_F64 sum bytes / 8 doubles in place over all ranks (send == recv)
 * Every rank issues the same sequence of calls.  fn returns 0 on success. */
enum dse_exchange_op { DSE_XCHG_ALLTOALL = 1, DSE_XCHG_SENDRECV = 2, DSE_XCHG_ALLREDUCE_F64 = 3 };
typedef int (*dse_exchange_fn)(void* user, int op, void* send, void* recv, uint64_t bytes, int peer);
int dse_dist_init_exchange(dse_ctx* ctx, int rank, int world, dse_exchange_fn fn, void* user);
/* Local state size (amplitudes) of a problem: 2^n, or 2^(n - shard_bits) for a dist shard. */
int64_t dse_problem_dim(const dse_ctx* ctx, int problem);

/* Diagnostics (host only, no device): the Walsh-Hadamard engine's pass plan for a register of
 * n_local local qubits (shard_bits of them global), tile_bits 12 or 13, max_bits high qubits per
 * pass (0: tile_bits - 2).  Writes groups_out[g][0] = carried low bits c, [g][1 + q] = the local
 * qubit of tile bit q (q < tile_bits), for g < G; returns G (group 0 = FIRST/FINAL, 1..G-2 =
 * FWD/INV, G-1 = MID), or 0 when the engine cannot take the register. */
int dse_wht_plan(int n_local, int shard_bits, int tile_bits, int max_bits, int32_t* groups_out /* [4][14] */);

/* ---- hot path ----------------------------------------------------------------------------- */
/* psi_out = H psi_in for one problem (interleaved complex, 2^n each).  Test/diagnostic hook:
 * runs the same matrix-free tile kernel as the propagator. */
int dse_apply_h(dse_ctx* ctx, int problem, const double* psi_in, double* psi_out);
/* The 7 observables of an arbitrary state of one problem (same kernel as dse_evolve). */
int dse_observables(dse_ctx* ctx, int problem, const double* psi, double* obs7);
/* The site-resolved sums of an arbitrary state of one problem: out[3][n], component 0 Ix, 1 Iy,
 * 2 Iz of register bit b, of the normalised state (the hook beside dse_observables; runs the
 * kernel of the option "site_obs" whatever the option's value; a loopback partitioned register:
 * shard 0's id and the whole 2^n state; not available for a dist shard, DSE_ERR_ARG). */
int dse_site_observables(dse_ctx* ctx, int problem, const double* psi, double* out);
/* The two-spin correlators of an arbitrary state of one problem: out[5][NP], NP = n (n - 1) / 2,
 * pair (i, j) of register bits i < j at p = j (j - 1) / 2 + i.  With s_b(x) = 1/2 - bit_b(x),
 * y = x ^ e_i ^ e_j and every sum divided by ||psi||^2:
 *   component 0     ZZ = <Iz_i Iz_j>  = sum_x |psi_x|^2 s_i(x) s_j(x)
 *   components 1, 2 Re, Im of ZQ = <I+_i I-_j> = sum_{bit_i(x)=0, bit_j(x)=1} conj(psi_x) psi_y
 *   components 3, 4 Re, Im of DQ = <I+_i I+_j> = sum_{bit_i(x)=0, bit_j(x)=0} conj(psi_x) psi_y
 * so <IxIx> = (Re ZQ + Re DQ) / 2, <IyIy> = (Re ZQ - Re DQ) / 2, <Ix_i Iy_j> = (Im DQ - Im ZQ) / 2,
 * <Iy_i Ix_j> = (Im DQ + Im ZQ) / 2, and with the sums of dse_site_observables
 *   <H> = shift + sum_b field[b] Z_b + 2 sum_b (flip[4b] X_b - flip[4b+1] Y_b)
 *         + sum_{i<j} zz[i][j] ZZ_ij + 2 sum_{i<j} pair[i][j] Re DQ_ij.
 * The hook beside dse_site_observables: runs the kernel of the option "pair_obs" whatever the
 * option's value; a loopback partitioned register: shard 0's id and the whole 2^n state.
 * DSE_ERR_ARG for a context holding a register partitioned over processes, and where the option
 * itself would be refused for the arena's size. */
int dse_pair_observables(dse_ctx* ctx, int problem, const double* psi, double* out);
/* Evolves every problem from its initial state at t[0] (the basis state psi0, or the state set by
 * dse_set_initial_state / dse_set_initial_product / dse_continue_from_final) through the output
 * times t[0..n_t) (strictly increasing) with an exact Chebyshev propagator (truncation tolerance
 * tol, e.g. 1e-14) and writes obs_out[problem][DSE_N_OBS][n_t].  stats may be NULL. */
int dse_evolve(dse_ctx* ctx, const double* t, int n_t, double tol, double* obs_out,
               dse_stats* stats);
/* After dse_evolve with option "site_obs" = 1: out[3][n][n_t], component 0 Ix, 1 Iy, 2 Iz of
 * register bit b at output j, of the normalised state; n = the register's qubits (a loopback
 * partitioned register: shard 0's id, whole register; other shard ids DSE_ERR_ARG).
 * DSE_ERR_STATE before an evolve or with the option off, and after any dse_evolve that did not
 * return DSE_OK (every dse_evolve call, failed ones included, ends the previous call's results). */
int dse_get_site_obs(dse_ctx* ctx, int problem, double* out);
/* n_t of the results dse_get_site_obs would return (the size its caller allocates from), 0 when
 * there are none. */
int dse_site_obs_outputs(const dse_ctx* ctx);
/* After dse_evolve with option "pair_obs" = 1: out[5][NP][n_t], the components and pair order of
 * dse_pair_observables at output j (a loopback partitioned register: shard 0's id, whole register;
 * other shard ids DSE_ERR_ARG).  The lifetime rules of dse_get_site_obs: DSE_ERR_STATE before an
 * evolve or with the option off, and after any dse_evolve that did not return DSE_OK. */
int dse_get_pair_obs(dse_ctx* ctx, int problem, double* out);
/* n_t of the results dse_get_pair_obs would return, 0 when there are none. */
int dse_pair_obs_outputs(const dse_ctx* ctx);
/* Registers whose pair sums the last successful dse_evolve produced (a loopback partitioned register
 * counts once), 0 when there are none. */
int dse_pair_obs_problems(const dse_ctx* ctx);
/* ---- overlaps with stored reference states (feature "overlap_obs") ---------------------------
 * A problem may carry K <= DSE_MAX_OVERLAP_REFS reference states phi_0 .. phi_{K-1}.  Every
 * dse_evolve then also keeps, for every output time t_j,
 *     o_k(t_j) = <phi_k|psi(t_j)> / ||psi(t_j)|| = sum_x conj(phi_k(x)) psi_x(t_j) / ||psi(t_j)||
 * with psi(t_j) = exp(-i H (t_j - t_0)) psi(t_0), H including `shift`: o_k carries the true phase (the
 * first observable of the engine that is not invariant under psi -> e^{i theta} psi).  Return
 * amplitudes <psi(t_0)|psi(t)> (whose Fourier transform is the spectrum of the prepared state),
 * fidelities with a target state, populations of chosen many-body states; the reference's
 * counterpart is e_ops = [phi.proj()] of qt.sesolve (:653-666), which gives |o_k|^2 only.
 *   - The references are used as given (not normalised: a caller may pass B psi_0).  They belong to
 *     the problem like the initial state: kept over repeated evolves, replaced as a set, dropped by
 *     dse_clear.  Storage: K device buffers of the state's size per register (per shard of a loopback
 *     register its 2^n_local slice).
 *   - With no references in the context nothing is allocated and no kernel is added; with them the
 *     aggregates and the "site_obs" / "pair_obs" traces are bitwise what they are without, and no
 *     engine choice (engine, lanes, chunks, outputs per launch) reads them.  Registers of one context
 *     may hold different K, 0 included.
 *   - Costs one more read of the state per output plus one read of each reference, and an arena of
 *     2 K_max + 2 doubles per tile and output slot (K_max: the most references a register of the
 *     context holds).
 *   - dse_evolve returns DSE_ERR_ARG for a context that holds both references and a register
 *     partitioned over processes (shard_rank >= 0).
 *
 * refs: [k][2^n] interleaved complex; k = 0 or refs = NULL clears.  DSE_ERR_ARG for a bad id, k above
 * the cap, a non-finite or all-zero reference, a non-zero shard id of a loopback register (shard 0's
 * id and whole 2^n references, as dse_set_initial_state) and a register partitioned over processes;
 * DSE_ERR_OOM leaves the previous set in place. */
int dse_set_overlap_refs(dse_ctx* ctx, int problem, int k, const double* refs);
/* K of the problem (0: none), or DSE_ERR_ARG for a bad id. */
int dse_overlap_refs(const dse_ctx* ctx, int problem);
/* The overlaps of an arbitrary state psi (2^n interleaved complex) with the problem's references:
 * out[2][K], Re block then Im block, divided by ||psi|| (the hook beside dse_site_observables; runs
 * the tile kernel of the evolve; DSE_ERR_STATE for a problem without references). */
int dse_overlaps(dse_ctx* ctx, int problem, const double* psi, double* out);
/* After dse_evolve: out[2][K][n_t], Re block then Im block of o_k(t_j) (a loopback partitioned
 * register: shard 0's id).  The lifetime rules of dse_get_site_obs: DSE_ERR_STATE before an evolve,
 * for a problem without references, and after any dse_evolve that did not return DSE_OK.  After
 * the re-run that follows a hand-off timeout the results are the re-run's (the dense engine's
 * registers keep their first-pass results, like their aggregates). */
int dse_get_overlaps(dse_ctx* ctx, int problem, double* out);
/* n_t of the results dse_get_overlaps would return, 0 when there are none. */
int dse_overlap_outputs(const dse_ctx* ctx);
/* Registers whose overlaps the last successful dse_evolve produced (a loopback partitioned register
 * counts once), 0 when there are none. */
int dse_overlap_problems(const dse_ctx* ctx);
/* ---- expectation values of operator strings (feature "op_strings") ---------------------------
 * A string assigns to every register bit b one spin-1/2 operator O_b out of eight (bit value 0 = up,
 * as everywhere in this header); its value on a state psi is the complex number
 *     v = <psi| prod_b O_b |psi> / <psi|psi>.
 * Multi-spin order <Iz Iz Iz ...>, multiple-quantum coherences (products of I+-), populations of a
 * spin configuration on a subset (products of Ea / Eb), and through the 4^m - 1 strings over
 * {Ix, Iy, Iz} on m spins their full reduced density matrix.  A one-factor string reproduces
 * dse_site_observables, Iz Iz / I+ I- / I+ I+ reproduce dse_pair_observables.
 * A problem may carry K <= DSE_MAX_OP_STRINGS strings; every dse_evolve then also keeps v_k(t_j) for
 * every output time.
 *   - The strings belong to the problem like the overlap references: kept over repeated evolves and
 *     over dse_set_hamiltonian, replaced as a set, dropped by dse_clear.  Storage: one table of 48 K
 *     bytes per register (per shard of a loopback register).
 *   - With no strings in the context nothing is allocated and no kernel is added; with them the
 *     aggregates, the "site_obs" / "pair_obs" / overlap traces and the final state are bitwise what
 *     they are without, and no engine choice reads them.  Registers of one context may hold different
 *     K, 0 included.
 *   - Costs one more read of the state per output, one more per string that flips a bit above the
 *     tile, and an arena of 2 K_max + 2 doubles per tile and output slot.
 *   - dse_evolve returns DSE_ERR_ARG before any work for a context that holds both strings and a
 *     register partitioned over processes (shard_rank >= 0).
 *   - Sums of strings with coefficients are the caller's: add the values on the host. */
enum dse_site_op {
  DSE_OP_1 = 0,  /* identity                      */
  DSE_OP_X = 1,  /* Ix = (I+ + I-) / 2            */
  DSE_OP_Y = 2,  /* Iy = (I+ - I-) / 2i           */
  DSE_OP_Z = 3,  /* Iz = (Ea - Eb) / 2            */
  DSE_OP_P = 4,  /* I+ = |up><down|               */
  DSE_OP_M = 5,  /* I- = |down><up|               */
  DSE_OP_EA = 6, /* Ea = |up><up|                 */
  DSE_OP_EB = 7  /* Eb = |down><down|             */
};
/* ops: [k][n], ops[s * n + b] the dse_site_op code of register bit b in string s; k = 0 or
 * ops = NULL clears.  An all-identity string is legal (its value is 1).  DSE_ERR_ARG for a bad id, k
 * above the cap, a code above 7, a non-zero shard id of a loopback register (shard 0's id, the codes
 * of all n bits) and a register partitioned over processes; a failed allocation leaves the previous
 * set in place. */
int dse_set_op_strings(dse_ctx* ctx, int problem, int k, const uint8_t* ops);
/* K of the problem (0: none), or DSE_ERR_ARG for a bad id. */
int dse_op_strings(const dse_ctx* ctx, int problem);
/* The values of the problem's strings on an arbitrary state psi (2^n interleaved complex): out[2][K],
 * Re block then Im block (the hook beside dse_overlaps; runs the tile kernel of the evolve;
 * DSE_ERR_STATE for a problem without strings). */
int dse_op_string_values(dse_ctx* ctx, int problem, const double* psi, double* out);
/* After dse_evolve: out[2][K][n_t], Re block then Im block of v_k(t_j) (a loopback partitioned
 * register: shard 0's id).  The lifetime rules of dse_get_overlaps: DSE_ERR_STATE before an evolve,
 * for a problem without strings, and after any dse_evolve that did not return DSE_OK.  After the
 * re-run that follows a hand-off timeout the results are the re-run's (the dense engine's registers
 * keep their first-pass results, like their aggregates). */
int dse_get_op_strings(dse_ctx* ctx, int problem, double* out);
/* n_t of the results dse_get_op_strings would return, 0 when there are none. */
int dse_op_string_outputs(const dse_ctx* ctx);
/* Registers whose string values the last successful dse_evolve produced (a loopback partitioned
 * register counts once), 0 when there are none. */
int dse_op_string_problems(const dse_ctx* ctx);
/* Host only: the compiler of one string of n codes (ops[b]: register bit b) into the masks and the
 * prefactor of
 *     <psi| prod_b O_b |psi> = pre * sum_{x : (x & cm) == cv} (-1)^popcount(x & zm) conj(psi_x) psi_{x ^ xm}
 * masks[4] = xm (bits of Ix, Iy, I+, I-: the flips), zm (Iz, Iy: the signs), cm (I+, I-, Ea, Eb: the
 * selected bits), cv (I-, Eb: their required value in x); pre[2] = Re, Im of
 * (1/2)^(#Ix + #Iy + #Iz) (-i)^#Iy.  DSE_ERR_ARG for n outside 1..DSE_MAX_QUBITS, a null pointer or a
 * code above 7. */
int dse_op_string_masks(int n, const uint8_t* ops, uint64_t* masks, double* pre);
/* ---- magnetisation-sector populations (feature "sector_obs") ----------------------------------
 * The distribution of a state over the sectors of a total spin projection.  A sector set is three
 * masks over register bits (bit value 0 = up): m the counted bits, cm the selecting bits, cv their
 * required values; m & cm == 0 and cv & ~cm == 0, m == 0 is allowed.  Its B = popcount(m) + 1 values
 * on a state psi are
 *     P_j = sum_{x : (x & cm) == cv, popcount(x & m) == j} |psi_x|^2 / <psi|psi>,   j = 0 .. popcount(m)
 * (j spins of m down): the full counting statistics of the polarisation of the spins m, whose mean
 * is popcount(m)/2 - sum_b <Iz_b> and whose second moment the Iz Iz correlators give; the norm is the
 * whole state's, so the bins of a set with a selection sum to the selection's probability.  For a pure
 * state the multiple-quantum-coherence intensities follow from them: I_q = sum_M P_M P_{M-q}.
 * A problem may carry K <= DSE_MAX_SECTOR_SETS sets; every dse_evolve then also keeps the U = sum_k B_k
 * values of every output time, the bins of set 0, then set 1, ....
 *   - The sets belong to the problem as the operator strings do: kept over repeated evolves and over
 *     dse_set_hamiltonian, replaced as a set, dropped by dse_clear.  Storage: one table of 32 K bytes
 *     per register (per shard of a loopback register).
 *   - With no sets in the context nothing is allocated and no kernel is added; with them every other
 *     result is bitwise what it is without, and no engine choice reads them.  Registers of one context
 *     may hold different K, 0 included.
 *   - Costs one more read of the state per output and an arena of U_max + 2 doubles per tile and
 *     output slot.  No atomics: two runs give bitwise equal values.
 *   - dse_evolve returns DSE_ERR_ARG before any work for a context that holds both sets and a
 *     register partitioned over processes (shard_rank >= 0). */
/* Host only: validation and layout of k sets on an n-bit register.  masks: [k][3], m, cm, cv of set
 * s at masks[3 s .. 3 s + 2].  Returns U and, with offsets non-null, offsets[s] the first unit of set
 * s and offsets[k] = U.  DSE_ERR_ARG for n outside 1..DSE_MAX_QUBITS, k outside
 * 1..DSE_MAX_SECTOR_SETS, a mask bit at or above n, m & cm != 0, cv & ~cm != 0 and null masks. */
int dse_sector_layout(int n, int k, const uint64_t* masks, int* offsets);
/* masks as above (bits are register bits); k = 0 drops the sets.  DSE_ERR_ARG for a bad id, a
 * non-zero shard id of a loopback register (shard 0's id, masks over all n bits), a register
 * partitioned over processes and whatever dse_sector_layout refuses; a failed allocation leaves the
 * previous sets in place. */
int dse_set_sectors(dse_ctx* ctx, int problem, int k, const uint64_t* masks);
/* K of the problem (0: none), or DSE_ERR_ARG for a bad id. */
int dse_sectors(const dse_ctx* ctx, int problem);
/* U of the problem (0: none), or DSE_ERR_ARG for a bad id. */
int dse_sector_units(const dse_ctx* ctx, int problem);
/* The values of the problem's sets on an arbitrary state psi (2^n interleaved complex): out[U] (the
 * hook beside dse_op_string_values; runs the tile kernel of the evolve; DSE_ERR_STATE for a problem
 * without sets). */
int dse_sector_values(dse_ctx* ctx, int problem, const double* psi, double* out);
/* After dse_evolve: out[U][n_t] (a loopback partitioned register: shard 0's id).  The lifetime rules
 * of dse_get_op_strings: DSE_ERR_STATE before an evolve, for a problem without sets, and after any
 * dse_evolve that did not return DSE_OK.  After the re-run that follows a hand-off timeout the
 * results are the re-run's (the dense engine's registers keep their first-pass results). */
int dse_get_sectors(dse_ctx* ctx, int problem, double* out);
/* n_t of the results dse_get_sectors would return, 0 when there are none. */
int dse_sector_outputs(const dse_ctx* ctx);
/* Registers whose sector populations the last successful dse_evolve produced (a loopback partitioned
 * register counts once), 0 when there are none. */
int dse_sector_problems(const dse_ctx* ctx);
/* Host only: 1 when this library has the named feature, else 0.  Names: "site_obs", "initial_state",
 * "pair_obs", "overlap_obs", "pulse", "set_hamiltonian", "op_strings", "sector_obs", "leap". */
int dse_has_feature(const char* name);
/* Registers the last successful dse_evolve ran on the leap path (option "leap", feature "leap"); they
 * are not counted in dse_stats.real_problems.  0 when there are none. */
int dse_leap_problems(const dse_ctx* ctx);
/* Host only: the leap path's grid rule.  1 and *delta = (t_last - t_0) / (n_t - 1) when
 * max_m |t_m - (t_0 + m delta)| <= 2 ulp(|t_last|) and delta > 0; else 0 and *delta = 0 (one point
 * included); DSE_ERR_ARG for a null t or n_t < 1.  delta may be null. */
int dse_uniform_spacing(const double* t, int n_t, double* delta);
/* Final state of one problem after dse_evolve (2^n interleaved complex). */
int dse_get_state(dse_ctx* ctx, int problem, double* psi_out);
/* ---- initial states other than a basis state (ABI 14.1) --------------------------------------
 * The reference prepares psi0 as a basis ket (:591-606); these entries let an evolution start from
 * any state: a product state after a pulse, the previous segment's final state of a pulse sequence,
 * a random state, a checkpoint.  The initial state belongs to the problem: it persists over
 * repeated dse_evolve calls (each starts from it again at t[0]) and is dropped by dse_clear.  It is
 * not normalised: state_norm reports its norm at every output, the expectations are of the
 * normalised state as everywhere else.
 *   - A stored state (dse_set_initial_state, dse_continue_from_final) lives in ONE extra device
 *     buffer of the state's size per register, allocated only for problems that have one; a
 *     product state keeps its 4 n doubles only.  With no custom initial state in the context
 *     nothing is allocated and no kernel beyond the basis-state path is launched.
 *   - No engine choice reads the initial state: a register runs on the engine it would run on from
 *     its basis state (k_small, the streaming / Walsh-Hadamard / k_interval / k_span / k_real
 *     Chebyshev paths, the dense engine with GEMM or non-uniform-FFT outputs, propagator-matrix
 *     mode, loopback shards), and from the basis state every result is bitwise what it was.  There
 *     are no exceptions.  (The Python host's frozen-rare reduction assumes the basis state; its
 *     helpers for general states build the unreduced register, see simulate_rare_from.)
 *   - The re-run after a hand-off timeout (stats handoff_fallbacks) starts from the same state.
 *   - Loopback partitioned registers (shard_rank = -1): shard 0's id and the whole 2^n state; the
 *     id of another shard is DSE_ERR_ARG.  A register partitioned over processes
 *     (shard_rank >= 0) is not supported: DSE_ERR_ARG.
 *   - Errors: DSE_ERR_ARG for a bad id, a non-finite or all-zero state or amplitude pair;
 *     DSE_ERR_OOM if a buffer cannot be allocated (the problem keeps its previous initial state).
 *
 * psi: 2^n interleaved complex.  The problem's later dse_evolve calls start from it at t[0].
 * NULL: back to the basis state psi0_index (the extra buffer is released). */
int dse_set_initial_state(dse_ctx* ctx, int problem, const double* psi);
/* Product state: amp[4 b + (0..3)] = (re a_b0, im a_b0, re a_b1, im a_b1);
 * psi(x) = prod_b a_b[bit_b(x)], built on the device by k_product_state at every dse_evolve
 * (nothing state-sized crosses the host; a shard writes its global indices (shard << n_local) | x). */
int dse_set_initial_product(dse_ctx* ctx, int problem, const double* amp /* [4n] */);
/* The final state of the last dse_evolve, which must have returned DSE_OK, becomes this problem's
 * initial state (device-to-device copy; DSE_ERR_STATE without such an evolve, or after a hook
 * call that used the state buffers).  Continuation of a run over t[k..], checkpoints. */
int dse_continue_from_final(dse_ctx* ctx, int problem);
/* The state the next dse_evolve would start from (the basis state, the stored state, or the
 * product state materialised by its kernel): test and diagnostic hook. */
int dse_get_initial_state(dse_ctx* ctx, int problem, double* psi_out);

/* ---- hard pulses and piecewise-constant H (features "pulse", "set_hamiltonian") -----------------
 * An instantaneous rotation of chosen spins between two periods of evolution (Hahn echo, CPMG, a
 * z-phase increment, a read-out pulse), and a new H for a problem that keeps its state: together a
 * pulse sequence whose state never leaves the device.  No reference counterpart (the reference has
 * one time-independent H per call).
 *
 * dse_apply_pulse transforms the state the next dse_evolve starts from by U = (x)_b U_b:
 *   u[8 b + ...] = (re u00, im u00, re u01, im u01, re u10, im u10, re u11, im u11) of register bit b,
 *   row / column index = bit value (0 = spin up): psi'(.., v, ..) = sum_w u_vw psi(.., w, ..).
 *   - A stored state (dse_set_initial_state, dse_continue_from_final): k_pulse (dse_pulse.hip) runs in
 *     place on it, one launch per pass of dse_pulse_plan; nothing state-sized is allocated or crosses
 *     the host.  A loopback partitioned register: shard 0's id, all shards transformed.
 *   - A product state stays one: a_b <- U_b a_b on the host, the 4 n doubles uploaded again.
 *   - The basis state psi0_index becomes the product state whose pair for bit b is column
 *     bit_b(psi0_index) of U_b.  The identity (every U_b exactly 1) changes nothing, whatever the start.
 *   - The matrices are used as given: unitarity is not checked (2 Ix_b is a legal factor).
 *   - DSE_ERR_ARG, the state left as it was: a non-finite entry, a matrix that is all zero, on the two
 *     host paths a resulting zero or non-finite amplitude pair, a bad id, a non-zero shard id of a
 *     loopback register, a register partitioned over processes.  A stored state that a singular pulse
 *     maps to zero is NOT detected: the next dse_evolve then reports state_norm 0 and undefined
 *     expectations.
 *   - A pulse before any dse_evolve and on a problem without a custom state is accepted.  The final
 *     state of the last evolve (dse_get_state) is not touched. */
int dse_apply_pulse(dse_ctx* ctx, int problem, const double* u /* [8 n] */);
/* out[0] = passes (kernel launches), out[1] = their HIP-event time in ms, out[2] = the bytes they
 * moved (32 per amplitude and pass) of the last dse_apply_pulse of the context; zeros for the host
 * paths, the identity and a refused call. */
int dse_pulse_stats(const dse_ctx* ctx, double* out /* [3] */);
/* Host only, like dse_wht_plan: the passes of a pulse on a register of n_local local and shard_bits
 * (0..3) shard bits (register bit n_local + s = shard bit s).  active_mask: the bits whose matrix is not
 * the identity; diag_mask: those of them whose matrix is diagonal (a subset, DSE_ERR_ARG otherwise).
 * Returns the number of passes G (0: the identity) and writes, for g < G,
 *   groups_out[g][0]      the carried low bits c (0: group 0, the low 12 bits)
 *   groups_out[g][1 + q]  the register bit of tile bit q < 12 (-1: none, registers below 12 bits)
 *   groups_out[g][13]     the mask of tile bits q the pass transforms (0: a pass for diagonal
 *                         matrices only).
 * The first pass also applies every diagonal matrix's phase. */
int dse_pulse_plan(int n_local, int shard_bits, uint64_t active_mask, uint64_t diag_mask,
                   int32_t* groups_out /* [4][14] */);
/* Replaces the tables of a problem (arrays as in dse_add_problem, validated the same way; on failure
 * the old H stays): the spectral bounds and the flop count follow, on every shard of a loopback
 * register (shard 0's id).  Kept: n, psi0_index, the masks, the shard layout, the initial state, the
 * overlap references, the options.  The device layout is dropped and rebuilt by the next dse_evolve,
 * which is bitwise what a fresh context with the new tables and the same initial state gives; the
 * previous final state goes with it (dse_get_state and dse_continue_from_final return DSE_ERR_STATE
 * until the next evolve: continue first, then change H).  Not available for a register partitioned
 * over processes (DSE_ERR_ARG). */
int dse_set_hamiltonian(dse_ctx* ctx, int problem, const double* field, const double* zz,
                        const double* pair, const double* flip, double shift);

/* Energy of the final state after dse_evolve, on the device: e_out[0] = <psi|H|psi> / <psi|psi>,
 * e_out[1] = <psi|psi> (a partitioned loopback register: shard 0's id, whole register).  Unitary
 * evolution conserves both exactly, so they check a run whose state is too large to compare
 * (the reference has no counterpart; its only diagnostic is state_norm, :669).  Not available
 * for a dist shard (DSE_ERR_ARG). */
int dse_energy(dse_ctx* ctx, int problem, double* e_out /* [2] */);
/* Times the Chebyshev step kernel alone: reps launches over all problems, HIP events around
 * each launch.  Returns the mean launch duration and the algorithmic bytes per launch. */
int dse_time_step_kernel(dse_ctx* ctx, int reps, double* ms_per_launch, double* bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* DSE_H */
