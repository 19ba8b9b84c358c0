"""k_real (csrc/dse_real.hip real_body<13> and real_body<14>, k_real_combine, k_real_init; dse_init.hip
k_real_split; dse_runtime.hip build_real_table, choose_real) on both register sizes, every
table class and series edge, against a CPU propagation of the same raw-table pb.Problem.

tests/test_gpu_real.py holds k_real to k_interval on the bench's registers; here every case is held to
scipy expm_multiply.  Every case sets real, span_tile = 0, span = 0, matrix = 0, dense = 0, tile_bits =
13 and the schedule options it depends on (_context, restored from RESTORE), and asserts mode 1,
real_problems equal to the expected count, span_problems = dense_problems = 0, handoff_fallbacks = 0,
outputs_per_launch and max_degree equal to the host prediction (tests/test_interval_cases_host.py).

A register of n = 13 or 14 qubits has 9 thread bits b < 9 and n - 9 register bits, the top one (bit n - 1)
splitting a thread's rows into halves (tests/test_real_cases_host.py: the registers, the Python
restatement of build_real_table, the class patterns).

1. size x start: the full imaginary-drive registers of n = 14 and 13 (every coupling and drive non-zero
   and distinct, rare_bit = n - 1) on the uneven grid T6 (at M = 2 launches of 2, 2, 1 outputs) from
   basis states of popcount 0, 1, 2, 3 (mod 4), |0..0> and |1..1> among them: the four branches of the
   combine's phase i^{|x0| - |x|} and k_real_init's index.  8 cases.
2. table classes at n = 14 and 13, from the full register by zeroing entries (class_problem; every case
   asserts pattern(real_table(p)) == class_table first).  The pair classes keep every drive and one kind
   of pair, the drive classes keep every pair:
     thread_pairs_only     pairs among bits < 9: ge[], real_pair_mask
     thread_reg_low_only   pairs (thread bit, register bit below the top): gsel
     thread_top_only       pairs (thread bit, top register bit): the oo other-half update
     reg_low_only          pairs among register bits below the top: own_half's rr_g loop
     reg_top_only          pairs (a, top): cross_half
     drive_top_only        drive on the top register bit only: cross_half's rflip[TOP]
     drive_reg_partial     drives on register bits 0 and 2 only: partial rflip_mask
     drive_threads_sparse  drives on thread bits 0, 3, 8, the thread pairs of bit 1 zeroed: zeros in S.it
     no_drives             flip = 0: rflip_mask = 0
     diagonal              no pairs, no drives, full field and zz, from a general complex psi0: td, zr,
                           shift - beta
     residue               re = 6e-17 |im|: dropped by the 1e-15 rule, still on k_real; the reference
                           propagates the tables as given
   22 cases.
3. series edges on the section-1 registers at outputs_per_launch 1 and 2, on the 8-point grid T8R chosen
   on the CPU (series_edges) so that the last update of output 0 and of output 1 carries 3, 1 and 2 terms
   in some launch, output 0 ends below the launch's K while output 1 still updates (phase5<2> with zero
   coefficients), and the last launch has one output (phase5<1>); and a coarse grid (alpha dt = 420 and
   462, degree > 400, M = 1 chosen by the runtime) on the n = 13 register.
4. initial states and continuation: a general complex psi0 and a product state at n = 14 and 13
   (k_real_split, x0pop = 0, custom_init_problems asserted); continue_from_final over the second half of
   T6 against the one-evolve run (1e-11) and the reference; three evolves of one context bitwise equal.
5. contexts and policy: five registers, n = 13 and 14 mixed, of unequal degree under real = 1, each against
   its reference and bitwise equal to the same register alone; the same context under real = 2
   (real_problems = the three 14-qubit registers; mode 1 with span_problems = dense_problems = 0 leaves
   the two 13-qubit ones on k_interval) against the reference and within 1e-11 of real = 0;
   choose_real's fall-backs (a complex-drive register, an n = 12 register, the above_residue register
   re = 1e-14 |im| in the context, obs_overlap = 1): real_problems = 0 and every register against its
   reference; one n = 14 register with site_obs, pair_obs and stored-reference overlaps on, against the
   references of test_gpu_site_obs.py, test_gpu_pair_obs.py and test_gpu_overlap_obs.py (1e-10).

Reference: scipy expm_multiply on problem_to_csr(prob), stepped output to output from the case's initial
state (test_gpu_site_obs.expm_states, test_gpu_initial_state.expm_from), oracle.reference_model.
observables_bitwise of every state; once per problem, start and grid.  Bounds are the project's
(test_gpu_interval_cases.py): 1e-10 for the seven observables at every output and for the final state,
1e-12 for the norm, 1e-11 between two exact propagators of the engine, bitwise equality where the same
kernel runs the same data.

Measured (MI355X; max over the observables at every output and the final state, per section's worst row):
  section 1   3.6e-15 (n = 14, x0 = 0); every row between 2.3e-15 and 3.6e-15
  section 2   drive_reg_partial 1.3e-14, drive_threads_sparse 9.3e-15, no_drives 8.0e-15, drive_top_only 6.3e-15,
              thread_reg_low_only 4.6e-15, reg_top_only 4.1e-15, residue 4.0e-15, reg_low_only 3.3e-15,
              thread_top_only 2.0e-15, thread_pairs_only 1.1e-15, diagonal 7.8e-16
  section 3   T8R m = 1 6.0e-15, m = 2 3.9e-15; coarse grid 2.5e-14
  section 4   general psi0 7.2e-16, product psi0 3.6e-15, continuation 2.9e-15; the continuation against the
              one-evolve run and the repeats: bitwise equal (0.0)
  section 5   mixed sizes 4.5e-15 under real = 1 and real = 2; each register in the context and alone, and the
              13-qubit registers under real = 2 and real = 0: bitwise equal; real = 2 against real = 0 4.4e-16;
              fall-backs 5.5e-15 (n = 12), 2.9e-15 (the others); site 8.9e-16, pair 2.2e-16, overlap 3.8e-16
No case found an error in k_real, k_real_combine, k_real_init, k_real_split, build_real_table or choose_real.

Sensitivity, with one-line changes of dse_real.hip in scratch builds (49 cases; coefficients and in-range data
indices only, never a barrier or a bound).  The drive classes and every other case on a full register hold
every kind of pair, so they fail with the pair classes named; the four fall-backs run on k_interval and pass
every time:
  gsel's bit test inverted                              37 fail: thread_reg_low_only, thread_top_only and every
        case that holds all pairs; thread_pairs_only, reg_low_only, reg_top_only, diagonal pass
  cross_half's (a, top) row test inverted               35 fail: reg_top_only and every case that holds all pairs;
        thread_pairs_only, thread_reg_low_only, thread_top_only, reg_low_only, diagonal pass.  (The change the
        kernel's rflip[TOP][hh] invites, [1 - hh], is invisible to any Hermitian problem: the rotated drive's
        two rows are equal, i^-1 (i a) = i (-i a) (test_real_cases_host.test_full_table), so the pair's row
        test stands in for it.)
  the oo update written to the same half                35 fail: thread_top_only and every case that holds all
        pairs; thread_pairs_only, thread_reg_low_only, reg_low_only, reg_top_only, diagonal pass
  1 + 1e-6 on ge[] in real_body<14> alone               19 fail, 1e-7: exactly the n = 14 cases with thread pairs
        (section 1's four, thread_pairs_only, the four drive classes and residue at n = 14, both series-edge
        cases, both custom starts, continuation, repeat, both mixed contexts, the observable families);
        every n = 13 case, the coarse grid and the n = 14 classes without thread pairs pass
  c[0] zero when an update carries three terms          45 fail: every case on k_real, diagonal and the series
        edges among them
so each pair class isolates the code path it names, and the register size selects the instantiation.
"""
import numpy as np
import pytest

from oracle import reference_model as rm
from test_gpu_initial_state import expm_from, kron_state
from test_gpu_overlap_obs import make_refs, ov_ref
from test_gpu_pair_obs import pair_ref_traces
from test_gpu_site_obs import expm_states, site_ref_traces
from test_interval_cases_host import T6, chosen_m, predicted_degrees, predicted_max_degree
from test_real_cases_host import (CASES1, CASES2, SIZES, T8R, class_problem, class_table, coarse_problem,
                                  fallback_problems, general_state, mixed_problems, pattern, problem1, product_amps,
                                  real_table, series_edges)

pytestmark = pytest.mark.gpu

BOUND = 1e-10
NORM_BOUND = 1e-12
ENGINE_BOUND = 1e-11   # two exact propagators of the engine
RESTORE = {"span_tile": -1, "span": 0, "real": 0, "matrix": 1, "dense": 1, "tile_bits": 13, "outputs_per_launch": 2,
           "obs_overlap": 0, "site_obs": 0, "pair_obs": 0}
SCHEDULE_OPTS = ("outputs_per_launch", "obs_overlap", "site_obs", "pair_obs")
assert len(CASES1) == 8 and len(CASES2) == 22


# ------------------------------------------------------------------------------ references
_REF = {}


def reference(key, p, t, psi0=None):
    """(states on t, their seven observables (7, n_t)) by expm_multiply from the register's basis state or
    from psi0, once per (problem, start, grid)."""
    k = (key, tuple(t.tolist()))
    if k not in _REF:
        if psi0 is None:
            states = expm_states(("real_cases",) + tuple(key), p, t)
        else:
            states = expm_from(("real_cases",) + tuple(key), p, t, psi0)
        obs = np.stack([rm.observables_bitwise(s, p.n_qubits, p.sea_mask, p.rare_bit) for s in states], axis=1)
        _REF[k] = (states, obs)
    return _REF[k]


# ------------------------------------------------------------------------------ plumbing
class _context:
    """The registers probs in the cleared session engine with option real: every option the cases depend
    on set on entry and restored on exit.  inits[i]: None, a ket, or ("product", amps)."""

    def __init__(self, engine, probs, real=1, inits=None, **opts):
        assert set(opts) <= set(SCHEDULE_OPTS), opts
        self.engine, self.probs, self.inits = engine, probs, inits
        self.opts = {"real": real, "span_tile": 0, "span": 0, "matrix": 0, "dense": 0, "tile_bits": 13}
        self.opts.update({k: RESTORE[k] for k in SCHEDULE_OPTS})
        self.opts.update(opts)

    def __enter__(self):
        self.engine.clear()
        try:
            for k, v in self.opts.items():
                self.engine.set_option(k, v)
            self.pids = [self.engine.add(p) for p in self.probs]
            for pid, init in zip(self.pids, self.inits or []):
                if isinstance(init, tuple):
                    self.engine.set_initial_product(pid, init[1])
                elif init is not None:
                    self.engine.set_initial_state(pid, init)
        except Exception:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in RESTORE.items():
            self.engine.set_option(k, v)
        self.engine.clear()

    def evolve(self, t):
        """obs (n_reg, 7, n_t), stats, final states."""
        obs, st = self.engine.evolve(t)
        return obs[self.pids], st, [self.engine.state(pid) for pid in self.pids]


def _evolve(engine, probs, t, real=1, inits=None, **opts):
    with _context(engine, probs, real, inits, **opts) as c:
        return c.evolve(t)


def _assert_ran(st, probs, t, m, n_real, n_custom=0):
    """The evolve ran on the persistent kernels alone, n_real registers on k_real, with the series the
    case means."""
    assert st["mode"] == 1, st["mode"]
    assert st["real_problems"] == n_real, (st["real_problems"], n_real)
    assert st["span_problems"] == 0 and st["dense_problems"] == 0, st
    assert st["handoff_fallbacks"] == 0
    assert st["custom_init_problems"] == n_custom, (st["custom_init_problems"], n_custom)
    M = chosen_m(probs, t, m)
    assert st["outputs_per_launch"] == M, (st["outputs_per_launch"], M)
    assert st["max_degree"] == predicted_max_degree(probs, t, M), (st["max_degree"], predicted_max_degree(probs, t, M))


_WORST = {}   # (section, row) -> max error seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nmax |k_real - expm_multiply| (observables at every output, final state):")
        for (sec, row), e in sorted(_WORST.items()):
            print(f"  section {sec} {row}: {e:.2e}")
        for sec in sorted({k[0] for k in _WORST}):
            print(f"  section {sec} worst: {max(e for k, e in _WORST.items() if k[0] == sec):.2e}")


def _note(sec, row, e):
    _WORST[sec, row] = max(_WORST.get((sec, row), 0.0), e)


def _check(sec, row, label, obs, final, ref):
    states, ref_obs = ref
    assert obs.shape == ref_obs.shape
    assert np.all(np.isfinite(obs)) and np.all(np.isfinite(final.view(float)))
    e_obs = float(np.max(np.abs(obs - ref_obs)))
    e_fin = float(np.max(np.abs(final - states[-1])))
    e_norm = float(np.max(np.abs(obs[6] - 1.0)))
    print(f"{label}: observables {e_obs:.2e}, final state {e_fin:.2e} (bound {BOUND:g}), norm {e_norm:.2e} "
          f"(bound {NORM_BOUND:g})")
    _note(sec, row, max(e_obs, e_fin))
    assert e_obs < BOUND, (label, e_obs)
    assert e_fin < BOUND, (label, e_fin)
    assert e_norm < NORM_BOUND, (label, e_norm)


def _bitwise(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _same_bits(label, run, base):
    """Observables and final states of every register identical to the base run's."""
    (obs, _, finals), (obs0, _, finals0) = run, base
    d = max(float(np.max(np.abs(obs - obs0))), max(float(np.max(np.abs(a - b))) for a, b in zip(finals, finals0)))
    print(f"{label}: max difference from the base run {d:.2e} (bitwise equal required)")
    assert np.array_equal(obs, obs0), (label, d)
    assert _bitwise(finals, finals0), (label, d)


def _close(sec, row, label, run, base):
    """Two exact propagators of the engine: observables and final states within ENGINE_BOUND."""
    (obs, _, finals), (obs0, _, finals0) = run, base
    d = max(float(np.max(np.abs(obs - obs0))), max(float(np.max(np.abs(a - b))) for a, b in zip(finals, finals0)))
    print(f"{label}: max difference {d:.2e} (bound {ENGINE_BOUND:g})")
    _note(sec, row, d)
    assert d < ENGINE_BOUND, (label, d)


# ------------------------------------------------------------------------------ 1. size x start
@pytest.mark.parametrize("n,x0", CASES1)
def test_size_and_start(engine, n, x0):
    p, key = problem1(n, x0)
    T = real_table(p)
    assert T["x0"] == x0 and T["x0pop"] % 4 == bin(x0).count("1") % 4
    obs, st, finals = _evolve(engine, [p], T6)
    _assert_ran(st, [p], T6, 2, 1)
    _check(1, f"n = {n} |x0| = {T['x0pop']}", f"real_body<{n}> x0 = {x0:#x} (popcount {T['x0pop']})", obs[0], finals[0],
           reference(key, p, T6))


# ------------------------------------------------------------------------------ 2. table classes
@pytest.mark.parametrize("cls,n", CASES2)
def test_table_classes(engine, cls, n):
    p, key = class_problem(cls, n)
    assert pattern(real_table(p)) == class_table(cls, n)
    psi0 = general_state(n, 8200 + n) if cls == "diagonal" else None
    obs, st, finals = _evolve(engine, [p], T6, inits=None if psi0 is None else [psi0])
    _assert_ran(st, [p], T6, 2, 1, n_custom=0 if psi0 is None else 1)
    _check(2, cls, f"real_body<{n}> {cls}", obs[0], finals[0], reference(key, p, T6, psi0))


# ------------------------------------------------------------------------------ 3. series edges
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_series_edges(engine, n, m):
    p, key = problem1(n)
    groups, K = series_edges(p, T8R)   # conditions on the inputs, from the host prediction
    obs, st, finals = _evolve(engine, [p], T8R, outputs_per_launch=m)
    _assert_ran(st, [p], T8R, m, 1)
    assert st["outputs_per_launch"] == m and st["max_degree"] == predicted_degrees(p, T8R, m)[1]
    print(f"n = {n}: degrees per launch at M = 2 {groups}, K = {K}")
    _check(3, f"T8R m = {m}", f"real_body<{n}> outputs_per_launch = {m}", obs[0], finals[0], reference(key, p, T8R))


def test_coarse_grid(engine):
    p, key, t = coarse_problem()
    obs, st, finals = _evolve(engine, [p], t, outputs_per_launch=2)
    _assert_ran(st, [p], t, 2, 1)
    assert st["outputs_per_launch"] == 1 and st["max_degree"] > 400, st
    print(f"coarse grid: degree {st['max_degree']}")
    _check(3, "coarse", "real_body<13>, alpha dt >= 400", obs[0], finals[0], reference(key, p, t))


# ------------------------------------------------------------------------------ 4. initial states, continuation
@pytest.mark.parametrize("kind", ["general", "product"])
@pytest.mark.parametrize("n", SIZES)
def test_custom_initial_states(engine, n, kind):
    p, key = problem1(n)
    if kind == "general":
        psi0 = init = general_state(n, 8300 + n)
    else:
        amps = product_amps(n, 8400 + n)
        psi0, init = kron_state(amps), ("product", amps)
    assert abs(np.linalg.norm(psi0) - 1.0) < 1e-14 and np.count_nonzero(psi0) == 1 << n
    obs, st, finals = _evolve(engine, [p], T6, inits=[init])
    _assert_ran(st, [p], T6, 2, 1, n_custom=1)
    _check(4, f"{kind} psi0", f"real_body<{n}> from a {kind} state (k_real_split)", obs[0], finals[0],
           reference(key + (kind,), p, T6, psi0))


@pytest.mark.parametrize("n", SIZES)
def test_continuation(engine, n):
    p, key = problem1(n)
    h = 2
    with _context(engine, [p]) as c:
        whole = c.evolve(T6)
        first = c.evolve(T6[:h + 1])
        engine.continue_from_final(c.pids[0])
        second = c.evolve(T6[h:])
    _assert_ran(whole[1], [p], T6, 2, 1)
    _assert_ran(first[1], [p], T6[:h + 1], 2, 1)
    _assert_ran(second[1], [p], T6[h:], 2, 1, n_custom=1)
    ref = reference(key, p, T6)
    _check(4, "continuation", f"n = {n}, one evolve over T6", whole[0][0], whole[2][0], ref)
    _check(4, "continuation", f"n = {n}, second half from the first half's final state", second[0][0], second[2][0],
           (ref[0][h:], ref[1][:, h:]))
    _close(4, "continuation against one evolve", f"n = {n}: two evolves against one",
           (second[0], None, second[2]), (whole[0][:, :, h:], None, whole[2]))


def test_repeated_evolves_are_bitwise_equal(engine):
    p, key = problem1(14)
    with _context(engine, [p]) as c:
        runs = [c.evolve(T6) for _ in range(3)]
    for r in runs:
        _assert_ran(r[1], [p], T6, 2, 1)
    _check(4, "repeat", "n = 14, first of three evolves", runs[0][0][0], runs[0][2][0], reference(key, p, T6))
    for i in (1, 2):
        _same_bits(f"evolve {i + 1} of 3", runs[i], runs[0])


# ------------------------------------------------------------------------------ 5. contexts and policy
def test_mixed_sizes_real_1(engine):
    probs, keys = mixed_problems()
    run = _evolve(engine, probs, T6)
    _assert_ran(run[1], probs, T6, 2, 5)
    for i, (p, key) in enumerate(zip(probs, keys)):
        _check(5, "n = 13 and 14 mixed, real = 1", f"register {i}: n = {p.n_qubits}", run[0][i], run[2][i],
               reference(key, p, T6))
        alone = _evolve(engine, [p], T6)
        assert alone[1]["real_problems"] == 1 and alone[1]["mode"] == 1
        _same_bits(f"register {i} alone", (run[0][i:i + 1], None, run[2][i:i + 1]), alone)


def test_mixed_sizes_real_2(engine):
    probs, keys = mixed_problems()
    n14 = sum(1 for p in probs if p.n_qubits == 14)
    assert 0 < n14 < len(probs)
    run = _evolve(engine, probs, T6, real=2)
    # mode 1 without span or dense registers: the registers not counted in real_problems ran on k_interval
    _assert_ran(run[1], probs, T6, 2, n14)
    for i, (p, key) in enumerate(zip(probs, keys)):
        _check(5, "n = 13 and 14 mixed, real = 2", f"register {i}: n = {p.n_qubits}", run[0][i], run[2][i],
               reference(key, p, T6))
    base = _evolve(engine, probs, T6, real=0)
    _assert_ran(base[1], probs, T6, 2, 0)
    _close(5, "real = 2 against real = 0", "real = 2 against real = 0", run, base)
    # the 13-qubit registers run the same kernel on the same data in both
    i13 = [i for i, p in enumerate(probs) if p.n_qubits == 13]
    _same_bits("13-qubit registers, real = 2 against real = 0", (run[0][i13], None, [run[2][i] for i in i13]),
               (base[0][i13], None, [base[2][i] for i in i13]))


@pytest.mark.parametrize("kind", ["complex", "n12", "above_residue", "obs_overlap"])
def test_fallbacks(engine, kind):
    """choose_real with real = 1 and a context that does not qualify: every register on k_interval."""
    if kind == "obs_overlap":
        (a, ka), (b, kb) = problem1(14), problem1(13)
        probs, keys, opts = [a, b], [ka, kb], {"obs_overlap": 1}
    else:
        probs, keys = fallback_problems(kind)
        opts = {}
    obs, st, finals = _evolve(engine, probs, T6, **opts)
    _assert_ran(st, probs, T6, 2, 0)
    for i, (p, key) in enumerate(zip(probs, keys)):
        _check(5, f"fall-back: {kind}", f"{kind} register {i}: n = {p.n_qubits}", obs[i], finals[i], reference(key, p, T6))


def test_site_pair_and_overlap_observables(engine):
    """The families that read the buffers k_real_combine writes (intermediate outputs and the state buffer)."""
    p, key = problem1(14)
    refs = make_refs(14, 8514, 3)
    with _context(engine, [p], site_obs=1, pair_obs=1) as c:
        engine.set_overlap_refs(c.pids[0], refs)
        obs, st, finals = c.evolve(T6)
        sites, pairs, ov = engine.site_traces(c.pids[0]), engine.pair_traces(c.pids[0]), engine.overlap_traces(c.pids[0])
        assert engine.overlap_problems() == 1 and engine.pair_obs_problems() == 1 and st["site_obs_problems"] == 1
    _assert_ran(st, [p], T6, 2, 1)
    ref = reference(key, p, T6)
    _check(5, "site, pair, overlap on", "n = 14 with the three families on", obs[0], finals[0], ref)
    for name, got, want in (("site", sites, site_ref_traces(ref[0], 14)), ("pair", pairs, pair_ref_traces(ref[0], 14)),
                            ("overlap", ov, ov_ref(refs, ref[0]))):
        assert got.shape == want.shape
        e = float(np.max(np.abs(got - want)))
        print(f"{name} traces: max |k_real - reference| = {e:.2e} (bound {BOUND:g})")
        _note(5, f"{name} traces", e)
        assert e < BOUND, (name, e)
