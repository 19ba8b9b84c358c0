"""The leap path (csrc/dse_real.hip k_leap_combine, k_leap_init, real_body on p_m alone; dse_runtime.hip
choose_leap, uniform_spacing; option "leap", dse_leap_problems): on a uniform output grid, from
basis states, one real Chebyshev recurrence per register and launch, the outputs by the time recurrence
(tests/test_leap_host.py states the arithmetic).

Every case sets leap and the options it depends on (_context, restored from RESTORE).  The registers are
tests/test_real_cases_host.py's: the full imaginary-drive registers of n = 13 and 14 (every coupling and drive
non-zero and distinct) from basis states of popcount 0, 1, 2, 3 (mod 4).  Grid: T22 = 3e-4 + 5e-5 m, m < 22
(t_0 != 0) and its prefixes (T10: the first ten points), so one expm_multiply reference per register serves
every grid length.

1. size x start x grid length with leap_fan 1 and 2: 1, 2, 3, 4, 5, 7, 8, 9 intervals (the first launch alone,
   every tail at one, two and four outputs per launch) and 17 to 21 intervals (the history ring has eight
   entries, output m in entry m mod 8: from output 9 on every launch reads entries that wrapped, up to 11
   launches at fan 1 and 6 at fan 2, again with every tail); a grid from t_0 = 0; and the bench's whole grid
   (101 outputs, 50 and 25 launches) on the bench's registers at three detunings against the reference-H
   traces of tests/test_gpu_config3_bench.py at its bounds.  The rest: against scipy expm_multiply stepped output to output, seven observables at every output
   and the final state within 1e-10, the norm within 1e-12 (test_gpu_real_cases.py's bounds), and within 1e-11
   of leap = 0 (k_interval).  leap_problems, real_problems = 0, max_degree and h_applications equal the host
   prediction (test_leap_host.leap_prediction), handoff_fallbacks = 0.
2. fall-backs, each with leap_problems = 0 and results bitwise equal to leap = 0: a non-uniform grid, a
   product and a custom state, continue_from_final after a leap evolve (its start is the complex final state,
   bitwise dse_get_state's), a general-phase drive, an n = 12 register in the context, obs_overlap = 1, alpha
   delta >= 400, outputs_per_launch = 1; and the automatic rule (leap = -1 with the automatic span policy's forms off, span_chunks = 0
   and span_partial = 0, so that two registers reach it): taken, and not taken with span_tile = 0, with real =
   1 (k_real keeps its registers) and with spin_limit off its default.
3. three evolves of one context bitwise equal; five registers of both sizes and unequal degree in one context,
   each bitwise equal to the register alone; leap_fan 1 and 2.
4. site, pair, overlap, string and sector observables (they read the buffers k_leap_combine writes) within
   1e-11 of leap = 0; leap_fan 1 and 2.

Measured (MI355X), worst over each section: against expm_multiply 3.0e-14, norm 2.1e-14, against leap = 0
1.1e-13 (grids up to 21 intervals); the bench grid 1.5e-12 against the reference-H traces at either fan-out,
norm 4.1e-13 (leap_fan 1, 50 launches) and 1.8e-13 (leap_fan 2, 25 launches); mixed context 7.5e-15; families
4.6e-15 (aggregate), 2.3e-15 (sector), below 6e-16 (site, pair, overlap, string).  Before the series were cut at
tol / launches (build_coefficients) the bench's 192 registers reached 9.3e-12 of norm at output 99.

Sensitivity: the four one-line errors the path invites (the sign of the odd sum, the factor 2, a history index
off by one, the m = 0 form used at m0 > 0) are checked on the numpy restatement of the same arithmetic,
test_leap_host.test_one_line_errors_miss_the_bound, where each misses the state bound by eight orders or more.
They were not run as scratch builds of k_leap_combine on the device.  Every section-1 grid of more than one
launch reads the history (and from 9 outputs on, wrapped entries), at bounds five orders below such an error.
"""
import numpy as np
import pytest

from oracle import reference_model as rm
from test_gpu_site_obs import expm_states
from test_interval_cases_host import T6, half_width
from test_leap_host import leap_prediction
from test_real_cases_host import CASES1, fallback_problems, general_state, mixed_problems, problem1, product_amps

pytestmark = pytest.mark.gpu

BOUND = 1e-10
NORM_BOUND = 1e-12
ENGINE_BOUND = 1e-11
DT = 5e-5
T22 = 3e-4 + DT * np.arange(22)
T10 = T22[:10]
INTERVALS = (1, 2, 3, 4, 5, 7, 8, 9, 17, 18, 19, 20, 21)
LEAP_FAN_DEFAULT = 2
RESTORE = {"leap": -1, "leap_fan": LEAP_FAN_DEFAULT, "span_tile": -1, "span": 0, "real": 0, "matrix": 1, "dense": 1, "tile_bits": 13,
           "outputs_per_launch": 2, "obs_overlap": 0, "site_obs": 0, "pair_obs": 0, "span_chunks": 2, "span_partial": 1,
           "spin_limit": 1 << 22}
CASE_OPTS = ("outputs_per_launch", "obs_overlap", "site_obs", "pair_obs", "span_tile", "span_chunks", "span_partial",
             "spin_limit", "real", "leap_fan")


class _context:
    """The registers probs in the cleared session engine with option leap; whole registers (span_tile = 0)
    unless the case says otherwise."""

    def __init__(self, engine, probs, leap, inits=None, **opts):
        assert set(opts) <= set(CASE_OPTS), opts
        self.engine, self.probs, self.inits = engine, probs, inits
        self.opts = {"leap": leap, "span_tile": 0, "span": 0, "real": 0, "matrix": 0, "dense": 0, "tile_bits": 13}
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
        obs, st = self.engine.evolve(t)
        return obs[self.pids], st, [self.engine.state(pid) for pid in self.pids]


def _evolve(engine, probs, t, leap, inits=None, **opts):
    with _context(engine, probs, leap, inits, **opts) as c:
        return c.evolve(t)


_REF = {}


def reference(key, p):
    """(states on T22, their seven observables (7, 22)) by expm_multiply, once per register and start."""
    if key not in _REF:
        states = expm_states(("leap",) + tuple(key), p, T22)
        _REF[key] = (states, np.stack([rm.observables_bitwise(s, p.n_qubits, p.sea_mask, p.rare_bit) for s in states], axis=1))
    return _REF[key]


_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, e in sorted(_WORST.items()):
        print(f"  worst {k}: {e:.2e}")


def _note(k, e):
    _WORST[k] = max(_WORST.get(k, 0.0), e)


def _diff(run, base):
    (obs, _, finals), (obs0, _, finals0) = run, base
    return max(float(np.max(np.abs(obs - obs0))), max(float(np.max(np.abs(a - b))) for a, b in zip(finals, finals0)))


def _same_bits(label, run, base):
    d = _diff(run, base)
    print(f"{label}: max difference {d:.2e} (bitwise equal required)")
    assert np.array_equal(run[0], base[0]), (label, d)
    assert all(np.array_equal(a, b) for a, b in zip(run[2], base[2])), (label, d)


def _assert_leapt(st, probs, t, m=2, fan=LEAP_FAN_DEFAULT):
    M, deg, happl = leap_prediction(probs, t, m, fan)
    assert st["mode"] == 1 and st["leap_problems"] == len(probs) and st["real_problems"] == 0, st
    assert st["span_problems"] == 0 and st["dense_problems"] == 0 and st["handoff_fallbacks"] == 0, st
    assert st["outputs_per_launch"] == M and st["max_degree"] == deg and st["h_applications"] == happl, (st, M, deg, happl)


# ------------------------------------------------------------------------------ 1. size x start x grid
@pytest.mark.parametrize("m,fan", [(2, 1), (2, 2)])
@pytest.mark.parametrize("n,x0", CASES1)
def test_size_start_and_grid(engine, n, x0, m, fan):
    p, key = problem1(n, x0)
    states, ref_obs = reference(key, p)
    for ni in INTERVALS:
        t = T22[:ni + 1]
        run = _evolve(engine, [p], t, 1, outputs_per_launch=m, leap_fan=fan)
        base = _evolve(engine, [p], t, 0, outputs_per_launch=m)
        _assert_leapt(run[1], [p], t, m, fan)
        assert base[1]["leap_problems"] == 0 and base[1]["mode"] == 1
        obs, final = run[0][0], run[2][0]
        e_obs = float(np.max(np.abs(obs - ref_obs[:, :ni + 1])))
        e_fin = float(np.max(np.abs(final - states[ni])))
        e_norm = float(np.max(np.abs(obs[6] - 1.0)))
        d = _diff(run, base)
        print(f"n = {n} x0 = {x0:#x} m = {m} fan = {fan}, {ni} intervals: observables {e_obs:.2e}, final state {e_fin:.2e} (bound "
              f"{BOUND:g}), norm {e_norm:.2e} (bound {NORM_BOUND:g}), against leap = 0 {d:.2e} (bound {ENGINE_BOUND:g})")
        _note("1 against expm_multiply", max(e_obs, e_fin))
        _note("1 norm", e_norm)
        _note("1 against leap = 0", d)
        assert e_obs < BOUND and e_fin < BOUND and e_norm < NORM_BOUND and d < ENGINE_BOUND, (ni, e_obs, e_fin, e_norm, d)


def test_grid_from_zero(engine):
    p, key = problem1(14)
    t = T10 - T10[0]
    run = _evolve(engine, [p], t, 1)
    _assert_leapt(run[1], [p], t)
    states, ref_obs = reference(key, p)   # H is constant: the same states on the shifted grid
    e = max(float(np.max(np.abs(run[0][0] - ref_obs[:, :10]))), float(np.max(np.abs(run[2][0] - states[9]))))
    print(f"t_0 = 0: against expm_multiply {e:.2e} (bound {BOUND:g})")
    assert e < BOUND and float(np.max(np.abs(run[0][0][6] - 1.0))) < NORM_BOUND


@pytest.mark.parametrize("fan", [1, 2])
def test_bench_grid_matches_reference_n14(engine, golden, fan):
    """The bench's whole grid (1 ms, 101 outputs: 50 launches of two outputs, 25 of four) on the bench's
    registers at three detunings, against the traces of the reference's own Hamiltonian that
    tests/test_gpu_config3_bench.py holds every other N = 14 path to, at its bounds: the time recurrence's
    rounding and truncation grow with the launches, and this is the longest chain the path is meant for."""
    from quantumsimulations_amd import problem as pb
    from quantumsimulations_amd.sweep import VARIANTS, sweep_point_params

    g = golden("hpsi_traces_n14_bench.npz")
    t = g["t"]
    assert len(t) == 101 and t[-1] == 1e-3
    keys = [f"{v}_{d}" for v in VARIANTS for d in (0, 75000, 150000)]
    probs = [pb.build_problem(sweep_point_params(13, float(d), v, 1e-3, 101)) for v in VARIANTS for d in (0, 75000, 150000)]
    obs, st, _ = _evolve(engine, probs, t, 1, leap_fan=fan)
    _assert_leapt(st, probs, t, 2, fan)
    worst = worst_norm = 0.0
    for i, key in enumerate(keys):
        for j, k in enumerate(("Ix_sea", "Iy_sea", "Iz_sea", "Iz_R", "Ix_R", "Iy_R")):
            worst = max(worst, float(np.max(np.abs(obs[i, j] - g[f"{key}_{k}"]))))
        worst_norm = max(worst_norm, float(np.max(np.abs(obs[i, 6] - g[f"{key}_state_norm"]))))
    print(f"bench grid, leap_fan = {fan}: max |GPU - reference-H oracle| = {worst:.2e} (bound {BOUND:g}), norm {worst_norm:.2e} "
          f"(bound {NORM_BOUND:g}), degree {st['max_degree']}")
    _note(f"1 bench grid fan {fan}", worst)
    _note(f"1 bench grid fan {fan} norm", worst_norm)
    assert worst < BOUND and worst_norm < NORM_BOUND, (worst, worst_norm)


# ------------------------------------------------------------------------------ 2. fall-backs
def _pair():
    (a, _), (b, _) = problem1(14), problem1(13)
    return [a, b]


def _coarse():
    p, _ = problem1(13)
    return [p], np.arange(3) * (420.0 / half_width(p))


FALLBACKS = {
    "non_uniform": lambda: (_pair(), T6, None, {}),
    "product_state": lambda: (_pair(), T10[:6], [("product", product_amps(14, 9414)), None], {}),
    "custom_state": lambda: (_pair(), T10[:6], [None, general_state(13, 9313)], {}),
    "general_phase_drive": lambda: (fallback_problems("complex")[0], T10[:6], None, {}),
    "n12_in_context": lambda: (fallback_problems("n12")[0], T10[:6], None, {}),
    "obs_overlap": lambda: (_pair(), T10[:6], None, {"obs_overlap": 1}),
    "coarse": lambda: _coarse() + (None, {}),
    "one_output_per_launch": lambda: (_pair(), T10[:6], None, {"outputs_per_launch": 1}),
}


@pytest.mark.parametrize("kind", sorted(FALLBACKS))
def test_fallbacks(engine, kind):
    probs, t, inits, opts = FALLBACKS[kind]()
    run = _evolve(engine, probs, t, 1, inits, **opts)
    base = _evolve(engine, probs, t, 0, inits, **opts)
    assert run[1]["leap_problems"] == 0 and base[1]["leap_problems"] == 0 and run[1]["mode"] == 1, run[1]
    _same_bits(f"fall-back {kind}", run, base)


def test_continue_from_final_falls_back(engine):
    p, key = problem1(14)
    h = 4
    with _context(engine, [p], 1) as c:
        first = c.evolve(T10[:h + 1])
        _assert_leapt(first[1], [p], T10[:h + 1])
        engine.continue_from_final(c.pids[0])
        start = engine.initial_state(c.pids[0])
        assert np.array_equal(start, first[2][0]) and np.iscomplexobj(start) and np.count_nonzero(start.imag) > 0
        second = c.evolve(T10[h:])
        assert second[1]["leap_problems"] == 0 and second[1]["custom_init_problems"] == 1
    base = _evolve(engine, [p], T10[h:], 0, [first[2][0]])
    _same_bits("second half from the leap evolve's final state", second, base)
    states, ref_obs = reference(key, p)
    e = max(float(np.max(np.abs(second[0][0] - ref_obs[:, h:10]))), float(np.max(np.abs(second[2][0] - states[9]))))
    print(f"continued evolve against expm_multiply {e:.2e} (bound {BOUND:g})")
    assert e < BOUND


AUTO = {"span_tile": -1, "span_chunks": 0, "span_partial": 0}   # the automatic span policy's forms off


def test_automatic_rule(engine):
    probs, t = _pair(), T10[:6]
    base = _evolve(engine, probs, t, 0, **AUTO)
    assert base[1]["leap_problems"] == 0 and base[1]["span_problems"] == 0 and base[1]["mode"] == 1
    auto = _evolve(engine, probs, t, -1, **AUTO)
    _assert_leapt(auto[1], probs, t)
    d = _diff(auto, base)
    print(f"leap = -1 against leap = 0: {d:.2e} (bound {ENGINE_BOUND:g})")
    assert d < ENGINE_BOUND
    for label, opts in (("span_tile = 0", dict(AUTO, span_tile=0)), ("spin_limit off its default", dict(AUTO, spin_limit=1 << 20))):
        run = _evolve(engine, probs, t, -1, **opts)
        assert run[1]["leap_problems"] == 0 and run[1]["real_problems"] == 0, (label, run[1])
        _same_bits(f"leap = -1 with {label}", run, _evolve(engine, probs, t, 0, **opts))
    real = _evolve(engine, probs, t, -1, **dict(AUTO, real=1))
    assert real[1]["leap_problems"] == 0 and real[1]["real_problems"] == 2, real[1]
    _same_bits("leap = -1 with real = 1", real, _evolve(engine, probs, t, 0, **dict(AUTO, real=1)))


# ------------------------------------------------------------------------------ 3. repeats, contexts
@pytest.mark.parametrize("fan", [1, 2])
def test_repeated_evolves_are_bitwise_equal(engine, fan):
    p, _ = problem1(14)
    with _context(engine, [p], 1, leap_fan=fan) as c:
        runs = [c.evolve(T10) for _ in range(3)]
    for i, r in enumerate(runs):
        _assert_leapt(r[1], [p], T10, 2, fan)
        if i:
            _same_bits(f"evolve {i + 1} of 3", r, runs[0])


@pytest.mark.parametrize("fan", [1, 2])
def test_mixed_context_equals_each_register_alone(engine, fan):
    probs, _ = mixed_problems()
    assert {p.n_qubits for p in probs} == {13, 14}
    run = _evolve(engine, probs, T10, 1, leap_fan=fan)
    _assert_leapt(run[1], probs, T10, 2, fan)
    assert len({leap_prediction([p], T10)[1] for p in probs}) > 1   # unequal degrees
    base = _evolve(engine, probs, T10, 0)
    d = _diff(run, base)
    print(f"five registers against leap = 0: {d:.2e} (bound {ENGINE_BOUND:g})")
    _note("3 mixed against leap = 0", d)
    assert d < ENGINE_BOUND
    for i, p in enumerate(probs):
        alone = _evolve(engine, [p], T10, 1, leap_fan=fan)
        assert alone[1]["leap_problems"] == 1
        _same_bits(f"register {i} (n = {p.n_qubits}) alone", (run[0][i:i + 1], None, run[2][i:i + 1]), alone)


# ------------------------------------------------------------------------------ 4. observable families
@pytest.mark.parametrize("fan", [1, 2])
def test_observable_families(engine, fan):
    from test_gpu_overlap_obs import make_refs

    p, _ = problem1(14)
    n = 14
    refs = make_refs(n, 9514, 3)
    rng = np.random.default_rng(9614)
    ops = rng.integers(0, 8, size=(5, n)).astype(np.uint8)
    ops[0] = 0
    ops[0, 3], ops[0, 12] = 1, 2
    masks = [[(1 << n) - 1, 0, 0], [0x1ff, 1 << 13, 1 << 13], [0x3e00, 1, 0]]
    got = {}
    for leap in (1, 0):
        with _context(engine, [p], leap, site_obs=1, pair_obs=1, leap_fan=fan) as c:
            pid = c.pids[0]
            engine.set_overlap_refs(pid, refs)
            engine.set_op_strings(pid, ops)
            engine.set_sectors(pid, masks)
            obs, st, finals = c.evolve(T10)
            assert st["leap_problems"] == leap
            got[leap] = {"aggregate": obs, "site": engine.site_traces(pid), "pair": engine.pair_traces(pid),
                         "overlap": engine.overlap_traces(pid), "string": engine.op_string_traces(pid),
                         "sector": np.concatenate(engine.sector_traces(pid))}
    for name in got[1]:
        assert got[1][name].shape == got[0][name].shape and got[1][name].shape[-1] == len(T10)
        e = float(np.max(np.abs(got[1][name] - got[0][name])))
        print(f"{name}: max |leap = 1 - leap = 0| = {e:.2e} (bound {ENGINE_BOUND:g})")
        _note(f"4 {name}", e)
        assert e < ENGINE_BOUND, (name, e)
