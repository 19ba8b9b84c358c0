"""k_interval<L, IMAG> (csrc/dse_interval.hip; dse_runtime.hip build_tables, assign_lanes,
order_interval_items) on every tile size, drive form and hand-off class, against a CPU
propagation of the same raw-table pb.Problem.

The sweep's tests and tests/test_gpu_parity.py run this kernel on 13- and 14-qubit registers, and
since the automatic span policy (option span_tile = -1) most contexts of few registers run on k_span
instead.  Here every case sets span_tile = 0, span = 0, real = 0, matrix = 0, dense = 0 and the
tile_bits of its registers, so that it reaches k_interval, and asserts mode 1, span_problems =
real_problems = dense_problems = 0, handoff_fallbacks = 0 (a fall-back reruns on another engine and
would hide a wrong kernel), tile_bits = L of the first register, outputs_per_launch, and max_degree
equal to the host prediction (tests/test_interval_cases_host.py predicted_degrees).  Every option a
case depends on is set by _context and restored from RESTORE.

A tile of 2^L amplitudes has TB = L - 4 thread bits b < TB, register bits TB <= b < L and, for a
2-tile register (n = L + 1, option tile_bits = L), the top bit L, whose terms cross the hand-off.  A
1-tile register has n = L (tile_bits = 13).

1. tile size x tiles x form: L = 10 .. 13, 1 and 2 tiles, _random_problem's complex drives
   (k_interval<L, false>) and test_gpu_site_obs._imag_problem (k_interval<L, true>), every coupling and
   drive non-zero, rare_bit = n - 1 (Ix_R, Iy_R, Iz_R on the top bit), on the uneven grid T6 (five
   intervals: at M = 2 launches of 2, 2, 1 outputs).  16 cases; n = 12 at L = 11 is the 2-tile
   register no other test runs.
2. table classes, built from _random_problem by zeroing entries (class_problem; every case asserts
   interval_table(p, L) == class_table first), 2-tile at L = 13 and 11, the marked ones at L = 10 too:
     flip_only       no crossing pair, top drive kept: raw hand-off, cfh[0] at b_me          (also L = 10)
     decoupled       no crossing pair, no top drive: raw hand-off with coefficient 0; the register
                     still hands off every term
     pairs_no_drive  crossing pairs, no top drive: u pre-pass with n_flips_hi = 0            (also L = 10)
     cross_reg012    crossing pairs from register bits 0 .. 2 only: S.xg[0 .. 2], S.xq all 0
     cross_reg3      the crossing pair of register bit 3 only: the half swap
     cross_lanes     crossing pairs from thread bits < 6 only: the pipelined loop            (also L = 10)
     cross_waves     crossing pairs from thread bits >= 6 only: the whole-wave branch (L >= 11)
     sparse          drives on thread bits 0 and 3, register bit 2 and the top bit only, the thread pairs
                     of thread bit 1 zeroed, register pairs zero except (0, 3): partial rflip_mask,
                     zeros in rr_g, zero padding in S.it (at L = 13 too: 28 of 36 slots)
     no_drives       flip = 0: IMAG vacuously, rflip_mask = 0
     residue         imaginary drives with re = 6e-17 |im|: dropped by build_tables' 1e-15 rule, IMAG
                     build; the reference propagates the tables as given
     above_residue   re = 1e-14 |im|: kept, general build
   sparse, no_drives and flip_only also as 1-tile registers at L = 13 and 10 (register bit 3 in the
   top bit's place).  31 cases.
3. series edges, on the complex n = 14 (L = 13) and the imaginary n = 12 (L = 11) register of section
   1: outputs_per_launch 1 and 2 on the 8-point grid T8, chosen on the CPU (series_edges) so that the
   last update of output 0 and of output 1 carries 3, 1 and 2 terms in some launch ((d_j - 1) mod 3),
   one launch has both d_j below the evolve's K (terms past d_j update nothing), and the last
   launch has one output; and a coarse grid (alpha dt = 420 and 462, degree > 400, M = 1 chosen by
   the runtime) on a complex n = 11 register at L = 10: some hundred wraps of the hand-off ring.
4. contexts and schedules: registers of n = 10 .. 14 in one context (tile sizes 10 .. 13 in one
   evolve, a mixed 1- and 2-tile launch at L = 13), forms alternating and all imaginary (an
   imaginary register then runs on the general and on the IMAG build: 1e-11 between them), and n = 10 ..
   12 at tile_bits 11; five 2-tile and two 1-tile registers at L = 11 with coresident 0, 4, 2 and
   xcd_pairs 1, 0 (chunked launches, the mixed launch off when 2 P > cap), bitwise equal per register;
   handoff_fences 1, obs_overlap 1 and mixed_launch 0 bitwise equal to the default run; three evolves
   of one context bitwise equal; continue_from_final over the second half of T6 (1e-11).

Reference: scipy expm_multiply on problem_to_csr(prob), stepped output to output from the basis state
(test_gpu_site_obs.expm_states), oracle.reference_model.observables_bitwise of every state; once per
problem and grid.  Bounds are the project's (test_gpu_parity.py, test_gpu_span_cases.py): 1e-10 for the
seven observables at every output and for the final state, 1e-12 for the norm, 1e-11 between two exact
propagators of the engine.

Measured (MI355X; max over the observables at every output and the final state, per section's worst row):
  section 1   3.9e-15 (L = 12 2-tile complex); every row between 8.8e-16 and 3.9e-15
  section 2   no_drives 1.4e-14, flip_only 8.3e-15, pairs_no_drive 7.2e-15, sparse 7.1e-15, cross_reg3 5.2e-15,
              cross_lanes 4.1e-15, above_residue 2.9e-15, decoupled 2.8e-15, cross_waves 1.8e-15,
              cross_reg012 1.8e-15, residue 1.7e-15
  section 3   T8 m = 1 5.8e-15, m = 2 2.7e-15; coarse grid (degree 537) 7.2e-14 and 3.9e-14 in two runs:
              that case's expm_multiply reference itself moves by 3.8e-14 with the host's thread count
  section 4   8.3e-15 (chunked launches); an imaginary register on the general and on the IMAG build,
              every coresident / xcd_pairs / handoff_fences / obs_overlap / mixed_launch variant, the
              repeats and the continuation: bitwise equal (0.0)
No case found an error in the kernel, in build_tables or in assign_lanes.  At span_tile = -1 the five
older tests named in test_gpu_parity.py / test_gpu_config3.py (now parametrised over span_tile) did run
on k_span: span_problems 3, 8, 6, 9, 6 of their 3, 8, 6, 9, 6 registers.

Sensitivity, with one-line changes of dse_interval.hip in scratch builds (58 cases; coefficients and data
indices only, never a flag, a poll or a wait):
  raw-exchange coefficient at b_pa instead of b_me      5 fail: flip_only at L = 13, 11, 10 and the two
        contexts that hold a flip_only register (chunked launches, option variants); nothing else
  S.xg[3] applied to the same half                      32 fail: cross_reg3 and every 2-tile register with
        all crossing pairs; cross_reg012, cross_lanes, cross_waves, flip_only, decoupled and every
        1-tile case pass
  whole-wave branch's bit test inverted                 28 fail: cross_waves and every full 2-tile register
        at L >= 11; every L = 10 case (coarse grid included), cross_lanes, cross_reg012, cross_reg3 pass
  c0 zero when an update carries three terms            all 58 fail
  hand-off slot of term k read at k % kXSlots           42 fail: every case with a 2-tile register except
        decoupled (its operand has coefficient 0); the 14 lone 1-tile cases and decoupled pass
  1 + 1e-6 on the sweep's drive in k_interval<11, false> alone
        15 fail: section 1 L = 11 complex (1 and 2 tiles), the nine general-drive classes at L = 11 (not
        no_drives, residue: IMAG), both mixed-size contexts, the chunked launches and the repeat
  the same in k_interval<12, true> alone                3 fail: section 1 L = 12 imag (1 and 2 tiles) and
        the mixed-size test (its all-imaginary context)
so option tile_bits and the drive form select the instantiation each case names.
"""
import numpy as np
import pytest

from oracle import reference_model as rm
from test_gpu_site_obs import expm_states
from test_interval_cases_host import (CASES1, CASES2, SECTION3, T6, T8, chosen_m, class_problem, class_table,
                                      coarse_problem, full_table, interval_table, predicted_degrees,
                                      predicted_max_degree, problem1, series_edges, tile_bits_for)

pytestmark = pytest.mark.gpu

BOUND = 1e-10
NORM_BOUND = 1e-12
ENGINE_BOUND = 1e-11   # two exact propagators of the engine
RESTORE = {"span_tile": -1, "span": 0, "real": 0, "matrix": 1, "dense": 1, "tile_bits": 13, "outputs_per_launch": 2,
           "mixed_launch": 1, "obs_overlap": 0, "handoff_fences": 0, "coresident": 0, "xcd_pairs": 1}
SCHEDULE_OPTS = ("outputs_per_launch", "mixed_launch", "obs_overlap", "handoff_fences", "coresident", "xcd_pairs")
assert len(CASES1) == 16 and len(CASES2) == 31 and len(SECTION3) == 2


# ------------------------------------------------------------------------------ references
_REF = {}


def reference(key, p, t):
    """(states on t, their seven observables (7, n_t)) by expm_multiply, once per (problem, grid)."""
    k = (key, tuple(t.tolist()))
    if k not in _REF:
        states = expm_states(("interval_cases",) + tuple(key), p, t)
        obs = np.stack([rm.observables_bitwise(s, p.n_qubits, p.sea_mask, p.rare_bit) for s in states], axis=1)
        _REF[k] = (states, obs)
    return _REF[k]


# ------------------------------------------------------------------------------ plumbing
class _context:
    """The registers probs in the cleared session engine, on k_interval: every option the cases
    depend on set on entry and restored on exit."""

    def __init__(self, engine, probs, tile_bits, **opts):
        assert set(opts) <= set(SCHEDULE_OPTS), opts
        assert opts.get("coresident", 0) in (0, 2, 4)   # never more workgroups than the chip holds resident
        self.engine, self.probs = engine, probs
        self.opts = {"span_tile": 0, "span": 0, "real": 0, "matrix": 0, "dense": 0, "tile_bits": tile_bits}
        self.opts.update({k: RESTORE[k] for k in SCHEDULE_OPTS})
        self.opts.update(opts)

    def __enter__(self):
        self.engine.clear()
        try:
            for k, v in self.opts.items():
                self.engine.set_option(k, v)
            self.pids = [self.engine.add(p) for p in self.probs]
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


def _evolve(engine, probs, t, tile_bits, **opts):
    with _context(engine, probs, tile_bits, **opts) as c:
        return c.evolve(t)


def _assert_interval(st, probs, t, L, m):
    """The evolve ran on k_interval alone, at the tile size and series the case means."""
    assert st["mode"] == 1, st["mode"]
    assert st["span_problems"] == 0 and st["real_problems"] == 0 and st["dense_problems"] == 0, st
    assert st["handoff_fallbacks"] == 0
    assert st["tile_bits"] == L, (st["tile_bits"], L)
    M = chosen_m(probs, t, m)
    assert st["outputs_per_launch"] == M, (st["outputs_per_launch"], M)
    assert st["max_degree"] == predicted_max_degree(probs, t, M), (st["max_degree"], predicted_max_degree(probs, t, M))


_WORST = {}   # (section, row) -> max error seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nmax |k_interval - expm_multiply| (observables at every output, final state):")
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


# ------------------------------------------------------------------------------ 1. tile size x tiles x form
@pytest.mark.parametrize("L,tiles,form,seed", CASES1)
def test_tile_size_tiles_form(engine, L, tiles, form, seed):
    p, key = problem1(L, tiles, form)
    n = p.n_qubits
    assert n == L + tiles - 1 and interval_table(p, L) == full_table(n, L, form == "imag")
    obs, st, finals = _evolve(engine, [p], T6, tile_bits_for(L, tiles))
    _assert_interval(st, [p], T6, L, 2)
    _check(1, f"L = {L} {tiles}-tile {form}", f"k_interval<{L}> n = {n} {form}", obs[0], finals[0], reference(key, p, T6))


# ------------------------------------------------------------------------------ 2. table classes
@pytest.mark.parametrize("cls,L,tiles", CASES2)
def test_table_classes(engine, cls, L, tiles):
    p, key = class_problem(cls, L, tiles)
    assert interval_table(p, L) == class_table(cls, L, tiles), interval_table(p, L)
    obs, st, finals = _evolve(engine, [p], T6, tile_bits_for(L, tiles))
    _assert_interval(st, [p], T6, L, 2)
    _check(2, cls, f"k_interval<{L}> n = {p.n_qubits} {cls}", obs[0], finals[0], reference(key, p, T6))


# ------------------------------------------------------------------------------ 3. series edges
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("L,tiles,form", SECTION3)
def test_series_edges(engine, L, tiles, form, m):
    p, key = problem1(L, tiles, form)
    groups, K = series_edges(p, T8)   # conditions on the inputs, from the host prediction
    obs, st, finals = _evolve(engine, [p], T8, tile_bits_for(L, tiles), outputs_per_launch=m)
    _assert_interval(st, [p], T8, L, m)
    assert st["outputs_per_launch"] == m and st["max_degree"] == predicted_degrees(p, T8, m)[1]
    print(f"n = {p.n_qubits} {form}: degrees per launch at M = 2 {groups}, K = {K}")
    _check(3, f"T8 m = {m}", f"k_interval<{L}> n = {p.n_qubits} {form} outputs_per_launch = {m}", obs[0], finals[0],
           reference(key, p, T8))


def test_coarse_grid(engine):
    p, key, t = coarse_problem()
    obs, st, finals = _evolve(engine, [p], t, 10, outputs_per_launch=2)
    _assert_interval(st, [p], t, 10, 2)
    assert st["outputs_per_launch"] == 1 and st["max_degree"] > 400, st
    print(f"coarse grid: degree {st['max_degree']}")
    _check(3, "coarse", "k_interval<10> n = 11 complex, alpha dt >= 400", obs[0], finals[0], reference(key, p, t))


# ------------------------------------------------------------------------------ 4. contexts and schedules
def _mixed_sizes(forms, sizes):
    """Section-1 registers of the given n -> (L, tiles) and forms."""
    out = [problem1(L, tiles, form) for (L, tiles), form in zip(sizes, forms)]
    return [p for p, _ in out], [k for _, k in out]


SIZES13 = [(10, 1), (11, 1), (12, 1), (13, 1), (13, 2)]   # n = 10 .. 14 at tile_bits 13
SIZES11 = [(10, 1), (11, 1), (11, 2)]                     # n = 10 .. 12 at tile_bits 11
ALTERNATING = ["imag", "complex", "imag", "complex", "imag"]


def test_mixed_tile_sizes(engine):
    runs = {}
    for name, forms in (("alternating", ALTERNATING), ("imaginary", ["imag"] * 5)):
        probs, keys = _mixed_sizes(forms, SIZES13)
        assert [p.n_qubits for p in probs] == [10, 11, 12, 13, 14]
        assert [interval_table(p, L)["imag"] for p, (L, _) in zip(probs, SIZES13)] == [f == "imag" for f in forms]
        obs, st, finals = runs[name] = _evolve(engine, probs, T6, 13)
        _assert_interval(st, probs, T6, 10, 2)
        for i, (p, key) in enumerate(zip(probs, keys)):
            _check(4, f"n = 10 .. 14, {name}", f"{name} register {i}: n = {p.n_qubits} {key[0]}", obs[i], finals[i],
                   reference(key, p, T6))
    # registers 0, 2, 4 are the same imaginary registers in both contexts: general against IMAG build
    for i in (0, 2, 4):
        d = max(float(np.max(np.abs(runs["alternating"][0][i] - runs["imaginary"][0][i]))),
                float(np.max(np.abs(runs["alternating"][2][i] - runs["imaginary"][2][i]))))
        print(f"imaginary register {i}: max |general build - IMAG build| = {d:.2e} (bound {ENGINE_BOUND:g})")
        _note(4, "general against IMAG build", d)
        assert d < ENGINE_BOUND, (i, d)


def test_mixed_tile_sizes_tile_bits_11(engine):
    probs, keys = _mixed_sizes(["complex", "imag", "complex"], SIZES11)
    assert [p.n_qubits for p in probs] == [10, 11, 12]
    obs, st, finals = _evolve(engine, probs, T6, 11)
    _assert_interval(st, probs, T6, 10, 2)
    for i, (p, key) in enumerate(zip(probs, keys)):
        _check(4, "n = 10 .. 12, tile_bits 11", f"register {i}: n = {p.n_qubits} {key[0]}", obs[i], finals[i],
               reference(key, p, T6))


def test_chunked_two_tile_launches(engine):
    """Five 2-tile registers at L = 11 (raw hand-off and u pre-pass side by side) and two 1-tile ones:
    whatever the chunking and the item order, every register's bits are those of the default run."""
    two = [problem1(11, 2, "complex"), problem1(11, 2, "imag"), class_problem("flip_only", 11, 2),
           class_problem("pairs_no_drive", 11, 2), class_problem("sparse", 11, 2)]
    one = [problem1(11, 1, "complex"), problem1(11, 1, "imag")]
    probs, keys = [p for p, _ in two + one], [k for _, k in two + one]
    assert [p.n_qubits for p in probs] == [12] * 5 + [11] * 2
    base = None
    for cores, xcd in ((0, 1), (4, 1), (2, 1), (0, 0), (4, 0), (2, 0)):
        run = _evolve(engine, probs, T6, 11, coresident=cores, xcd_pairs=xcd)
        _assert_interval(run[1], probs, T6, 11, 2)
        for i, (p, key) in enumerate(zip(probs, keys)):
            _check(4, "chunked 2-tile launches", f"coresident {cores} xcd_pairs {xcd} register {i} ({key[0]})",
                   run[0][i], run[2][i], reference(key, p, T6))
        if base is None:
            base = run
        else:
            _same_bits(f"coresident {cores} xcd_pairs {xcd}", run, base)


def test_option_variants_are_bitwise_equal(engine):
    regs = [class_problem("pairs_no_drive", 13, 2), class_problem("flip_only", 13, 2), problem1(13, 1, "complex")]
    probs, keys = [p for p, _ in regs], [k for _, k in regs]
    base = _evolve(engine, probs, T6, 13)
    _assert_interval(base[1], probs, T6, 13, 2)
    for i, (p, key) in enumerate(zip(probs, keys)):
        _check(4, "option variants", f"default options, register {i} ({key[0]})", base[0][i], base[2][i],
               reference(key, p, T6))
    for opt, v in (("handoff_fences", 1), ("obs_overlap", 1), ("mixed_launch", 0)):
        run = _evolve(engine, probs, T6, 13, **{opt: v})
        _assert_interval(run[1], probs, T6, 13, 2)
        _same_bits(f"{opt} = {v}", run, base)


def test_repeated_evolves_are_bitwise_equal(engine):
    p, key = problem1(11, 2, "complex")
    with _context(engine, [p], 11) as c:
        runs = [c.evolve(T6) for _ in range(3)]
    for r in runs:
        _assert_interval(r[1], [p], T6, 11, 2)
    _check(4, "repeat", "n = 12 complex, first of three evolves", runs[0][0][0], runs[0][2][0], reference(key, p, T6))
    for i in (1, 2):
        _same_bits(f"evolve {i + 1} of 3", runs[i], runs[0])


def test_continuation(engine):
    p, key = problem1(13, 2, "complex")
    h = 2
    with _context(engine, [p], 13) as c:
        whole = c.evolve(T6)
        first = c.evolve(T6[:h + 1])
        engine.continue_from_final(c.pids[0])
        second = c.evolve(T6[h:])
    for r, t in ((whole, T6), (first, T6[:h + 1]), (second, T6[h:])):
        _assert_interval(r[1], [p], t, 13, 2)
    ref = reference(key, p, T6)
    _check(4, "continuation", "n = 14 complex, one evolve over T6", whole[0][0], whole[2][0], ref)
    _check(4, "continuation", "n = 14 complex, second half from the first half's final state", second[0][0],
           second[2][0], (ref[0][h:], ref[1][:, h:]))
    d = max(float(np.max(np.abs(second[0][0] - whole[0][0][:, h:]))), float(np.max(np.abs(second[2][0] - whole[2][0]))))
    print(f"continuation: max |two evolves - one| = {d:.2e} (bound {ENGINE_BOUND:g})")
    _note(4, "continuation against one evolve", d)
    assert d < ENGINE_BOUND, d
