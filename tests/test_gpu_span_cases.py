"""k_span (csrc/dse_span.hip; dse_runtime.hip build_span_table, order_span_items) on
every instantiated geometry, span width, drive form and operand-kind class, against a CPU
propagation of the same raw-table pb.Problem.

tests/test_gpu_span.py and the kernel's cases in the other files run it on the sweep's Hamiltonians
(13 / 14 qubits, imaginary drives) and mostly against k_interval.  Here every case is one lone
register (section 4: three) with options matrix = 0, dense = 0, so that it reaches k_span, on the
uneven grid T6 = [0, 1e-4, 1.5e-4, 3e-4, 3.2e-4, 5e-4]: five intervals, at the default
span_outputs = 4 a full launch and then a one-output launch.

Geometries (option span_tile, option span_rb -> k_span<L, RB>; from SpanGeo and k_span):
  (11, 0) -> (11, 2)   R = 4 rows, NT = 512 threads, TB = 9 thread bits, NPI = 4, US = 3, NB = 4
  (10, 0) -> (10, 1)   R = 2,      NT = 512,         TB = 9,             NPI = 4, US = 4, NB = 4
  (10, 2) -> (10, 2)   R = 4,      NT = 256,         TB = 8,             NPI = 4, US = 4, NB = 4
(10, 2) is reachable through span_rb = 2 only.  US u operands are built per pre-pass sweep, NB
operands loaded together in phase 4.  A register with every coupling non-zero over s top bits has s
u operands and s + s (s - 1) / 2 SpanOps: 1, 3, 6, 10 for s = 1 .. 4.  So s = 4 on (11, 2) takes two
pre-pass sweeps (3 + 1), s = 3 two phase-4 batches (4 + 2) and s = 4 three (4 + 4 + 2) on every
geometry; s = 1, 2 stay inside one sweep and one batch.

1. geometry x s = 1 .. 4 (n = L + s) x drive form: _random_problem's complex drives (k_span<.,.,false>)
   and test_gpu_site_obs._imag_problem (k_span<.,.,true>).  Every pair and drive non-zero: every top
   bit kind 0, every top-top pair kind 2.  Seeds in CASES1.
2. operand-kind classes, built from _random_problem by zeroing table entries, at (11, 2) n = 14,
   (10, 2) n = 13, (10, 1) n = 12 (mixed: n = 13, it needs three top bits).  L the tile size, TB = L - RB,
   top bits b >= L.  SpanTab by construction (span_table below mirrors build_span_table's sorting and
   every case asserts it):
     raw_only       pair[i, b] = 0 for i < L: ug = 0, u_mask = 0; every top bit kind 1 (c = uflip),
                    every top-top pair kind 2; need_raw = 1; n_ops = s + s (s - 1) / 2
     mixed          top bit L keeps its crossing pairs (kind 0, u_mask = 1); L + 1 has them zeroed and
                    its drive kept (kind 1); L + 2 has neither (no op of its own, uflip = 0; zz, field
                    and its top-top pairs only); 3 kind-2 ops; n_ops = 5, need_raw = 1
     decoupled      every pair and drive touching a top bit zeroed: ug = uflip = 0, u_mask = 0,
                    n_ops = 0, need_raw = 0; nothing is published or polled.  span_eligible does not
                    look at the tables: the register still spans (span_problems = 1), without fallback
     sparse_drives  drives on thread bits 0 and 3, on register bit RB - 1 (rflip_mask = 1 << (RB - 1):
                    partial for RB = 2, the only bit for RB = 1) and on top bit s - 1 only (uflip of the
                    other top bits 0); the thread-thread pairs of thread bit 1 zeroed (TB - 1 fewer
                    entries in the iteration rows), rr_g = 0; crossing pairs kept: every top bit kind 0
     no_drives      flip = 0: imag vacuously true (k_span<.,.,true>), rflip_mask = 0, uflip = 0,
                    iteration rows' drive entries 0; every top bit kind 0, every top-top pair kind 2
   The tables stay in bounds: TB (4 + NPI) = 72 or 64 <= kSpanMaxIt = 160, at most TB (TB - 1) / 2 = 36
   or 28 thread pairs <= TB NPI = 36 or 32, n_ops <= 10 = kSpanMaxOps.
3. span_outputs = 1 .. 4 on the complex n = 14 (11, 2) and the imaginary n = 13 (10, 2) register of
   section 1, on the 8-point uneven grid T8 (7 intervals: launches of 1 x 7; 2, 2, 2, 1; 3, 3, 1; 4, 3
   outputs), every output against the stepped reference; at m = 4 also against span_tile = 0
   (k_interval, 1e-11, two exact propagators of the engine).
4. registers of 13 and 14 qubits in one context at span_tile = 11 (s = 2 and 3 in one launch block,
   sized by its widest register): an imaginary-drive 13-qubit one, a complex 14-qubit one and the
   complex 14-qubit register of section 1.  One complex register makes the launch the general-drive
   form, so the imaginary register runs on k_span<11, 2, false>.

Every case asserts mode 1, span_problems = the number of registers, handoff_fallbacks = 0 (a
fall-back reruns on another engine and would hide a wrong kernel), outputs_per_launch, and restores
span_tile, span_rb, span_outputs, matrix, dense.

Reference: scipy expm_multiply on problem_to_csr(prob), stepped output to output from the basis state
(test_gpu_site_obs.expm_states), oracle.reference_model.observables_bitwise of every state; once per
problem and grid.  Bounds are the project's (test_gpu_parity.py, test_gpu_small.py): 1e-10 for the
seven observables at every output and for the final state, 1e-12 for the norm.

Measured (MI355X; max over the observables at every output and the final state):
  section 1   (11, 2) complex 2.4e-15, imaginary 2.0e-15; (10, 1) complex 2.4e-15, imaginary 3.7e-15;
              (10, 2) complex 2.5e-15, imaginary 4.1e-15
  section 2   raw_only 2.7e-15, mixed 2.1e-15, decoupled 3.7e-15, sparse_drives 6.7e-15, no_drives 1.8e-14
  section 3   m = 1 .. 4: 1.3e-14, 4.0e-15, 3.0e-15, 3.6e-15; against span_tile = 0: 2.8e-15
  section 4   1.6e-15
No case found an error in the kernel or in build_span_table.  Sensitivity, with one-line changes of
dse_span.hip in scratch builds (48 cases): the kind-1 coefficient taken at the other value of the
tile's bit fails 6 (raw_only and mixed on every geometry, nothing else); the a_{k-2} coefficient of a
staggered sum dropped when an update covers three terms (nt >= 4 for nt >= 3) fails all 48, m = 1
included (deterministic: test_gpu_span.py::test_spanned_evolve_is_repeatable passes it); the second
pre-pass sweep storing to the first sweep's slots fails 2 (s = 4 on (11, 2), both forms); the second
and third phase-4 batch applying the first batch's SpanOps fails the 30 cases with more than NB
operands; a factor 1 + 1e-6 on the kind-0 operand in k_span<10, 2, .> alone fails the 15 (10, 2) cases
that have a u operand and no other case, so option span_rb = 2 does reach that instantiation.
"""
import dataclasses

import numpy as np
import pytest

from oracle import reference_model as rm
from test_gpu_parity import _random_problem
from test_gpu_site_obs import _imag_problem, expm_states

pytestmark = pytest.mark.gpu

BOUND = 1e-10
NORM_BOUND = 1e-12
T6 = np.array([0.0, 1e-4, 1.5e-4, 3e-4, 3.2e-4, 5e-4])
T8 = np.array([0.0, 0.6e-4, 1e-4, 1.5e-4, 3e-4, 3.2e-4, 4.1e-4, 5e-4])
RESTORE = {"span_tile": -1, "span_rb": 0, "span_outputs": 4, "matrix": 1, "dense": 1}
GEO = {(11, 0): (11, 2), (10, 0): (10, 1), (10, 2): (10, 2)}  # (span_tile, span_rb) -> (L, RB)


# ------------------------------------------------------------------------------ the tables k_span reads
def span_table(p, L, RB):
    """What build_span_table sorts p into, per class: the kind of every top bit's own operand (0 u,
    1 raw partner under the drive, None no operand), the kind-2 count, and the masks and counts."""
    n = p.n_qubits
    TB, s = L - RB, n - L
    assert s >= 1
    drive = [bool(np.any(p.flip[b] != 0.0)) for b in range(n)]
    cross = [bool(np.any(p.pair[:L, L + b] != 0.0)) for b in range(s)]
    kinds = [0 if cross[b] else (1 if drive[L + b] else None) for b in range(s)]
    n_kind2 = int(np.count_nonzero(np.triu(p.pair[L:, L:], 1)))
    return {
        "kinds": kinds,
        "n_kind2": n_kind2,
        "n_ops": n_kind2 + sum(k is not None for k in kinds),
        "u_mask": sum(1 << b for b in range(s) if cross[b]),
        "need_raw": int(n_kind2 > 0 or 1 in kinds),
        "rflip_mask": sum(1 << (b - TB) for b in range(TB, L) if drive[b]),
        "thread_drives": [b for b in range(TB) if drive[b]],
        "top_drives": [b - L for b in range(L, n) if drive[b]],
        "n_tpairs": int(np.count_nonzero(np.triu(p.pair[:TB, :TB], 1))),
        "n_rr": int(np.count_nonzero(np.triu(p.pair[TB:L, TB:L], 1))),
        "imag": bool(np.all(p.flip[:, 0] == 0.0) and np.all(p.flip[:, 2] == 0.0)),
    }


def _full_table(n, L, RB, imag):
    TB, s = L - RB, n - L
    return {"kinds": [0] * s, "n_kind2": s * (s - 1) // 2, "n_ops": s + s * (s - 1) // 2, "u_mask": (1 << s) - 1,
            "need_raw": int(s > 1), "rflip_mask": (1 << RB) - 1, "thread_drives": list(range(TB)),
            "top_drives": list(range(s)), "n_tpairs": TB * (TB - 1) // 2, "n_rr": RB * (RB - 1) // 2, "imag": imag}


# ------------------------------------------------------------------------------ references
_REF = {}


def reference(key, p, t):
    """(states on t, their seven observables (7, n_t)) by expm_multiply, once per (problem, grid)."""
    k = (key, len(t))
    if k not in _REF:
        states = expm_states(("span_cases",) + tuple(key), p, t)
        obs = np.stack([rm.observables_bitwise(s, p.n_qubits, p.sea_mask, p.rare_bit) for s in states], axis=1)
        _REF[k] = (states, obs)
    return _REF[k]


# ------------------------------------------------------------------------------ plumbing
def _evolve(engine, probs, t, span_tile, span_rb=0, span_outputs=4):
    """Lone registers on k_span (matrix = 0, dense = 0): obs (n_reg, 7, n_t), stats, final states."""
    engine.clear()
    try:
        engine.set_option("matrix", 0)
        engine.set_option("dense", 0)
        engine.set_option("span_tile", span_tile)
        engine.set_option("span_rb", span_rb)
        engine.set_option("span_outputs", span_outputs)
        pids = [engine.add(p) for p in probs]
        obs, st = engine.evolve(t)
        finals = [engine.state(pid) for pid in pids]
    finally:
        for k, v in RESTORE.items():
            engine.set_option(k, v)
        engine.clear()
    return obs[pids], st, finals


def _assert_spanned(st, n_reg, m):
    assert st["mode"] == 1, st["mode"]
    assert st["span_problems"] == n_reg, st["span_problems"]
    assert st["handoff_fallbacks"] == 0
    assert st["outputs_per_launch"] == m, st["outputs_per_launch"]


_WORST = {}   # (section, row) -> max error seen


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nmax |k_span - expm_multiply| (observables at every output, final state):")
        for (sec, row), e in sorted(_WORST.items()):
            print(f"  section {sec} {row}: {e:.2e}")
        for sec in sorted({k[0] for k in _WORST}):
            print(f"  section {sec} worst: {max(e for k, e in _WORST.items() if k[0] == sec):.2e}")


def _check(sec, row, label, obs, final, ref):
    states, ref_obs = ref
    assert obs.shape == ref_obs.shape
    assert np.all(np.isfinite(obs)) and np.all(np.isfinite(final.view(float)))
    e_obs = float(np.max(np.abs(obs - ref_obs)))
    e_fin = float(np.max(np.abs(final - states[-1])))
    e_norm = float(np.max(np.abs(obs[6] - 1.0)))
    print(f"{label}: observables {e_obs:.2e}, final state {e_fin:.2e} (bound {BOUND:g}), norm {e_norm:.2e} "
          f"(bound {NORM_BOUND:g})")
    _WORST[sec, row] = max(_WORST.get((sec, row), 0.0), e_obs, e_fin)
    assert e_obs < BOUND, (label, e_obs)
    assert e_fin < BOUND, (label, e_fin)
    assert e_norm < NORM_BOUND, (label, e_norm)


# ------------------------------------------------------------------------------ 1. geometry x width x form
#         span_tile, span_rb, s, form, seed
CASES1 = [(11, 0, 1, "complex", 7111), (11, 0, 2, "complex", 7112), (11, 0, 3, "complex", 7113), (11, 0, 4, "complex", 7114),
          (11, 0, 1, "imag", 7121), (11, 0, 2, "imag", 7122), (11, 0, 3, "imag", 7123), (11, 0, 4, "imag", 7124),
          (10, 0, 1, "complex", 7211), (10, 0, 2, "complex", 7212), (10, 0, 3, "complex", 7213), (10, 0, 4, "complex", 7214),
          (10, 0, 1, "imag", 7221), (10, 0, 2, "imag", 7222), (10, 0, 3, "imag", 7223), (10, 0, 4, "imag", 7224),
          (10, 2, 1, "complex", 7311), (10, 2, 2, "complex", 7312), (10, 2, 3, "complex", 7313), (10, 2, 4, "complex", 7314),
          (10, 2, 1, "imag", 7321), (10, 2, 2, "imag", 7322), (10, 2, 3, "imag", 7323), (10, 2, 4, "imag", 7324)]
SEED1 = {c[:4]: c[4] for c in CASES1}
assert len(set(SEED1.values())) == len(CASES1) == 24


def _problem1(tile, rb, s, form):
    """The section-1 register of a case and its reference key."""
    n, seed = tile + s, SEED1[tile, rb, s, form]
    p = _random_problem(n, seed, rare_bit=n - 1) if form == "complex" else _imag_problem(n, seed)
    return p, (form, n, seed)


@pytest.mark.parametrize("tile,rb,s,form,seed", CASES1)
def test_geometry_width_form(engine, tile, rb, s, form, seed):
    L, RB = GEO[tile, rb]
    p, key = _problem1(tile, rb, s, form)
    n = p.n_qubits
    assert n == L + s and span_table(p, L, RB) == _full_table(n, L, RB, form == "imag")
    obs, st, finals = _evolve(engine, [p], T6, tile, rb)
    _assert_spanned(st, 1, 4)
    _check(1, f"({L}, {RB}) {form}", f"k_span<{L}, {RB}> s = {s} n = {n} {form}", obs[0], finals[0],
           reference(key, p, T6))


# ------------------------------------------------------------------------------ 2. operand-kind classes
CLASSES = ["raw_only", "mixed", "decoupled", "sparse_drives", "no_drives"]
GEO2 = [(11, 0, 14), (10, 2, 13), (10, 0, 12)]  # span_tile, span_rb, n
SEED2 = {("raw_only", 11, 0): 8111, ("raw_only", 10, 2): 8112, ("raw_only", 10, 0): 8113,
         ("mixed", 11, 0): 8121, ("mixed", 10, 2): 8122, ("mixed", 10, 0): 8123,
         ("decoupled", 11, 0): 8131, ("decoupled", 10, 2): 8132, ("decoupled", 10, 0): 8133,
         ("sparse_drives", 11, 0): 8141, ("sparse_drives", 10, 2): 8142, ("sparse_drives", 10, 0): 8143,
         ("no_drives", 11, 0): 8151, ("no_drives", 10, 2): 8152, ("no_drives", 10, 0): 8153}


def _class_problem(cls, n, L, RB, seed):
    p = _random_problem(n, seed, rare_bit=n - 1)
    TB = L - RB
    pair, flip = p.pair.copy(), p.flip.copy()
    if cls == "raw_only":
        pair[:L, L:] = 0.0
    elif cls == "mixed":
        assert n - L == 3
        pair[:L, L + 1:] = 0.0
        flip[L + 2] = 0.0
    elif cls == "decoupled":
        pair[:, L:] = 0.0
        flip[L:] = 0.0
    elif cls == "sparse_drives":
        for b in range(n):
            if b not in (0, 3, L - 1, n - 1):
                flip[b] = 0.0
        pair[:TB, 1] = 0.0
        pair[1, :TB] = 0.0
        pair[TB:L, TB:L] = 0.0
    elif cls == "no_drives":
        flip[:] = 0.0
    else:
        raise ValueError(cls)
    return dataclasses.replace(p, pair=pair, flip=flip)


def _class_table(cls, n, L, RB):
    """span_table of the class, by construction."""
    TB, s = L - RB, n - L
    T = _full_table(n, L, RB, False)
    if cls == "raw_only":
        T.update(kinds=[1] * s, u_mask=0, need_raw=1)
    elif cls == "mixed":
        T.update(kinds=[0, 1, None], n_ops=5, u_mask=1, need_raw=1, top_drives=[0, 1])
    elif cls == "decoupled":
        T.update(kinds=[None] * s, n_kind2=0, n_ops=0, u_mask=0, need_raw=0, top_drives=[])
    elif cls == "sparse_drives":
        T.update(rflip_mask=1 << (RB - 1), thread_drives=[0, 3], top_drives=[s - 1],
                 n_tpairs=TB * (TB - 1) // 2 - (TB - 1), n_rr=0)
    elif cls == "no_drives":
        T.update(rflip_mask=0, thread_drives=[], top_drives=[], imag=True)
    return T


# mixed needs three top bits: the nearest n that has them
CASES2 = [(cls, tile, rb, max(n, tile + 3) if cls == "mixed" else n) for cls in CLASSES for tile, rb, n in GEO2]


@pytest.mark.parametrize("cls,tile,rb,n", CASES2)
def test_operand_classes(engine, cls, tile, rb, n):
    L, RB = GEO[tile, rb]
    seed = SEED2[cls, tile, rb]
    p = _class_problem(cls, n, L, RB, seed)
    assert span_table(p, L, RB) == _class_table(cls, n, L, RB), span_table(p, L, RB)
    obs, st, finals = _evolve(engine, [p], T6, tile, rb)
    _assert_spanned(st, 1, 4)
    _check(2, cls, f"k_span<{L}, {RB}> n = {n} {cls}", obs[0], finals[0], reference((cls, n, seed), p, T6))


# ------------------------------------------------------------------------------ 3. outputs per launch
@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("tile,rb,s,form", [(11, 0, 3, "complex"), (10, 2, 3, "imag")])
def test_outputs_per_launch(engine, tile, rb, s, form, m):
    L, RB = GEO[tile, rb]
    p, key = _problem1(tile, rb, s, form)
    assert len(T8) - 1 == 7 and np.ptp(np.diff(T8)) > 0.0
    obs, st, finals = _evolve(engine, [p], T8, tile, rb, span_outputs=m)
    _assert_spanned(st, 1, m)
    _check(3, f"m = {m}", f"k_span<{L}, {RB}> n = {p.n_qubits} {form} span_outputs = {m}", obs[0], finals[0],
           reference(key, p, T8))
    if m == 4:
        obs0, st0, finals0 = _evolve(engine, [p], T8, 0)
        assert st0["mode"] == 1 and st0["span_problems"] == 0 and st0["handoff_fallbacks"] == 0
        d = max(float(np.max(np.abs(obs[0] - obs0[0]))), float(np.max(np.abs(finals[0] - finals0[0]))))
        print(f"n = {p.n_qubits} {form}: max |k_span - k_interval| = {d:.2e} (bound 1e-11)")
        _WORST[3, "against span_tile = 0"] = max(_WORST.get((3, "against span_tile = 0"), 0.0), d)
        assert d < 1e-11, d


# ------------------------------------------------------------------------------ 4. mixed widths
def test_mixed_widths_in_one_context(engine):
    p13, p14 = _imag_problem(13, 9113), _random_problem(14, 9114, rare_bit=13)
    p14c, key14c = _problem1(11, 0, 3, "complex")
    probs = [p13, p14, p14c]
    keys = [("imag", 13, 9113), ("complex", 14, 9114), key14c]
    assert [span_table(p, 11, 2)["imag"] for p in probs] == [True, False, False]
    obs, st, finals = _evolve(engine, probs, T6, 11)
    _assert_spanned(st, 3, 4)
    for i, (p, key) in enumerate(zip(probs, keys)):
        _check(4, "s = 2 and 3 in one block", f"register {i}: n = {p.n_qubits} {key[0]}", obs[i], finals[i],
               reference(key, p, T6))
