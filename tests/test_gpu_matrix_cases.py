"""Propagator-matrix mode (csrc/dse_matrix.hip k_ucols, k_symv, k_symv_reduce; dse_runtime.hip
matrix_run) at every tile size, drive class and thread-pair count, against a CPU
propagation of the same raw-table pb.Problem.

tests/test_gpu_matrix.py and the mode's cases in the other files run it at n = 10 (and config 2 at
n = 12) on Hamiltonians whose list of thread-bit pairs is full.  Here, on t = linspace(0, 1e-3, 17)
(the fewest outputs matrix_eligible takes), options matrix = 2, dense = 0, default tile_bits (L = n,
one tile), registers from test_gpu_parity._random_problem with the drives forced into a class:

  imaginary   flip[b] = [0, a, 0, -a]: rot = 1, parity = 1 (the i^{|c| - |r|} twist, U_cr = s_r s_c U_rc)
  real        flip[b] = [a, 0, a, 0]:  rot = 0, parity = 0
  complex     _random_problem's own drives: k_interval in column mode + zgemv on the whole matrix

1. n = 10 .. 13 (k_ucols<10> .. <13>; nb = 16, 32, 64, 128 block rows in k_symv and its reduce) x
   imaginary / real x the number ntt of non-zero couplings pair[i, j], i < j < TB = n - 4, left by a
   seeded shuffle (the couplings that touch one of the four register bits stay): 0, TB (NPI - 1)
   (ja = 0), TB (NPI - 1) + 1 (ja = 1), the full C(TB, 2), and ntt = 20 at n = 11 (ja = 6: the single
   wave bit takes NPI - 1 pairs), ntt = 34 at n = 13 (ja = 7: wave bit 6 takes NPI pairs, bits 7 and 8
   NPI - 1); tests/test_matrix_algebra.py pins the slot arithmetic.  Each from the register's basis
   state (psi_1 is the column k_ucols writes whole, the later outputs go through the tiles) and from a
   random complex psi0 of norm 1.7 (the first product reads every stored tile).
2. n = 11, both classes: the basis state at index 0 (its column almost entirely in transposed tiles),
   2^n - 1 (entirely in direct tiles), 63, 64, and an odd- and an even-popcount index of the last
   block row.
3. n = 11, 13, imaginary: drives on the thread bits only, on the four register bits only, none.
4. the complex build at n = 11, 12, and at n = 11 imaginary drives on every bit but one real one.
5. option symv_fused = 1 (the reduction inside the product's launch) at n = 10, 11, 13, both classes,
   and its difference from the two-launch form (another summation order: reported, not bounded).
6. sizes back to back on one context (ctx->d_mx only grows; the partials and counters stay with it):
   13 real, 10 imaginary, 11 complex, 11 imaginary fused, 13 real again, bitwise equal to the first.
7. n = 12 real three times: array_equal observables (k_symv_reduce sums in a fixed order).

Every case asserts mode 5, the number of products (n_t - 2 from the basis state, n_t - 1 from a
custom one) and the bytes one product reads: 16 (nb (nb + 1) / 2 64^2 + 2^n) for the half-matrix
tiles of the real build, 16 (4^n + 2^n) for the complex one -- a fall-back to another engine or
build cannot pass.

Reference: scipy expm_multiply on problem_to_csr(prob), step by step on the grid; at n = 10 and 11
also numpy.linalg.eigh (of the rotated real H' where there is one), and the two agree to 3.8e-15
(states 1.6e-15, observables 3.8e-15; n = 10, 11, all three classes, basis start;
test_references_agree holds them to 1e-12: eps ||H|| T ~ 2e-15 per eigenphase, sums over 2^n
terms).  The bound is the project's standing 1e-10 against the exact propagator, for all seven
observables at every output and for the final state.

Measured (MI355X; max over the observables at every output and the final state, over every case of
the size and class in this file, the fused and back-to-back runs included):
  n = 10   imaginary 7.1e-14, real 6.9e-14
  n = 11   imaginary 8.2e-14, real 3.4e-14, complex 6.7e-15, one real drive among imaginary 3.4e-14
  n = 12   imaginary 9.1e-14, real 9.4e-14, complex 8.7e-15
  n = 13   imaginary 7.7e-14, real 5.9e-14
  symv_fused = 1 against symv_fused = 0 (same case, observables and final state): 2.2e-16 to
  4.4e-16 at n = 10, 11 and 13, both classes
No case found an error in the kernels.  Sensitivity, with one-line mutations of dse_matrix.hip in a
scratch build (71 cases in all): cases 1 and 3 of the (pc - popc(x)) & 3 switch of k_ucols swapped
fails 32 (every imaginary-class case with a drive, errors 0.03 to 4.8); max(0, j - ja - 1) in the
slot index fails 26 (every pair count with ja < TB - 1 and a non-empty list, both classes, 4e-4 to
2e-2); the sc sign of k_symv's transposed partial dropped fails 34 (every imaginary-class case, 0.13
to 3.4).
"""
import dataclasses

import numpy as np
import pytest

from test_gpu_initial_state import _run, eigh_from, expm_from, obs_ref
from test_gpu_parity import _rand, _random_problem
from test_matrix_algebra import ja_of, n_pairs, npi_of

pytestmark = pytest.mark.gpu

BOUND = 1e-10
T17 = np.linspace(0.0, 1e-3, 17)
N_T = len(T17)
SCALE = 1.7
BS = 64  # kSymvBlock


# ------------------------------------------------------------------------------ the registers
def _base(n):
    return _random_problem(n, 600 + n, rare_bit=n - 1)


def _with_class(p, cls, real_bit=None):
    """The drives of p forced into a class; the amplitude a_b is the imaginary part _random_problem drew."""
    n = p.n_qubits
    a, z = p.flip[:, 1].copy(), np.zeros(n)
    if cls == "complex":
        return p
    if cls == "imag":
        flip = np.stack([z, a, z, -a], axis=1)
    elif cls == "real":
        flip = np.stack([a, z, a, z], axis=1)
    elif cls == "mixed":  # imaginary but for one real drive: no real rotated form
        flip = np.stack([z, a, z, -a], axis=1)
        flip[real_bit] = [a[real_bit], 0.0, a[real_bit], 0.0]
    else:
        raise ValueError(cls)
    return dataclasses.replace(p, flip=flip)


def _with_ntt(p, ntt):
    """Zero couplings pair[i, j], i < j < TB, chosen by a seeded shuffle, until exactly ntt remain."""
    n = p.n_qubits
    tb = n - 4
    slots = [(i, j) for i in range(tb) for j in range(i + 1, tb)]
    assert len(slots) == n_pairs(tb) and all(p.pair[s] != 0.0 for s in slots)
    order = np.random.default_rng(9000 + n).permutation(len(slots))
    pair = p.pair.copy()
    for k in order[: len(slots) - ntt]:
        pair[slots[k]] = 0.0
    assert sum(pair[s] != 0.0 for s in slots) == ntt
    return dataclasses.replace(p, pair=pair)


def _ntts(n):
    tb = n - 4
    lo = tb * (npi_of(tb) - 1)
    out = [0, lo, lo + 1, n_pairs(tb)]
    if n == 11:
        out.append(20)
    if n == 13:
        out.append(34)
    return out


def _full(n):
    return n_pairs(n - 4)


def _case(n, cls, ntt=None, drives="all", psi0_index=None, real_bit=None):
    p = _with_class(_base(n), cls, real_bit)
    if ntt is not None and ntt != _full(n):
        p = _with_ntt(p, ntt)
    if drives != "all":
        flip = p.flip.copy()
        tb = n - 4
        if drives in ("register", "none"):
            flip[:tb] = 0.0
        if drives in ("thread", "none"):
            flip[tb:] = 0.0
        p = dataclasses.replace(p, flip=flip)
    if psi0_index is not None:
        p = dataclasses.replace(p, psi0_index=int(psi0_index))
    return p


def _psi0(n):
    """Random, fully complex, unnormalised."""
    return _rand(n, 800 + n) * SCALE


def _basis(p):
    v = np.zeros(1 << p.n_qubits, dtype=complex)
    v[p.psi0_index] = 1.0
    return v


# ------------------------------------------------------------------------------ references
_REF = {}


def reference(key, p, start):
    """(states on T17, their observables) by expm_multiply, once per (case, start)."""
    k = (key, start)
    if k not in _REF:
        psi0 = _basis(p) if start == "basis" else _psi0(p.n_qubits)
        states = expm_from(("matrix_cases",) + k, p, T17, psi0)
        _REF[k] = (states, obs_ref(p, states))
    return _REF[k]


# ------------------------------------------------------------------------------ plumbing
def _evolve(engine, p, start, fused=0):
    """One register in matrix mode from its basis state or the custom psi0: obs (7, n_t), stats, final state."""
    init = None if start == "basis" else _psi0(p.n_qubits)
    if fused:
        engine.set_option("symv_fused", 1)
    try:
        obs, st, final = _run(engine, [p], T17, [init], keep=lambda e, pids: e.state(pids[0]), matrix=2, dense=0)
    finally:
        if fused:
            engine.set_option("symv_fused", 0)
    return obs[0], st, final


def _assert_stats(st, n, start, build):
    dim = 1 << n
    nb = dim // BS
    assert st["mode"] == 5, st["mode"]
    assert st["custom_init_problems"] == (0 if start == "basis" else 1)
    assert st["matrix_products"] == N_T - (2 if start == "basis" else 1), st["matrix_products"]
    stored = nb * (nb + 1) // 2 * BS * BS if build == "real" else dim * dim
    assert st["matrix_bytes_per_product"] == 16 * (stored + dim), (st["matrix_bytes_per_product"], build)


_WORST = {}   # (n, class) -> max error seen
_FUSED = {}   # (n, class) -> max |fused - two-launch|


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nmax |matrix mode - expm_multiply| (observables at every output, final state):")
        for (n, cls), e in sorted(_WORST.items()):
            print(f"  n = {n} {cls}: {e:.2e}")
    if _FUSED:
        print("max |symv_fused = 1 - symv_fused = 0| (observables, final state):")
        for (n, cls), e in sorted(_FUSED.items()):
            print(f"  n = {n} {cls}: {e:.2e}")


def _check(label, n, cls, obs, final, ref):
    states, ref_obs = ref
    assert obs.shape == ref_obs.shape
    assert np.all(np.isfinite(obs)) and np.all(np.isfinite(final.view(float)))
    e_obs = float(np.max(np.abs(obs - ref_obs)))
    e_fin = float(np.max(np.abs(final - states[-1])))
    print(f"{label}: observables {e_obs:.2e}, final state {e_fin:.2e} (bound {BOUND:g})")
    _WORST[n, cls] = max(_WORST.get((n, cls), 0.0), e_obs, e_fin)
    assert e_obs < BOUND, (label, e_obs)
    assert e_fin < BOUND, (label, e_fin)


def _both_starts(engine, key, p, n, cls, build="real"):
    for start in ("basis", "custom"):
        obs, st, final = _evolve(engine, p, start)
        _assert_stats(st, n, start, build)
        _check(f"{key} {start}", n, cls, obs, final, reference(key, p, start))


# ------------------------------------------------------------------------------ 0. the references
@pytest.mark.parametrize("cls", ["imag", "real", "complex"])
@pytest.mark.parametrize("n", [10, 11])
def test_references_agree(n, cls):
    """expm_multiply against numpy eigh (of the rotated real H' for the imaginary class).  1e-12: every
    eigenphase is off by eps ||H|| T ~ 2e-15, a state's amplitude sums 2^n of them."""
    p = _case(n, cls)
    states, ref_obs = reference((n, cls, _full(n)), p, "basis")
    eig = eigh_from(("matrix_cases", n, cls), p, T17, _basis(p))
    d_st = max(float(np.max(np.abs(a - b))) for a, b in zip(states, eig))
    d_obs = float(np.max(np.abs(obs_ref(p, eig) - ref_obs)))
    print(f"n = {n} {cls}: expm_multiply against eigh: states {d_st:.2e}, observables {d_obs:.2e}")
    assert d_st < 1e-12 and d_obs < 1e-12


# ------------------------------------------------------------------------------ 1. size x class x pair count
CASES1 = [(n, cls, ntt) for n in (10, 11, 12, 13) for cls in ("imag", "real") for ntt in _ntts(n)]


@pytest.mark.parametrize("n,cls,ntt", CASES1)
def test_size_class_pairs(engine, n, cls, ntt):
    tb = n - 4
    if ntt in (20, 34) and ntt != _full(n):
        assert ja_of(tb, ntt) == {20: 6, 34: 7}[ntt]
    p = _case(n, cls, ntt)
    _both_starts(engine, (n, cls, ntt), p, n, cls)


# ------------------------------------------------------------------------------ 2. the basis column
N2 = 11
ODD_LAST, EVEN_LAST = 2004, 2005   # 0b11111010100, 0b11111010101: block row 31 of 32
COLUMNS = [0, (1 << N2) - 1, 63, 64, ODD_LAST, EVEN_LAST]


@pytest.mark.parametrize("cls", ["imag", "real"])
@pytest.mark.parametrize("x0", COLUMNS)
def test_basis_column(engine, x0, cls):
    assert ODD_LAST // BS == EVEN_LAST // BS == (1 << N2) // BS - 1
    assert bin(ODD_LAST).count("1") % 2 == 1 and bin(EVEN_LAST).count("1") % 2 == 0
    p = _case(N2, cls, psi0_index=x0)
    obs, st, final = _evolve(engine, p, "basis")
    _assert_stats(st, N2, "basis", "real")
    _check(f"n = {N2} {cls} psi0 = e_{x0}", N2, cls, obs, final, reference((N2, cls, "x0", x0), p, "basis"))


# ------------------------------------------------------------------------------ 3. drives on a subset of bits
@pytest.mark.parametrize("drives", ["thread", "register", "none"])
@pytest.mark.parametrize("n", [11, 13])
def test_drive_subsets(engine, n, drives):
    p = _case(n, "imag", drives=drives)
    tb = n - 4
    assert np.any(p.flip[:tb] != 0.0) == (drives == "thread")
    assert np.any(p.flip[tb:] != 0.0) == (drives == "register")
    _both_starts(engine, (n, "imag", "drives", drives), p, n, "imag")


# ------------------------------------------------------------------------------ 4. the complex build
@pytest.mark.parametrize("n", [11, 12])
def test_complex_build(engine, n):
    p = _case(n, "complex")
    assert np.all(p.flip[:, 0] != 0.0) and np.all(p.flip[:, 1] != 0.0)
    _both_starts(engine, (n, "complex", _full(n)), p, n, "complex", build="complex")


def test_one_real_drive_among_imaginary_takes_the_complex_build(engine):
    n = 11
    p = _case(n, "mixed", real_bit=3)
    assert np.count_nonzero(p.flip[:, 0]) == 1 and np.count_nonzero(p.flip[:, 1]) == n - 1
    _both_starts(engine, (n, "mixed", 3), p, n, "mixed", build="complex")


# ------------------------------------------------------------------------------ 5. the fused reduction
@pytest.mark.parametrize("cls", ["imag", "real"])
@pytest.mark.parametrize("n", [10, 11, 13])
def test_symv_fused(engine, n, cls):
    p = _case(n, cls)
    obs, st, final = _evolve(engine, p, "custom", fused=1)
    _assert_stats(st, n, "custom", "real")
    _check(f"n = {n} {cls} symv_fused = 1", n, cls, obs, final, reference((n, cls, _full(n)), p, "custom"))
    obs0, st0, final0 = _evolve(engine, p, "custom")
    _assert_stats(st0, n, "custom", "real")
    d = max(float(np.max(np.abs(obs - obs0))), float(np.max(np.abs(final - final0))))
    _FUSED[n, cls] = d
    print(f"n = {n} {cls}: max |symv_fused = 1 - symv_fused = 0| = {d:.2e}")


# ------------------------------------------------------------------------------ 6. buffer reuse
def test_sizes_back_to_back_on_one_context(engine):
    seq = [(13, "real", 0), (10, "imag", 0), (11, "complex", 0), (11, "imag", 1), (13, "real", 0)]
    got = []
    for n, cls, fused in seq:
        p = _case(n, cls)
        obs, st, final = _evolve(engine, p, "custom", fused=fused)
        _assert_stats(st, n, "custom", "complex" if cls == "complex" else "real")
        _check(f"back to back: n = {n} {cls}" + (" fused" if fused else ""), n, cls, obs, final,
               reference((n, cls, _full(n)), p, "custom"))
        got.append((obs, final))
    assert np.array_equal(got[0][0], got[-1][0]) and np.array_equal(got[0][1], got[-1][1])


# ------------------------------------------------------------------------------ 7. repeatability
def test_repeatable(engine):
    p = _case(12, "real")
    runs = [_evolve(engine, p, "custom") for _ in range(3)]
    for obs, st, final in runs:
        _assert_stats(st, 12, "custom", "real")
    _check("n = 12 real, first of three", 12, "real", runs[0][0], runs[0][2], reference((12, "real", _full(12)), p, "custom"))
    for obs, _, final in runs[1:]:
        assert np.array_equal(obs, runs[0][0])
        assert np.array_equal(final, runs[0][2])
