"""Host side of the leap path (dse_real.hip k_leap_combine, dse_runtime.hip choose_leap): a
numpy restatement of what the path computes, the uniform-grid rule, and the host's degree and term-count
prediction that tests/test_gpu_leap.py holds the stats to.  No device is touched.

With imaginary drives H' = D H D^dagger, D = diag(i^popcount), is real symmetric.  With H' = alpha H~' + beta
and chi(t) = e^{i beta (t - t0)} D psi(t) / i^|x0| = p(t) + i q(t) from the basis state x0,
    p(t) = cos(alpha H~' (t - t0)) e_x0,    q(t) = -sin(alpha H~' (t - t0)) e_x0
and on a uniform grid of spacing delta, with C_j = cos(alpha H~' j delta), S_j = sin(alpha H~' j delta):
    p_{m+j} = 2 C_j p_m - p_{m-j},    q_{m+j} = q_{m-j} - 2 S_j p_m     (m >= j)
    p_j = C_j p_0,                    q_j = -S_j p_0                    (m = 0).
C_j p_m and S_j p_m are the even and the odd part of ONE real Chebyshev series T_k(H~') p_m with the
coefficients a_k = (2 - delta_k0) (-i)^k J_k(alpha j delta): real for even k, imaginary for odd k.  A launch at
output m covers the outputs m + 1 .. m + 2 G (G = 1: one workgroup's two sums; G = 2: a second workgroup's
two sums of the offsets 3 delta, 4 delta from the same p_m).

* leap_states: the restatement, on D H D^dagger of problem_to_csr at n = 8, 9, 10, 101 outputs at alpha delta
  = 70, G = 1 and 2, against eigh of the unrotated H: state within 1e-11, norm within 1e-12.  One-line errors
  of the restatement (the sign of the odd sum, the factor 2, a history index off by one, the m = 0 form at
  m > 0) must each miss the state bound.
* dse_uniform_spacing (the rule choose_leap applies) on linspace grids, on t_0 != 0, on a grid with one point
  moved by 4 ulp(t_last) and by 1 ulp, against a numpy restatement of the rule.
* leap_prediction: max_degree = the largest series degree of the offsets j delta, j <= M, and
  h_applications = sum over registers of that degree x launches, ceil((n_t - 1) / M) launches; at the bench's
  alpha = 7.0e6 rad/s, delta = 1e-5 s the degrees DESIGN 4.1d quotes, K(2 delta) = 192 and K(4 delta) = 345,
  to within the two terms by which the quoting rule and cheb_series' differ.
"""
import math

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd.dipolar_ensemble_with_rare import problem_to_csr
from quantumsimulations_amd.engine import bessel_native, spectral_bounds_native
from test_gpu_site_obs import _imag_problem
from test_interval_cases_host import half_width, series_degree

STATE_BOUND = 1e-11
NORM_BOUND = 1e-12


# ------------------------------------------------------------------------------ the restatement
def rotated_h(p):
    """D H D^dagger as a dense real matrix (the imaginary part must vanish: imaginary drives)."""
    H = problem_to_csr(p).toarray()
    pop = np.array([bin(v).count("1") for v in range(1 << p.n_qubits)])
    Hr = H * np.array([1.0, 1j, -1.0, -1j])[(pop[:, None] - pop[None, :]) % 4]
    assert np.max(np.abs(Hr.imag)) == 0.0
    return Hr.real, pop


def parity_sums(Ht, v, z, flaw=None, tol=1e-14):
    """(E, O) = (cos(z Ht) v, sin(z Ht) v): the even and odd parts of the one real series sum_k a_k T_k(Ht) v,
    a_k = (2 - delta_k0) (-i)^k J_k(z); the kernel's sums hold (E, -O)."""
    d = series_degree(z, tol)
    J = bessel_native(z, d + 1, tol)[0]
    w0, w1 = v, Ht @ v
    E, O = J[0] * w0, 2.0 * J[1] * w1
    for k in range(2, d + 1):
        w0, w1 = w1, 2.0 * (Ht @ w1) - w0
        if k % 2 == 0:
            E = E + 2.0 * (-1) ** (k // 2) * J[k] * w1
        else:
            O = O + 2.0 * (-1) ** ((k - 1) // 2) * J[k] * w1
    return E, (-O if flaw == "sign_of_O" else O)


def leap_tol(n_t, M, tol=1e-14):
    """The truncation tolerance of the leap path's series (build_coefficients): tol / launches.  A truncation
    error E of C_j shifts cos(theta) of every mode in every launch alike, and where |cos(theta)| = 1 the
    time recurrence grows like N^2 E over N launches; E = tol / N keeps the total at the chained schemes' N tol."""
    return tol / max(1, math.ceil((n_t - 1) / M))


def leap_states(p, t, G, flaw=None):
    """psi(t_m) of every output, computational frame, by the leap path's arithmetic with 2 G outputs per launch."""
    Hr, pop = rotated_h(p)
    lo, hi = spectral_bounds_native(p)
    alpha, beta = 0.5 * (hi - lo), 0.5 * (hi + lo)
    Ht = (Hr - beta * np.eye(Hr.shape[0])) / alpha
    delta = _lib.uniform_spacing(t)
    assert delta > 0.0
    n_t, x0 = len(t), int(p.psi0_index)
    tol = leap_tol(n_t, 2 * G)
    two = 1.0 if flaw == "factor_2" else 2.0
    back = 0 if flaw == "history_index" else 1
    P, Q = [np.zeros(1 << p.n_qubits)], [np.zeros(1 << p.n_qubits)]
    P[0][x0] = 1.0
    for m0 in range(0, n_t - 1, 2 * G):
        for j in range(1, min(2 * G, n_t - 1 - m0) + 1):
            E, O = parity_sums(Ht, P[m0], alpha * j * delta, flaw, tol)
            if m0 == 0 or flaw == "first_form":
                P.append(E), Q.append(-O)
            else:
                P.append(two * E - P[m0 - j + 1 - back]), Q.append(Q[m0 - j + 1 - back] - two * O)
    rot = np.array([1.0, 1j, -1.0, -1j])[(pop[x0] - pop) % 4]   # i^{|x0| - |x|}
    return [rot * np.exp(-1j * beta * (t[m] - t[0])) * (P[m] + 1j * Q[m]) for m in range(n_t)], alpha


_EIG = {}


def exact_states(p, t):
    k = (p.n_qubits, int(p.psi0_index), tuple(t.tolist()))
    if k not in _EIG:
        ev, V = np.linalg.eigh(problem_to_csr(p).toarray())
        c0 = V[int(p.psi0_index)].conj()
        _EIG[k] = [V @ (np.exp(-1j * ev * (tm - t[0])) * c0) for tm in t]
    return _EIG[k]


def _grid(p, n_t=101, z=70.0, t0=0.0):
    return t0 + np.arange(n_t) * (z / half_width(p))


def _errors(states, exact):
    e_state = max(float(np.max(np.abs(a - b))) for a, b in zip(states, exact))
    e_norm = max(abs(float(np.vdot(a, a).real) - 1.0) for a in states)
    return e_state, e_norm


CASES = [(8, 9108), (9, 9109), (10, 9110)]


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("n,seed", CASES)
def test_restatement_matches_eigh(n, seed, G):
    p = _imag_problem(n, seed)
    t = _grid(p, t0=0.0 if n != 9 else 2.5e-4)
    states, alpha = leap_states(p, t, G)
    e_state, e_norm = _errors(states, exact_states(p, t))
    print(f"n = {n}, G = {G}, alpha delta = {alpha * (t[1] - t[0]):.1f}, 101 outputs: state {e_state:.2e} "
          f"(bound {STATE_BOUND:g}), norm {e_norm:.2e} (bound {NORM_BOUND:g})")
    assert e_state < STATE_BOUND and e_norm < NORM_BOUND


@pytest.mark.parametrize("flaw", ["sign_of_O", "factor_2", "history_index", "first_form"])
def test_one_line_errors_miss_the_bound(flaw):
    p = _imag_problem(8, 9108)
    t = _grid(p, n_t=10)
    good, _ = leap_states(p, t, 1)
    assert _errors(good, exact_states(p, t))[0] < STATE_BOUND
    e_state, _ = _errors(leap_states(p, t, 1, flaw)[0], exact_states(p, t))
    print(f"{flaw}: state error {e_state:.2e}")
    assert e_state > 1e-3


# ------------------------------------------------------------------------------ the uniform-grid rule
def uniform_rule(t):
    """The rule restated: delta when max_m |t_m - (t_0 + m delta)| <= 2 ulp(|t_last|), else 0."""
    t = np.asarray(t, dtype=float)
    if len(t) < 2:
        return 0.0
    delta = (t[-1] - t[0]) / (len(t) - 1)
    ok = delta > 0 and np.max(np.abs(t - (t[0] + np.arange(len(t)) * delta))) <= 2.0 * np.spacing(abs(t[-1]))
    return float(delta) if ok else 0.0


GRIDS = {"bench": np.linspace(0.0, 1e-3, 101), "t0": np.linspace(3e-4, 1.3e-3, 101), "two": np.array([0.5, 0.75]),
         "arange": 3e-4 + 5e-5 * np.arange(10), "long": np.linspace(0.0, 30.0, 20000)}


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_uniform_grids(name):
    t = GRIDS[name]
    d = _lib.uniform_spacing(t)
    assert d > 0.0 and d == uniform_rule(t) == (t[-1] - t[0]) / (len(t) - 1)


def test_non_uniform_grids():
    t = GRIDS["bench"].copy()
    ulp = np.spacing(t[-1])
    moved4, moved1 = t.copy(), t.copy()
    moved4[50] += 4.0 * ulp
    moved1[50] += 1.0 * ulp
    assert moved4[50] != t[50] and moved1[50] != t[50]
    assert _lib.uniform_spacing(moved4) == 0.0 == uniform_rule(moved4)
    assert _lib.uniform_spacing(moved1) == uniform_rule(moved1) == uniform_rule(t) > 0.0   # within 2 ulp
    uneven = np.array([0.0, 1e-4, 1.5e-4, 3e-4, 3.2e-4, 5e-4])
    assert _lib.uniform_spacing(uneven) == 0.0 == uniform_rule(uneven)
    assert _lib.uniform_spacing(np.array([1e-3])) == 0.0
    with pytest.raises(ValueError):
        _lib.uniform_spacing(np.array([]))


# ------------------------------------------------------------------------------ degrees and terms
def leap_prediction(probs, t, m=2, fan=1):
    """(M, max_degree, h_applications) of an evolve of probs on the leap path with outputs_per_launch = m and
    leap_fan = fan (fan workgroups of two outputs each when m = 2): a launch runs the series of the offsets
    j delta, j <= M, and its chain is the longest of them, which is what h_applications counts."""
    delta = _lib.uniform_spacing(t)
    assert delta > 0.0
    assert m == 2   # choose_leap: two outputs per series only
    M = max(1, min(m * fan, len(t) - 1))
    launches = math.ceil((len(t) - 1) / M)
    tol = leap_tol(len(t), M)
    deg = [max(series_degree(half_width(p) * j * delta, tol) for j in range(1, M + 1)) for p in probs]
    return M, max(deg), float(sum(deg) * launches)


def test_bench_degrees():
    """The degrees DESIGN 4.1d quotes for the bench's stiffest register (alpha = 7.0e6 rad/s, 1 ms / 100)."""
    z = 7.0e6 * 1e-5
    # (quoted from |J_k| < 1e-15 at k and k + 1; cheb_series stops at the last |J_k| > 1e-14: a term or two apart)
    print(f"K(2 delta) = {series_degree(2 * z)}, K(4 delta) = {series_degree(4 * z)}")
    assert abs(series_degree(2 * z) - 192) <= 2 and abs(series_degree(4 * z) - 345) <= 2
    assert series_degree(z) < series_degree(2 * z) < 2 * series_degree(z)
    # the cut at tol / launches (leap_tol) on the bench's grid: 50 launches of two outputs, 25 of four
    k2, k4 = series_degree(2 * z, leap_tol(101, 2)), series_degree(4 * z, leap_tol(101, 4))
    print(f"at tol / launches: K(2 delta) = {k2}, K(4 delta) = {k4}")
    assert 0 < k2 - series_degree(2 * z) <= 6 and 0 < k4 - series_degree(4 * z) <= 6


def test_prediction():
    probs = [_imag_problem(13, 7113), _imag_problem(14, 7114)]
    t = 3e-4 + 5e-5 * np.arange(10)
    M, deg, happl = leap_prediction(probs, t)
    d = [series_degree(half_width(p) * 1e-4, 1e-14 / 5) for p in probs]
    assert M == 2 and deg == max(d) and happl == 5.0 * sum(d)
    assert leap_prediction(probs, t[:2])[0] == 1
    d4 = [series_degree(half_width(p) * 2e-4, 1e-14 / 3) for p in probs]
    assert leap_prediction(probs, t, 2, 2) == (4, max(d4), 3.0 * sum(d4))   # launches of 4, 4, 1 outputs
    assert leap_prediction(probs, t[:4], 2, 2)[0] == 3
