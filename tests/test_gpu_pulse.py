"""Hard pulses on the device state (dse_apply_pulse, dse_pulse_stats; feature "pulse"), a new H for a
problem that keeps its state (dse_set_hamiltonian) and the pulse sequences built on them
(simulate_rare_sequence(pulses=...)).

Reference: numpy, per bit a tensordot of U_b into the reshaped state (np_pulse).  Bound, componentwise
and derived, not tuned: with B = ((x)_b |U_b|) |psi| from the same routine,
    |kernel - numpy|(x) <= 4 n 2^-52 B(x)   for every x:
n stages of a 2x2 complex product at under 4 ulp each, on both sides (numpy alone, against clongdouble
for n = 3..20, stays below 0.1 of half that bound).  States are dense, complex and scaled by 1.7 as in
test_gpu_initial_state.py; the state of each size is made once and shared.  Two exact propagations of the
engine agree to 1e-11, traces against an exact propagation to 1e-10 (the project's tolerances).

The sizes of the kernel test: 3 and 9 (k_pulse_small: fewer amplitudes than a workgroup, several rows),
12 (one tile), 13 (two tiles, one high bit), 16, and 23, the smallest register whose pulse takes three
passes (group 0 and 11 high bits in two groups); the numpy reference of a 23-bit case takes a few
seconds.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.dipolar_ensemble_with_rare import rotation_matrices
from quantumsimulations_amd.sweep import sweep_point_params
from test_gpu_initial_state import ENGINE_KEYS, SCALE, _amps, _eigh_propagate, _ref_obs, kron_state
from test_gpu_parity import _random_problem
from test_gpu_site_obs import DEFAULTS, T7

pytestmark = pytest.mark.gpu

TB = 12
EPS = 2.0 ** -52
X = np.array([[0, 1], [1, 0]], dtype=complex)


# ------------------------------------------------------------------------------ references
def np_pulse(psi, mats):
    """U psi, U = (x)_b mats[b] (bit b of the index = axis n - 1 - b); an exact identity is skipped
    (it would change nothing: 1 x + 0 y = x)."""
    n = len(mats)
    for b in range(n):
        if np.array_equal(mats[b], np.eye(2)):
            continue
        v = psi.reshape(1 << (n - 1 - b), 2, 1 << b)
        psi = np.tensordot(mats[b], v, axes=(1, 1)).transpose(1, 0, 2).reshape(-1)
    return psi


def bound(psi, mats, factor=1.0):
    return factor * 4 * len(mats) * EPS * np_pulse(np.abs(psi), np.abs(np.asarray(mats)))


_STATES = {}


def state(n):
    if n not in _STATES:
        rng = np.random.default_rng(2300 + n)
        v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
        _STATES[n] = v * (SCALE / np.linalg.norm(v))
    return _STATES[n]


def unitaries(n, seed):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((n, 2, 2)) + 1j * rng.standard_normal((n, 2, 2)))[0]
    return np.ascontiguousarray(q)


def general(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 2, 2)) + 1j * rng.standard_normal((n, 2, 2))


def diagonals(n, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 2, 2), dtype=complex)
    m[:, 0, 0], m[:, 1, 1] = np.exp(1j * rng.uniform(0, 6.28, n)), np.exp(1j * rng.uniform(0, 6.28, n))
    return m


def mix(n, off, seed):
    """identity / diagonal / X / random unitary, bit b of kind (b + off) % 4."""
    m, d = unitaries(n, seed), diagonals(n, seed + 1)
    for b in range(n):
        k = (b + off) % 4
        if k == 0:
            m[b] = np.eye(2)
        elif k == 1:
            m[b] = d[b]
        elif k == 2:
            m[b] = X
    return m


def only(n, bits, mats):
    """mats on the given bits, the identity elsewhere."""
    m = np.tile(np.eye(2, dtype=complex), (n, 1, 1))
    for b in bits:
        m[b] = mats[b]
    return m


def masks(mats):
    act = dg = 0
    for b, m in enumerate(mats):
        d = m[0, 1] == 0 and m[1, 0] == 0
        i = d and m[0, 0] == 1 and m[1, 1] == 1
        act |= int(not i) << b
        dg |= int(d and not i) << b
    return act, dg


def plan_passes(n_local, shard_bits, mats):
    g = (ctypes.c_int32 * 56)()
    G = _lib.lib().dse_pulse_plan(n_local, shard_bits, *masks(mats), g)
    assert G >= 0
    return G


# ------------------------------------------------------------------------------ plumbing
class _ctx:
    """The engine cleared, with options set and restored."""

    def __init__(self, engine, **opts):
        self.engine, self.opts = engine, opts

    def __enter__(self):
        self.engine.clear()
        for k, v in self.opts.items():
            self.engine.set_option(k, v)
        return self.engine

    def __exit__(self, *exc):
        for k in self.opts:
            self.engine.set_option(k, DEFAULTS[k])
        self.engine.clear()


def _add(engine, n, bits=0, seed=None):
    p = _random_problem(n, 700 + n if seed is None else seed, rare_bit=n - 1)
    return p, (engine.add_sharded(p, bits) if bits else engine.add(p))


def _pulsed(engine, pid, v, mats):
    engine.set_initial_state(pid, v)
    engine.apply_pulse(pid, mats)
    return engine.initial_state(pid), engine.pulse_stats()


def _check_case(engine, n, mats, bits=0, passes=None):
    v = state(n)
    with _ctx(engine) as e:
        _, pid = _add(e, n, bits)
        got, st = _pulsed(e, pid, v, mats)
        again, st2 = _pulsed(e, pid, v, mats)
    ref = np_pulse(v, mats)
    lim = bound(v, mats)
    excess = float(np.max(np.abs(got - ref) / lim))
    print(f"n = {n}, shard bits {bits}: passes {st['passes']}, {st['ms']:.3f} ms, "
          f"max |kernel - numpy| / (4 n 2^-52 B) = {excess:.3f}")
    assert np.all(np.abs(got - ref) <= lim), excess
    want = plan_passes(n - bits, bits, mats)
    assert st["passes"] == st2["passes"] == want and (passes is None or want == passes)
    assert st["bytes"] == 32.0 * want * (1 << n)
    assert np.array_equal(got, again)
    return got, ref


# ------------------------------------------------------------------------------ 1. the kernel against numpy
SIZES = (3, 9, TB, TB + 1, 16, 23)
SETS = ("unitary", "general", "mix0", "mix1", "mix2", "mix3")


def _set(n, name):
    if name == "unitary":
        return unitaries(n, 10 * n + 1)
    if name == "general":
        return general(n, 10 * n + 2)
    return mix(n, int(name[3]), 10 * n + 3)


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_numpy(engine, n, name):
    mats = _set(n, name)
    _check_case(engine, n, mats)
    if n == 23 and name in ("unitary", "general"):
        assert plan_passes(23, 0, mats) == 3 and plan_passes(22, 0, mats[:22]) == 2


def test_single_bit_of_each_class_is_one_pass(engine):
    """n = 16: a lane bit, another thread bit, a register bit (all in group 0, two of them also carried
    by a group of high bits), a high bit and the top bit."""
    n = 16
    u = general(n, 161)
    for b in (0, 1, 3, 5, 7, 9, 11, 12, 13, 15):
        _check_case(engine, n, only(n, [b], u), passes=1)
    _check_case(engine, n, only(n, [1, 14], u), passes=2)   # a carried bit and a high bit


@pytest.mark.parametrize("n", [9, 16])
def test_all_diagonal_is_one_pass_and_identity_none(engine, n):
    d = diagonals(n, 31 + n) * np.linspace(0.5, 2.0, n)[:, None, None]  # not unitary either
    _check_case(engine, n, d, passes=1)
    _check_case(engine, n, only(n, [n - 1], d), passes=1)
    v = state(n)
    with _ctx(engine) as e:
        _, pid = _add(e, n)
        got, st = _pulsed(e, pid, v, np.tile(np.eye(2), (n, 1, 1)))
    assert st["passes"] == 0 and st["bytes"] == 0.0 and np.array_equal(got, v)


# ------------------------------------------------------------------------------ 2. loopback registers
@pytest.mark.parametrize("where", ["shard", "local", "both"])
@pytest.mark.parametrize("n,bits", [(10, 1), (13, 3), (16, 2)])
def test_loopback_registers(engine, n, bits, where):
    """Shard bits are high bits that select a base pointer; initial_state returns every shard's slice."""
    u = general(n, 50 * n + bits)
    shard = list(range(n - bits, n))
    local = [0, 2, n - bits - 1] + ([9] if n - bits > 9 else [])
    sel = {"shard": shard, "local": local, "both": list(range(n))}[where]
    got, ref = _check_case(engine, n, only(n, sel, u), bits=bits)
    ok = (np.abs(got - ref) <= bound(state(n), only(n, sel, u))).reshape(1 << bits, -1)
    assert [bool(s.all()) for s in ok] == [True] * (1 << bits)  # shard by shard


# ------------------------------------------------------------------------------ 3. the three kinds of start
@pytest.mark.parametrize("n,bits", [(9, 0), (14, 0), (13, 2)])
def test_product_and_basis_starts(engine, n, bits):
    u = general(n, 77 + n)
    amps = _amps(n, 78 + n)
    with _ctx(engine) as e:
        p, pid = _add(e, n, bits)
        e.set_initial_product(pid, amps)
        e.apply_pulse(pid, u)
        st = e.pulse_stats()
        got = e.initial_state(pid)
        e.set_initial_state(pid, None)      # the basis state
        e.apply_pulse(pid, u)
        got0 = e.initial_state(pid)
    assert st["passes"] == 0 and st["bytes"] == 0.0  # a host path: no kernel
    ref = kron_state(np.einsum("bvw,bw->bv", u, amps))
    excess = float(np.max(np.abs(got - ref) / (4 * n * EPS * np.abs(ref))))
    cols = np.stack([u[b][:, (p.psi0_index >> b) & 1] for b in range(n)])
    ref0 = kron_state(cols)
    excess0 = float(np.max(np.abs(got0 - ref0) / (4 * n * EPS * np.abs(ref0))))
    print(f"product start: max |state - kron| / (4 n 2^-52 |psi|) = {excess:.3f}; basis start: {excess0:.3f}")
    assert excess <= 1.0 and excess0 <= 1.0


@pytest.mark.parametrize("n", [9, 14])
def test_composition_and_inverse(engine, n):
    v = state(n)
    U, V = general(n, 91 + n), unitaries(n, 92 + n)
    W = np.einsum("bij,bjk->bik", V, U)
    Ud = np.conj(np.transpose(unitaries(n, 93 + n), (0, 2, 1)))
    Uu = np.conj(np.transpose(Ud, (0, 2, 1)))
    with _ctx(engine) as e:
        _, pid = _add(e, n)
        e.set_initial_state(pid, v)
        e.apply_pulse(pid, U)
        e.apply_pulse(pid, V)
        two = e.initial_state(pid)
        one, _ = _pulsed(e, pid, v, W)
        e.set_initial_state(pid, v)
        e.apply_pulse(pid, Uu)
        e.apply_pulse(pid, Ud)
        back = e.initial_state(pid)
    lim = 4 * n * EPS * np_pulse(np.abs(v), np.einsum("bij,bjk->bik", np.abs(V), np.abs(U)))
    lim_b = 4 * n * EPS * np_pulse(np.abs(v), np.einsum("bij,bjk->bik", np.abs(Ud), np.abs(Uu)))
    print(f"V after U against VU: {float(np.max(np.abs(two - one) / lim)):.3f} of the bound; "
          f"U then U^+: {float(np.max(np.abs(back - v) / lim_b)):.3f}")
    assert np.all(np.abs(two - one) <= lim)
    assert np.all(np.abs(back - v) <= lim_b)


# ------------------------------------------------------------------------------ 4. engines
def _n7():
    return pb.build_problem(sweep_point_params(6, 50e3, "center_on", 1e-3, 7), order="engine", reduce=False)


ENGINES = {
    "small": (lambda: _n7(), dict(dense=0), T7, lambda st: st["mode"] == 3),
    "interval": (lambda: _random_problem(13, 513, rare_bit=12), dict(tile_bits=13, span_tile=0, matrix=0, dense=0), T7,
                 lambda st: st["mode"] == 1 and st["span_problems"] == 0),
    "wht": (lambda: _random_problem(15, 515, rare_bit=14), dict(span_tile=0), np.linspace(0.0, 1e-3, 3),
            lambda st: st["mode"] == 2),
    "dense": (lambda: _n7(), dict(dense=2), T7, lambda st: st["dense_problems"] == 1),
}


@pytest.mark.parametrize("which", list(ENGINES))
def test_evolve_from_the_pulsed_state(engine, which):
    make, opts, t, on_engine = ENGINES[which]
    p = make()
    n = p.n_qubits
    v, u = state(n), unitaries(n, 40 + n)
    with _ctx(engine, **opts) as e:
        pid = e.add(p)
        e.set_initial_state(pid, v)
        e.apply_pulse(pid, u)
        a, st_a = e.evolve(t)
    with _ctx(engine, **opts) as e:
        pid = e.add(p)
        e.set_initial_state(pid, np_pulse(v, u))
        b, st_b = e.evolve(t)
    assert on_engine(st_a), st_a
    err = float(np.max(np.abs(a - b)))
    print(f"{which}: max |traces(device pulse) - traces(numpy pulse)| = {err:.3e}")
    assert err < 1e-11
    for k in ENGINE_KEYS:
        assert st_a[k] == st_b[k], k


# ------------------------------------------------------------------------------ 5. an echo
def test_hahn_echo_refocuses_every_spin(engine):
    """Ten spins with distinct fields, no couplings, no drives, all along x: tau, pi about x on every
    spin, tau.  The spins dephase (asserted on the host) and the pulse brings every one back."""
    n, tau = 10, 4e-4
    field = 2 * np.pi * (1000.0 + 437.0 * np.arange(n) ** 1.3)
    n_sea = n - 1
    p = pb.Problem(n, field, np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, 4)), 0.0, 0, (1 << n_sea) - 1, n - 1,
                   0.0, np.arange(n), n, False, "engine")
    free = 0.5 * float(np.sum(np.cos(field[:n_sea] * 2 * tau)))  # <Ix_sea>(2 tau) without the pulse
    assert free < 0.5 * n_sea - 0.1, free
    t = np.array([0.0, tau])
    with _ctx(engine) as e:
        pid = e.add(p)
        e.set_initial_product(pid, np.full((n, 2), np.sqrt(0.5), dtype=complex))
        first, _ = e.evolve(t)
        e.continue_from_final(pid)
        none, _ = e.evolve(t)
        e.apply_pulse(pid, rotation_matrices(np.tile([np.pi, 0.0, 0.0], (n, 1))))
        assert e.pulse_stats()["passes"] == 1
        echo, _ = e.evolve(t)
    print(f"Ix_sea: start {first[0, 0, 0]:.12f}, 2 tau without the pulse {none[0, 0, 1]:.6f} (host {free:.6f}), "
          f"echo {echo[0, 0, 1]:.12f}")
    assert abs(first[0, 0, 0] - 0.5 * n_sea) < 1e-12
    assert abs(none[0, 0, 1] - free) < 1e-10
    assert abs(echo[0, 0, 1] - 0.5 * n_sea) < 1e-10


# ------------------------------------------------------------------------------ 6. set_hamiltonian
@pytest.mark.parametrize("bits", [0, 2])
def test_set_hamiltonian_is_a_fresh_context(engine, bits):
    n = 13
    A, B = _random_problem(n, 613, rare_bit=n - 1), _random_problem(n, 614, rare_bit=n - 1)
    B = dataclasses.replace(B, psi0_index=A.psi0_index)
    v = state(n)
    refs = np.stack([state(n)[::-1].copy(), np.roll(state(n), 5) * (0.3 - 0.2j)])
    opts = dict(tile_bits=9) if bits else {}
    t = T7[:4]

    def start(e, prob):
        pid = e.add_sharded(prob, bits) if bits else e.add(prob)
        e.set_overlap_refs(pid, refs)
        e.set_initial_state(pid, v)
        return pid

    with _ctx(engine, **opts) as e:
        pid = start(e, A)
        e.evolve(t)
        e.set_hamiltonian(pid, B)
        for call in (lambda: e.state(pid), lambda: e.continue_from_final(pid)):
            with pytest.raises(RuntimeError, match="-5"):  # DSE_ERR_STATE until the next evolve
                call()
        assert np.array_equal(e.initial_state(pid), v) and e.overlap_refs(pid) == 2
        obs, st = e.evolve(t)
        final, ovl = e.state(pid), e.overlap_traces(pid)
        bad = dataclasses.replace(A, flip=A.flip + np.array([0.0, 1.0, 0.0, 0.0]))  # not Hermitian
        with pytest.raises(ValueError):
            e.set_hamiltonian(pid, bad)
        with pytest.raises(ValueError):
            e.set_hamiltonian(pid, _random_problem(n - 1, 1, rare_bit=n - 2))
        if bits:
            with pytest.raises(ValueError):
                e.set_hamiltonian(pid + 1, A)
        obs2, _ = e.evolve(t)  # the old H (B) stayed
        final2 = e.state(pid)
    with _ctx(engine, **opts) as e:
        pid = start(e, B)
        fresh, st_f = e.evolve(t)
        fresh_final, fresh_ovl = e.state(pid), e.overlap_traces(pid)
    assert np.array_equal(obs, fresh) and np.array_equal(final, fresh_final) and np.array_equal(ovl, fresh_ovl)
    assert np.array_equal(obs2, obs) and np.array_equal(final2, final)
    for k in ENGINE_KEYS:
        assert st[k] == st_f[k], k


# ------------------------------------------------------------------------------ 7. simulate_rare_sequence
def _segments():
    a = sweep_point_params(6, 0.0, "center_on", 1e-3, 9)
    b = sweep_point_params(6, 30e3, "center_on", 5e-4, 6, phi_sea=0.7, phi_rare=0.7)
    c = sweep_point_params(6, -20e3, "center_on", 7e-4, 8, phi_sea=0.0, phi_rare=0.0)
    return [a, b, c]


def test_sequence_without_pulses_is_the_chain_of_simulate_rare_from():
    from quantumsimulations_amd.dipolar_ensemble_with_rare import simulate_rare_from, simulate_rare_sequence
    segs = _segments()
    psi0 = state(7)
    out, final = simulate_rare_sequence(segs, psi0=psi0)
    out_none, final_none = simulate_rare_sequence(segs, psi0=psi0, pulses=[None, None, None])
    psi, t_off = psi0, 0.0
    for seg, (t, obs), (t2, obs2) in zip(segs, out, out_none):
        t1, obs1, psi = simulate_rare_from(seg, psi0=psi, return_state=True)
        assert np.array_equal(t, t1 + t_off) and np.array_equal(t, t2)
        assert list(obs) == list(obs1)
        for k in obs1:
            assert np.array_equal(obs[k], obs1[k]) and np.array_equal(obs2[k], obs1[k]), k
        t_off += float(seg.t_final)
    assert np.array_equal(final, psi) and np.array_equal(final_none, psi)


def test_sequence_with_pulses_matches_numpy_chain():
    """Three segments of different drive phase and detuning at n_sea = 6; rotation vectors (pi / 2 about
    y on the sea, the rare spin left alone), no pulse, and general unitaries given as matrices."""
    from quantumsimulations_amd.dipolar_ensemble_with_rare import build_hamiltonian_rare, simulate_rare_sequence
    segs = _segments()
    n_sites = 7
    rot = np.tile([0.0, np.pi / 2, 0.0], (n_sites, 1))
    rot[6] = 0.0
    rot[2] = [0.3, -1.1, 2.0]
    pulses = [rot, None, unitaries(n_sites, 7007)]
    psi0 = state(7)
    out, final = simulate_rare_sequence(segs, psi0=psi0, pulses=pulses)
    psi, worst = psi0, 0.0
    for seg, pulse, (t, obs) in zip(segs, pulses, out):
        if pulse is not None:
            m = rotation_matrices(pulse) if pulse.ndim == 2 else pulse
            psi = np_pulse(psi, m[::-1])  # site 0 = most significant bit of the reference ket
        H, ops = build_hamiltonian_rare(seg)
        states = _eigh_propagate(H, psi, np.linspace(0.0, seg.t_final, seg.steps))
        ref = _ref_obs(ops, states)
        for k in ref:
            worst = max(worst, float(np.max(np.abs(obs[k] - ref[k]))))
            np.testing.assert_allclose(obs[k], ref[k], rtol=0, atol=1e-10, err_msg=k)
        psi = states[-1]
    print(f"max |traces - numpy chain| = {worst:.3e}, final state {float(np.max(np.abs(final - psi))):.3e}")
    np.testing.assert_allclose(final, psi, rtol=0, atol=1e-10)


# ------------------------------------------------------------------------------ 8. errors, lifetime
def test_errors_leave_the_state_and_lifetime(engine):
    n = 10
    v = state(n)
    u = general(n, 808)
    nan, zero, short = u.copy(), u.copy(), u[:-1]
    nan[3, 0, 1] = np.nan
    zero[4] = 0.0
    kill = np.tile(np.eye(2, dtype=complex), (n, 1, 1))
    with _ctx(engine) as e:
        p, pid = _add(e, n)
        e0 = np.zeros(1 << n, dtype=complex)
        e0[p.psi0_index] = 1.0
        kill[2] = [[0, 1], [0, 0]] if not (p.psi0_index >> 2) & 1 else [[0, 0], [1, 0]]  # maps bit 2's pair to zero
        amps = _amps(n, 809)
        amps[2] = [1.0, 0.0] if not (p.psi0_index >> 2) & 1 else [0.0, 1.0]

        def refused(before):
            for bad in (nan, zero):
                with pytest.raises(ValueError):
                    e.apply_pulse(pid, bad)
            with pytest.raises(ValueError):
                e.apply_pulse(pid, short)
            with pytest.raises(ValueError):
                e.apply_pulse(pid + 1, u)
            assert e._L.dse_apply_pulse(e._h, 7, _lib.ptr(u)) == _lib.DSE_ERR_ARG
            assert e._L.dse_apply_pulse(e._h, pid, None) == _lib.DSE_ERR_ARG
            assert np.array_equal(e.initial_state(pid), before)

        refused(e0)                       # the basis state, before any evolve
        with pytest.raises(ValueError):   # host path: the column of the basis bit is zero
            e.apply_pulse(pid, kill)
        assert np.array_equal(e.initial_state(pid), e0)
        e.set_initial_product(pid, amps)
        before = e.initial_state(pid)
        refused(before)
        with pytest.raises(ValueError):   # host path: the rotated pair is zero
            e.apply_pulse(pid, kill)
        assert np.array_equal(e.initial_state(pid), before)
        e.set_initial_state(pid, v)
        refused(v)
        e.apply_pulse(pid, kill)          # a stored state: singular pulses are not detected
        assert np.all(np.abs(e.initial_state(pid) - np_pulse(v, kill)) <= bound(v, kill))
        # a pulse before any evolve and on a register without a custom state is accepted
        e.clear()
        p, pid = _add(e, n)
        e.apply_pulse(pid, u)
        cols = np.stack([u[b][:, (p.psi0_index >> b) & 1] for b in range(n)])
        ref = kron_state(cols)
        assert np.all(np.abs(e.initial_state(pid) - ref) <= 4 * n * EPS * np.abs(ref))
        obs, st = e.evolve(T7[:3])
        assert st["custom_init_problems"] == 1
        # clear drops everything: the re-added register starts from its basis state
        e.clear()
        with pytest.raises(ValueError):
            e.apply_pulse(pid, u)
        p, pid = _add(e, n)
        assert np.array_equal(e.initial_state(pid), e0)
        # loopback shards: shard 0's id, the other ids are refused and leave the state
        e.clear()
        p, ps = _add(e, n, bits=1)
        e.set_initial_state(ps, v)
        with pytest.raises(ValueError):
            e.apply_pulse(ps + 1, u)
        assert np.array_equal(e.initial_state(ps), v)
