"""Host-side checks of the hard pulses and of set_hamiltonian (no device): rotation_matrices, the
site -> bit mapping of a pulse, the ValueErrors of simulate_rare_sequence(pulses=...), the header /
_lib surface and dse_has_feature, the pass plan (dse_pulse_plan), and the compiler's resource report
of dse_pulse.hip."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.dipolar_ensemble_with_rare import (pulse_matrices_by_bit, reference_to_engine_state,
                                                                rotation_matrices, simulate_rare_sequence)
from quantumsimulations_amd.sweep import VARIANTS, sweep_point_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dse_apply_pulse", "dse_pulse_stats", "dse_pulse_plan", "dse_set_hamiltonian")
TB = 12   # tile bits of a pass (kPulseTB)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]])
SZ = np.array([[1, 0], [0, -1]], dtype=complex)


# ------------------------------------------------------------------------------ rotation_matrices
def test_rotation_matrices_match_expm():
    from scipy.linalg import expm
    rng = np.random.default_rng(11)
    vecs = rng.standard_normal((40, 3)) * rng.uniform(0.0, 3.0, (40, 1))
    vecs[0] = 0.0                      # the identity
    vecs[1] = [np.pi, 0.0, 0.0]        # pi about x
    vecs[2] = [0.0, np.pi / 2, 0.0]    # pi / 2 about y
    vecs[3] = [0.0, 0.0, 1.234]        # about z: diagonal
    vecs[4] = [1e-9, -2e-9, 5e-10]     # a tiny angle
    u = rotation_matrices(vecs)
    assert u.shape == (40, 2, 2) and u.dtype == np.complex128
    worst = 0.0
    for v, m in zip(vecs, u):
        ref = expm(-0.5j * (v[0] * SX + v[1] * SY + v[2] * SZ))
        worst = max(worst, float(np.max(np.abs(m - ref))))
    print(f"max |rotation_matrices - expm| = {worst:.3e}")
    assert worst <= 1e-15
    assert np.array_equal(u[0], np.eye(2))
    assert u[3][0, 1] == 0.0 and u[3][1, 0] == 0.0  # z rotations stay exactly diagonal (no butterfly)
    assert np.max(np.abs(u[1] - (-1j) * SX)) < 1e-15
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((4, 3), dtype=complex), np.full((2, 3), np.nan)):
        with pytest.raises(ValueError):
            rotation_matrices(bad)


# ------------------------------------------------------------------------------ site -> bit
def _apply_numpy(psi, mats_by_bit):
    """U psi, U = (x)_b mats_by_bit[b], bit b of the index = axis n - 1 - b."""
    n = len(mats_by_bit)
    for b in range(n):
        v = psi.reshape(1 << (n - 1 - b), 2, 1 << b)
        psi = np.tensordot(mats_by_bit[b], v, axes=(1, 1)).transpose(1, 0, 2).reshape(-1)
    return psi


@pytest.mark.parametrize("variant", VARIANTS)
def test_site_to_bit_mapping(variant):
    """The pulse given per site in the reference's order (site 0 = most significant bit of the
    reference ket) acts on the register state as the Kronecker product over the sites does on the
    reference ket, for the unreduced register of every variant and for a permuted register."""
    params = sweep_point_params(4, 50e3, variant, 1e-3, 5)
    n_sites = params.n_sea + 1
    rng = np.random.default_rng(5)
    mats = rng.standard_normal((n_sites, 2, 2)) + 1j * rng.standard_normal((n_sites, 2, 2))
    psi_ref = rng.standard_normal(1 << n_sites) + 1j * rng.standard_normal(1 << n_sites)
    U = np.ones((1, 1), dtype=complex)
    for s in range(n_sites):
        U = np.kron(U, mats[s])
    want = U @ psi_ref
    prob = pb.build_problem(params, order="engine", reduce=False)
    assert prob.n_qubits == n_sites
    for sob in (prob.site_of_bit, pb.build_problem(params, order="reference", reduce=False).site_of_bit,
                np.array([2, 0, 4, 1, 3])):
        by_bit = pulse_matrices_by_bit(mats, sob)
        for b in range(n_sites):
            assert np.array_equal(by_bit[b], mats[sob[b]])
        got = _apply_numpy(reference_to_engine_state(psi_ref, sob), by_bit)
        assert np.max(np.abs(got - reference_to_engine_state(want, sob))) < 1e-13
    with pytest.raises(ValueError):
        pulse_matrices_by_bit(mats, np.array([0, 1, 2, 3, 3]))
    with pytest.raises(ValueError):
        pulse_matrices_by_bit(mats[:-1], prob.site_of_bit)


# ------------------------------------------------------------------------------ pulses= errors
def test_pulses_argument_errors(monkeypatch):
    """A wrong length or shape raises ValueError before a device is touched."""
    import quantumsimulations_amd.dipolar_ensemble_with_rare as mod

    def no_device(_device):
        raise AssertionError("the engine was asked for before the arguments were checked")

    monkeypatch.setattr(mod, "_engine", no_device)
    a = sweep_point_params(4, 50e3, "center_on", 1e-3, 5)
    b = dataclasses.replace(a, drive_sea=False)
    psi0 = np.ones(32, dtype=complex)
    rot = np.zeros((5, 3))
    for bad in ([rot], [rot, None, None], [rot, np.zeros((4, 3))], [np.zeros((5, 2)), None],
                [None, np.zeros((5, 2, 3))], [np.zeros((6, 2, 2)), None], [None, np.full((5, 2, 2), np.inf)],
                [np.zeros((5, 3), dtype=complex), None], [None, "x"]):
        with pytest.raises(ValueError):
            simulate_rare_sequence([a, b], psi0=psi0, pulses=bad)
    with pytest.raises(AssertionError):  # well-formed pulses get as far as the engine
        simulate_rare_sequence([a, b], psi0=psi0, pulses=[rot, np.tile(np.eye(2), (5, 1, 1))])
    with pytest.raises(AssertionError):
        simulate_rare_sequence([a, b], psi0=psi0, pulses=None)


# ------------------------------------------------------------------------------ surface
def test_header_and_lib_surface():
    with open(os.path.join(ROOT, "include", "dse.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.EXPORTED, name
        assert re.search(r"\bint %s\(" % name, header), name
    assert '"pulse"' in header and '"set_hamiltonian"' in header
    assert "#define DSE_ABI_VERSION 14" in header and "#define DSE_ABI_MINOR 1" in header  # no version bump
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.dse_has_feature(b"pulse") == 1 and L.dse_has_feature(b"set_hamiltonian") == 1
    assert L.dse_has_feature(b"pulses") == 0 and L.dse_has_feature(b"overlap_obs") == 1
    assert _lib.has_feature("pulse") and _lib.has_feature("set_hamiltonian")
    from quantumsimulations_amd.engine import Engine
    for name in ("apply_pulse", "pulse_stats", "set_hamiltonian"):
        assert callable(getattr(Engine, name))
    from quantumsimulations_amd.build import SOURCES
    assert "dse_pulse.hip" in SOURCES


# ------------------------------------------------------------------------------ the plan
def plan(n_local, shard_bits, active, diag):
    g = (ctypes.c_int32 * 56)(*([-7] * 56))
    G = _lib.lib().dse_pulse_plan(n_local, shard_bits, active, diag, g)
    assert G >= 0, (n_local, shard_bits, active, diag, G)
    return [dict(c=g[14 * i], pos=[g[14 * i + 1 + q] for q in range(TB)], bfly=g[14 * i + 13]) for i in range(G)]


def expected_passes(n, active, diag):
    """What the plan's rule gives: registers below 2^12 amplitudes one pass; else group 0 when a low bit
    has a non-diagonal matrix, ceil(h / 10) groups for the h such high bits, and one pass for
    diagonal matrices only."""
    nd = active & ~diag
    if not active:
        return 0
    if n < TB:
        return 1
    low = nd & ((1 << TB) - 1)
    h = bin(nd >> TB).count("1")
    return max(1, (1 if low else 0) + (h + 9) // 10)


def check_plan(n_local, S, active, diag):
    n = n_local + S
    P = plan(n_local, S, active, diag)
    nd = active & ~diag
    assert len(P) == expected_passes(n, active, diag), (n_local, S, hex(active), hex(diag))
    seen = 0
    for p in P:
        bits = [b for b in p["pos"] if b >= 0]
        assert len(set(bits)) == len(bits) == min(n, TB) and all(0 <= b < n for b in bits)
        done = 0
        for q in range(TB):
            if (p["bfly"] >> q) & 1:
                assert p["pos"][q] >= 0
                done |= 1 << p["pos"][q]
        assert done & ~nd == 0, "a pass transforms only bits with a non-diagonal matrix"
        assert seen & done == 0, "a bit is transformed once"
        seen |= done
        if any(b >= TB for b in bits):  # a group of high bits: the lowest c >= 2 bits are carried
            assert p["c"] >= 2 and p["pos"][:p["c"]] == list(range(p["c"]))
            assert all(b >= TB for b in p["pos"][p["c"]:]) and p["bfly"] == ((1 << TB) - 1) & ~((1 << p["c"]) - 1)
        else:
            assert p["c"] == 0 and p["pos"][:len(bits)] == list(range(len(bits)))
        assert done or (len(P) == 1 and nd == 0 and diag), "no group without an active bit"
    assert seen == nd, "every bit with a non-diagonal matrix is in exactly one group"
    return len(P)


def test_pulse_plan():
    rng = np.random.default_rng(2024)
    for n in range(1, 35):
        for S in range(0, 4):
            n_local = n - S
            if n_local < 1:
                continue
            full = (1 << n) - 1
            cases = [(0, 0), (full, 0), (full, full), (1, 0), (1 << (n - 1), 0), (1 << (n - 1), 1 << (n - 1))]
            for _ in range(12):
                active = int(rng.integers(0, 1 << 62)) & full
                if rng.integers(0, 3) == 0:  # sparse
                    active &= int(rng.integers(0, 1 << 62))
                cases.append((active, active & int(rng.integers(0, 1 << 62))))
            for active, diag in cases:
                check_plan(n_local, S, active, diag)
            assert check_plan(n_local, S, 0, 0) == 0               # the identity
            assert check_plan(n_local, S, full, full) == 1         # all diagonal
            for b in (0, n // 2, n - 1):                           # one spin
                assert check_plan(n_local, S, 1 << b, 0) == 1
    # three passes first at 23 bits: group 0 and 11 high bits in two groups
    assert check_plan(22, 0, (1 << 22) - 1, 0) == 2 and check_plan(23, 0, (1 << 23) - 1, 0) == 3
    assert check_plan(34, 0, (1 << 34) - 1, 0) == 4
    g = (ctypes.c_int32 * 56)()
    L = _lib.lib()
    for bad in ((0, 0, 0, 0), (35, 0, 0, 0), (32, 3, 0, 0), (10, 4, 0, 0), (10, -1, 0, 0), (10, 0, 1 << 10, 0),
                (10, 0, 1, 2)):
        assert L.dse_pulse_plan(*bad, g) == _lib.DSE_ERR_ARG, bad
    assert L.dse_pulse_plan(10, 0, 1, 0, None) == _lib.DSE_ERR_ARG


# ------------------------------------------------------------------------------ compiler resources
def test_pulse_kernels_use_no_scratch(tmp_path):
    """k_pulse keeps its 16 amplitudes in registers through the three rounds (every index into them
    and into the pass's kernel argument is a compile-time constant) and fits two workgroups per CU;
    k_pulse_small works in LDS."""
    from test_pair_obs_host import _compile_resources
    rows = _compile_resources(tmp_path, "dse_pulse.hip")
    kernels = [k for k in rows if "k_pulse" in k[0]]
    assert len(kernels) == 2 and len(rows) == 2, rows
    assert all(sp == 0 and sc == 0 for _, sp, sc in kernels), kernels
