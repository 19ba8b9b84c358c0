"""Host side of the custom initial states (ABI 14.1): the reference-order <-> engine-order
permutation, Bloch vectors -> amplitudes, the sequence helper's argument checks, the ctypes mirror
and the new kernels' resources.  No device call."""
import ctypes
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd import dipolar_ensemble_with_rare as dr
from quantumsimulations_amd import engine as eng_mod
from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.sweep import sweep_point_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _amps(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))


def _engine_product(amps_by_bit):
    """psi(x) = prod_b a_b[bit_b(x)]: Kronecker product with bit n - 1 the most significant."""
    v = np.ones(1, dtype=complex)
    for a in amps_by_bit[::-1]:
        v = np.kron(v, a)
    return v


@pytest.mark.parametrize("order", ["engine", "reference"])
@pytest.mark.parametrize("variant", ["center_on", "shell_off"])
def test_permutation_against_kronecker_products(order, variant):
    """A product ket of distinct per-site amplitudes, reference order (site 0 most significant)
    against the register order of a built problem (bit b = site site_of_bit[b])."""
    prob = pb.build_problem(sweep_point_params(5, 25e3, variant, 1e-3, 5), order=order, reduce=False)
    n = prob.n_qubits
    assert n == 6
    amps = _amps(n, 11)
    ref = dr.product_state_reference(amps)
    np.testing.assert_allclose(ref, np.kron(np.kron(np.kron(amps[0], amps[1]), np.kron(amps[2], amps[3])),
                                            np.kron(amps[4], amps[5])), rtol=1e-15, atol=0)
    want = _engine_product(amps[prob.site_of_bit])
    got = dr.reference_to_engine_state(ref, prob.site_of_bit)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    if order == "reference":  # that register order is the reference's own
        assert np.array_equal(got, ref)
    assert np.array_equal(dr.engine_to_reference_state(got, prob.site_of_bit), ref)


def test_permutation_of_a_scrambled_register():
    sob = np.array([2, 0, 3, 1, 4])
    amps = _amps(5, 12)
    ref = dr.product_state_reference(amps)
    got = dr.reference_to_engine_state(ref, sob)
    np.testing.assert_allclose(got, _engine_product(amps[sob]), rtol=1e-14, atol=0)
    rng = np.random.default_rng(13)
    v = rng.standard_normal(32) + 1j * rng.standard_normal(32)
    assert np.array_equal(dr.engine_to_reference_state(dr.reference_to_engine_state(v, sob), sob), v)
    with pytest.raises(ValueError):
        dr.reference_to_engine_state(v[:16], sob)
    with pytest.raises(ValueError):
        dr.reference_to_engine_state(v, np.array([0, 1, 2, 3, 3]))


def test_bloch_vectors_to_amplitudes():
    s = 1.0 / np.sqrt(2.0)
    a = dr.spin_amplitudes(np.array([[1.0, 0, 0], [-2.0, 0, 0], [0, 3.0, 0], [0, 0, 0.5], [0, 0, -1.0]]), 5)
    np.testing.assert_allclose(a, [[s, s], [s, -s], [s, 1j * s], [1, 0], [0, 1]], rtol=0, atol=1e-15)
    rng = np.random.default_rng(14)
    r = rng.standard_normal((6, 3)) * 3.0
    a = dr.spin_amplitudes(r, 6)
    unit = r / np.linalg.norm(r, axis=1)[:, None]
    np.testing.assert_allclose(np.abs(a[:, 0]) ** 2 + np.abs(a[:, 1]) ** 2, 1.0, rtol=0, atol=1e-15)
    xy = np.conj(a[:, 0]) * a[:, 1]  # <Ix> + i <Iy> of one spin
    np.testing.assert_allclose(xy.real, 0.5 * unit[:, 0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(xy.imag, 0.5 * unit[:, 1], rtol=0, atol=1e-15)
    np.testing.assert_allclose(0.5 * (np.abs(a[:, 0]) ** 2 - np.abs(a[:, 1]) ** 2), 0.5 * unit[:, 2], rtol=0, atol=1e-15)
    # the product ket of the Bloch vectors: each site's expectation in the Kronecker product
    psi = dr.product_state_reference(a).reshape([2] * 6)
    for k in range(6):
        m = np.moveaxis(psi, k, 0)
        assert abs(np.vdot(m[0], m[1]) - xy[k]) < 1e-14
    # amplitudes pass through unchanged (unnormalised, complex)
    amps = _amps(4, 15)
    assert np.array_equal(dr.spin_amplitudes(amps, 4), amps)
    for bad in (np.zeros((4, 3)), np.ones((3, 3)), np.ones((4, 4)), np.ones(4),
                np.array([[1.0, 0], [0, 0], [1, 0], [1, 0]]), np.array([[np.nan, 0, 1.0]] * 4)):
        with pytest.raises(ValueError):
            dr.spin_amplitudes(bad, 4)


def test_sequence_and_start_argument_checks():
    a = sweep_point_params(6, 50e3, "center_on", 1e-3, 9)
    ok = dataclasses.replace(a, drive_sea=False, phi_rare=0.0, B1_rare=0.0, omega_rf_sea=None, t_final=2e-4, steps=3)
    assert dr._check_segments([a, ok]) == [a, ok]
    for name, value in (("n_sea", 5), ("is_center_rare", False), ("gamma_rare", 1.0), ("dipolar_scale", 1.0),
                        ("shell_scale", 1.0), ("gamma_sea", 2.0)):
        with pytest.raises(ValueError, match=name):
            dr._check_segments([a, ok, dataclasses.replace(a, **{name: value})])
    with pytest.raises(ValueError):
        dr._check_segments([])
    psi0 = np.ones(1 << 7, dtype=complex)
    spins = np.ones((7, 2))
    # argument errors are raised before any engine is created
    with pytest.raises(ValueError):
        dr.simulate_rare_sequence([a, dataclasses.replace(a, n_sea=5)], psi0=psi0)
    with pytest.raises(ValueError):
        dr.simulate_rare_sequence([a], psi0=psi0, spins=spins)
    with pytest.raises(ValueError):
        dr.simulate_rare_sequence([a])
    with pytest.raises(ValueError):
        dr.simulate_rare_from(a)
    with pytest.raises(ValueError):
        dr.simulate_rare_from(a, psi0=psi0, spins=spins)
    with pytest.raises(ValueError):
        dr.simulate_rare_from(a, psi0=psi0[:-1])
    with pytest.raises(ValueError):
        dr.simulate_rare_from(a, spins=np.ones((6, 2)))


def test_problem_bytes_counts_the_stored_state():
    prob = pb.build_problem(sweep_point_params(13, 0.0, "center_on", 1e-3, 5))
    assert eng_mod.problem_bytes(prob, True) - eng_mod.problem_bytes(prob) == 16 * prob.dim
    assert eng_mod.problem_bytes(prob, False) == eng_mod.problem_bytes(prob)


def test_abi_14_1_surface():
    """The additions leave every earlier entry as it is: the version stays 14, the minor number says
    that the initial-state entries are there."""
    assert _lib.DSE_ABI_VERSION == 14 and _lib.DSE_ABI_MINOR == 1
    with open(os.path.join(ROOT, "include", "dse.h")) as f:
        header = f.read()
    assert "#define DSE_ABI_VERSION 14" in header and "#define DSE_ABI_MINOR 1" in header
    assert "dse_abi_minor" in _lib.EXPORTED and "int dse_abi_minor(void);" in header
    for name in ("dse_set_initial_state", "dse_set_initial_product", "dse_continue_from_final",
                 "dse_get_initial_state"):
        assert name in _lib.EXPORTED and f"int {name}(" in header
    assert _lib.DseStats._fields_[-1] == ("custom_init_problems", ctypes.c_int32)


def test_dse_stats_mirror_has_the_new_counter_where_c_has_it(tmp_path):
    from test_site_obs_host import _host_cc
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dse.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(dse_stats), offsetof(dse_stats, custom_init_problems)); return 0; }\n')
    exe = tmp_path / "sz"
    res = subprocess.run([_host_cc(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    size, off = (int(x) for x in run.stdout.split())
    assert ctypes.sizeof(_lib.DseStats) == size
    assert _lib.DseStats.custom_init_problems.offset == off


def test_initial_state_kernels_use_no_scratch(tmp_path):
    """k_product_state, k_real_split, k_dense_project (dse_init.hip) and k_dense_phase_c
    (dse_dense.hip): no spills, no scratch; the product kernel's LDS is its 256-entry row table."""
    from test_build import CSRC, _hipcc, _resources
    found = {}
    for src, names in (("dse_init.hip", ("k_product_state", "k_real_split", "k_dense_project")),
                       ("dse_dense.hip", ("k_dense_phase_c",))):
        res = subprocess.run(
            [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
             "--cuda-device-only", "-c", os.path.join(CSRC, src), "-o", str(tmp_path / (src + ".o")),
             "-Rpass-analysis=kernel-resource-usage"],
            capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        for name in names:
            rows = [k for k in _resources(res.stderr) if name in k[0]]
            assert len(rows) == 1, (name, rows)
            found[name] = rows[0]
        if src == "dse_init.hip":
            lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", res.stderr)]
            assert max(lds) == 256 * 16, lds
    assert all(sp == 0 and sc == 0 for _, sp, sc in found.values()), found
