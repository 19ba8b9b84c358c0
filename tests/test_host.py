"""Host restatement (parameters -> coefficient tables) and libdse's host-only functions, CPU only."""
import dataclasses
import re
import os

import numpy as np
import pytest
import scipy.special as ss

from conftest import ROOT, csr_from
from oracle import reference_model as rm
from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.dipolar_ensemble_with_rare import build_hamiltonian_rare, initial_state_rare, problem_to_csr
from quantumsimulations_amd.model import (dipolar_couplings_from_positions, get_derived_frequencies,
                                          shell_positions_with_rare_center, DipolarRareParams)
from quantumsimulations_amd.sweep import VARIANTS, sweep_point_params


def _tables(prob):
    return {"n": prob.n_qubits, "field": prob.field, "zz": prob.zz, "pair": prob.pair,
            "flip": prob.flip, "shift": prob.shift}


# ---------------------------------------------------------------- parameters / geometry
def test_sweep_params_and_freqs_bit_exact(golden):
    rows = golden("freqs.json")
    for row in rows:
        p = sweep_point_params(6, row["delta_Hz"], row["variant"], 2e-3, 201)
        assert dataclasses.asdict(p) == row["params"]
        f = get_derived_frequencies(p)
        assert list(f.keys()) == list(row["freqs"].keys())
        for k, v in row["freqs"].items():
            assert f[k] == v, k      # bit-for-bit (same float expressions)


def test_geometry_bit_exact(golden):
    g = golden("geometry.npz")
    for n in (1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 20, 29):
        pos = shell_positions_with_rare_center(n, radius=0.282393e-9)
        np.testing.assert_array_equal(pos, g[f"pos_{n}"])
        b = dipolar_couplings_from_positions(pos, 1.0e-7 * 1.054571817e-34, 8.1812e7, 6.976e7)
        np.testing.assert_array_equal(b, g[f"b_center_{n}"])
        b2 = dipolar_couplings_from_positions(pos, 1.0e-7 * 1.054571817e-34, 8.1812e7, 8.1812e7)
        np.testing.assert_array_equal(b2, g[f"b_shell_{n}"])


def test_geometry_errors():
    with pytest.raises(ValueError):
        shell_positions_with_rare_center(0)
    with pytest.raises(ValueError):
        dipolar_couplings_from_positions(np.zeros((2, 3)), 1.0, 1.0, 1.0)


def test_bad_grid_and_spin_three_half():
    p = sweep_point_params(6, 0.0, "center_on", 2e-3, 1)
    with pytest.raises(ValueError):
        pb.time_grid(p)
    with pytest.raises(ValueError):
        pb.time_grid(dataclasses.replace(p, steps=10, t_final=0.0))
    with pytest.raises(ValueError):
        pb.build_problem(DipolarRareParams(n_sea=3))        # default is_spin_three_half=True


# ---------------------------------------------------------------- coefficient tables
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("delta", [0, 25000, 150000])
def test_tables_reproduce_reference_H_n7(golden, variant, delta):
    g = golden("hamiltonian_n7.npz")
    key = f"{variant}_{delta}"
    Href = csr_from(g, key)
    p = sweep_point_params(6, float(delta), variant, 2e-3, 201)
    prob = pb.build_problem(p, order="reference", reduce=False)
    assert prob.psi0_index == int(g[f"{key}_psi0_index"])
    H = problem_to_csr(prob)
    assert abs(H - Href).max() <= 2e-15 * abs(Href).max()
    v = g[f"{key}_v"]
    np.testing.assert_allclose(rm.bitwise_apply(_tables(prob), v), Href @ v, rtol=0,
                               atol=2e-15 * abs(Href).max())


@pytest.mark.parametrize("variant", VARIANTS)
def test_tables_reproduce_reference_Hv_n12(golden, variant):
    g = golden("hpsi_n12.npz")
    p = sweep_point_params(11, 50000.0, variant, 2e-3, 201)
    prob = pb.build_problem(p, order="reference", reduce=False)
    hv = rm.bitwise_apply(_tables(prob), g[f"{variant}_v"])
    ref = g[f"{variant}_Hv"]
    assert np.max(np.abs(hv - ref)) <= 1e-14 * np.max(np.abs(ref))
    obs = rm.observables_bitwise(g[f"{variant}_v"], prob.n_qubits, prob.sea_mask, prob.rare_bit)
    for j, k in enumerate(rm.OBS_ORDER):
        assert abs(obs[j] - float(g[f"{variant}_expect_{k}"])) < 1e-13


def test_build_hamiltonian_rare_observables_match_reference(golden):
    g = golden("hamiltonian_n7.npz")
    p = sweep_point_params(6, 25000.0, "center_on", 2e-3, 201)
    H, obs = build_hamiltonian_rare(p)
    v = g["center_on_25000_v"]
    for k in rm.OBS_ORDER:
        np.testing.assert_allclose(obs[k] @ v, g[f"center_on_25000_O_{k}"], atol=1e-15)
    assert np.argmax(np.abs(initial_state_rare(p))) == int(g["center_on_25000_psi0_index"])


@pytest.mark.parametrize("delta", [0.0, 50000.0])
def test_reduced_center_off_is_exact(delta):
    """center_off: the rare bit is conserved; the reduced register reproduces the full H on
    the psi0 sector (engine order, rare = top bit)."""
    p = sweep_point_params(6, delta, "center_off", 2e-3, 201)
    full = pb.build_problem(p, order="engine", reduce=False)
    red = pb.build_problem(p, order="engine", reduce=True)
    assert red.reduced and red.n_qubits == full.n_qubits - 1 and red.rare_bit == -1
    rare_val = (full.psi0_index >> full.rare_bit) & 1
    assert red.psi0_index == full.psi0_index & ((1 << red.n_qubits) - 1)
    rng = np.random.default_rng(3)
    v = rng.standard_normal(1 << red.n_qubits) + 1j * rng.standard_normal(1 << red.n_qubits)
    vf = np.zeros(1 << full.n_qubits, dtype=complex)
    vf[(rare_val << full.rare_bit) + np.arange(1 << red.n_qubits)] = v
    hf = rm.bitwise_apply(_tables(full), vf)
    hr = rm.bitwise_apply(_tables(red), v)
    sector = (rare_val << full.rare_bit) + np.arange(1 << red.n_qubits)
    np.testing.assert_allclose(hf[sector], hr, rtol=0, atol=1e-9 * np.max(np.abs(hr)))
    assert np.max(np.abs(np.delete(hf, sector))) == 0.0


def test_engine_order_is_permutation_of_reference_order():
    p = sweep_point_params(6, 50000.0, "shell_off", 2e-3, 201)
    a = pb.build_problem(p, order="reference", reduce=False)
    b = pb.build_problem(p, order="engine", reduce=False)
    n = a.n_qubits
    perm = np.zeros(1 << n, dtype=np.int64)   # reference index -> engine index (bit reversal)
    x = np.arange(1 << n)
    for bit in range(n):
        perm |= ((x >> bit) & 1) << (n - 1 - bit)
    rng = np.random.default_rng(5)
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    ve = np.empty_like(v)
    ve[perm] = v
    ha = rm.bitwise_apply(_tables(a), v)
    hb = rm.bitwise_apply(_tables(b), ve)
    np.testing.assert_allclose(hb[perm], ha, atol=1e-9)
    assert perm[a.psi0_index] == b.psi0_index


@pytest.mark.parametrize("variant", VARIANTS)
def test_spectral_bounds_contain_spectrum(variant):
    for delta in (0.0, 150000.0):
        p = sweep_point_params(6, delta, variant, 2e-3, 201)
        prob = pb.build_problem(p, order="engine", reduce=True)
        w = np.linalg.eigvalsh(problem_to_csr(prob).toarray())
        lo, hi = pb.spectral_bounds(prob)
        assert lo <= w.min() + 1e-6 and w.max() <= hi + 1e-6
        # tight: the non-interacting part saturates the bound up to the dipolar width
        assert (hi - lo) < 1.05 * (w.max() - w.min()) + 2e4


# ---------------------------------------------------------------- libdse host-only API
def _lib_or_skip():
    from quantumsimulations_amd import _lib
    return _lib.lib()


def test_library_exports_every_declared_symbol():
    lib = _lib_or_skip()
    from quantumsimulations_amd import _lib
    with open(os.path.join(ROOT, "include", "dse.h")) as f:
        hdr = f.read()
    declared = sorted(set(re.findall(r"\b(dse_[a-z_]+)\s*\(", hdr)))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(_lib.EXPORTED) == declared
    assert lib.dse_abi_version() == _lib.DSE_ABI_VERSION
    assert lib.dse_device_count() >= 0


def test_native_spectral_bounds_match_python():
    from quantumsimulations_amd.engine import spectral_bounds_native
    for variant in VARIANTS:
        p = sweep_point_params(11, 75000.0, variant, 2e-3, 201)
        prob = pb.build_problem(p, order="engine", reduce=True)
        a = spectral_bounds_native(prob)
        b = pb.spectral_bounds(prob)
        np.testing.assert_allclose(a, b, rtol=1e-14)


@pytest.mark.parametrize("z", [0.0, 1e-3, 0.7, 5.0, 37.5, 250.0, 3000.0, 1.2e4])
def test_native_bessel_accuracy(z):
    """J_k(z) against scipy where scipy is accurate (z <= 250), against mpmath spot values and
    the identity J_0^2 + 2 sum J_k^2 = 1 at large z (scipy's jv drifts ~1e-13 there)."""
    from quantumsimulations_amd.engine import bessel_native
    kmax = int(np.ceil(z + 12 * np.cbrt(z + 1) + 60))
    j, deg = bessel_native(z, kmax, 1e-14)
    assert deg >= 1 and deg <= kmax
    if z <= 250.0:
        ref = ss.jv(np.arange(kmax + 1), z)
        assert np.max(np.abs(j - ref)) < 5e-14
        if z > 0:
            assert np.all(np.abs(ref[deg + 1:]) <= 1e-14)
    else:
        mpmath = pytest.importorskip("mpmath")
        mpmath.mp.dps = 30
        for k in (0, 1, 7, 207):
            assert abs(j[k] - float(mpmath.besselj(k, z))) < 1e-15
        assert abs(j[0] ** 2 + 2 * np.sum(j[1:] ** 2) - 1.0) < 1e-13
        assert np.all(np.abs(j[deg + 1:]) <= 1e-14) and abs(j[deg]) > 1e-14


@pytest.mark.parametrize("z", [5e-324, 5e-303, 1e-100, 1e-60, 1e-57, 0.99e-40, 1e-40, 1e-20, 1e-8])
def test_native_bessel_tiny_arguments(z):
    """A register whose H is a multiple of 1 has spectral half-width 0 (clamped to 1e-300), so z =
    alpha dt ~ 1e-302: Miller's recurrence overflowed to NaN below z ~ 1e-58.  For z <= 1e-8 the
    ascending series' first term (z/2)^k / k! is J_k(z) to a relative z^2 / 4(k + 1) < 2.5e-17.
    Below 1e-40 the library takes that term by a product of k factors (2 roundings each; the
    reference here: a power and a division, 3 more): (2k + 3) eps / 2, plus the smallest subnormal.
    Above, the recurrence: test_native_bessel_accuracy's absolute 5e-14."""
    from math import factorial
    from quantumsimulations_amd.engine import bessel_native
    kmax = 72
    j, deg = bessel_native(z, kmax, 1e-14)
    assert np.all(np.isfinite(j)) and deg == 1
    assert j[0] == 1.0
    for k in (1, 2, 3, 7):
        ref = (z / 2.0) ** k / factorial(k)
        bound = (k + 2) * np.finfo(float).eps * ref + 5e-324 if z < 1e-40 else 5e-14
        assert abs(j[k] - ref) <= bound, (k, j[k], ref)
    assert np.all(j >= 0.0) and np.all(j[8:] < 1e-60)


def test_create_without_device_fails_cleanly():
    lib = _lib_or_skip()
    if lib.dse_device_count() > 0:
        pytest.skip("a device is visible")
    from quantumsimulations_amd.engine import Engine
    with pytest.raises(RuntimeError):
        Engine(0)


# ---------------------------------------------------------------- the propagator algorithm
def chebyshev_host(H, psi0, t, alpha, beta, tol=1e-14):
    """numpy restatement of exactly what dse_evolve does (library coefficients), for CPU checks."""
    from quantumsimulations_amd.engine import bessel_native
    out = [psi0.copy()]
    psi = psi0.copy()
    for m in range(len(t) - 1):
        dt = t[m + 1] - t[m]
        z = alpha * dt
        kmax = int(np.ceil(z + 12 * np.cbrt(z + 1) + 60))
        J, deg = bessel_native(z, kmax, tol)
        ph = np.exp(-1j * beta * dt)
        a = [ph * ((-1j) ** k) * (1.0 if k == 0 else 2.0) * J[k] for k in range(deg + 1)]
        w0 = psi
        w1 = (H @ w0 - beta * w0) / alpha
        acc = a[0] * w0 + a[1] * w1
        for k in range(2, deg + 1):
            w2 = 2.0 * (H @ w1 - beta * w1) / alpha - w0
            acc = acc + a[k] * w2
            w0, w1 = w1, w2
        psi = acc
        out.append(psi.copy())
    return np.array(out)


@pytest.mark.parametrize("variant", VARIANTS)
def test_chebyshev_algorithm_matches_exact_n7(golden, variant):
    tr = golden("traces_n7.npz")
    p = sweep_point_params(6, 50000.0, variant, 2e-3, 201)
    prob = pb.build_problem(p, order="engine", reduce=True)
    H = problem_to_csr(prob)
    lo, hi = pb.spectral_bounds(prob)
    psi0 = np.zeros(1 << prob.n_qubits, dtype=complex)
    psi0[prob.psi0_index] = 1.0
    t = tr["t"]
    states = chebyshev_host(H, psi0, t, 0.5 * (hi - lo), 0.5 * (hi + lo))
    got = np.array([rm.observables_bitwise(s, prob.n_qubits, prob.sea_mask, prob.rare_bit,
                                           prob.rare_z_const) for s in states])
    for j, k in enumerate(rm.OBS_ORDER):
        np.testing.assert_allclose(got[:, j], tr[f"{variant}_exact_{k}"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got[:, 6], 1.0, atol=1e-12)


def _wht_plan(n_local, shard_bits, wl, max_bits=0):
    import ctypes as C
    lib = _lib_or_skip()
    buf = (C.c_int32 * 56)()
    G = lib.dse_wht_plan(n_local, shard_bits, wl, max_bits, buf)
    return G, [(buf[g * 14], list(buf[g * 14 + 1:g * 14 + 1 + wl])) for g in range(max(G, 0))]


@pytest.mark.parametrize("wl", [12, 13])
@pytest.mark.parametrize("shard_bits,mid_inpage", [(0, 0), (1, 0), (2, 0), (3, 0), (0, 2), (0, 4)])
def test_wht_pass_plans_transform_every_bit_once(wl, shard_bits, mid_inpage):
    """Walsh-Hadamard pass plans (csrc/dse_runtime.hip wht_layout): group 0 is the low tile; every
    local bit is transformed once (the MID group's top-S positions carry the arriving shard bits,
    so the top S local bits must leave through an earlier group); carried bits are the lowest ones
    and groups respect the size limit.  mid_inpage (option wht_mid_inpage, passed in max_bits'
    second byte): the MID group holds that many high bits below the 2-MiB page (local bit 17)
    when there are that many, the group sizes unchanged."""
    for n_local in range(wl + 1, 35 - shard_bits):
        for max_bits in (0, 2, 4, 7, 11):
            G, groups = _wht_plan(n_local, shard_bits, wl, max_bits | mid_inpage << 8)
            if mid_inpage and G >= 3:
                G0, groups0 = _wht_plan(n_local, shard_bits, wl, max_bits)
                assert sorted(wl - c for c, _ in groups) == sorted(wl - c for c, _ in groups0)
                c, pos = groups[-1]
                inpage = [b for b in range(wl, min(17, n_local))]
                m = min(mid_inpage, len(inpage), wl - c)
                if n_local - 17 >= wl - c - m:
                    assert sum(1 for b in pos[c:] if b < 17) == m, (n_local, max_bits, groups)
            mb = min(max_bits or wl - 2, wl - 2)
            h = n_local - wl
            if shard_bits == 0:
                expect = -(-h // mb) + 1
            elif h < shard_bits or mb <= shard_bits:
                expect = 0
            else:
                m = min(mb - shard_bits, h - shard_bits)
                expect = -(-(h - m) // mb) + 2
            assert G == (expect if expect <= 4 else 0)
            if G == 0:  # the engine cannot take it (the step kernels do)
                continue
            assert 2 <= G <= 4
            c0, pos0 = groups[0]
            assert c0 == 0 and pos0 == list(range(wl))
            seen = list(range(wl))
            for c, pos in groups[1:]:
                assert 1 <= wl - c <= mb
                assert pos[:c] == list(range(c))
                seen += pos[c:]
            top = list(range(n_local - shard_bits, n_local))
            if shard_bits == 0:
                assert sorted(seen) == list(range(n_local))
            else:
                pre = [b for c, pos in groups[1:-1] for b in pos[c:]]
                mid = groups[-1][1][groups[-1][0]:]
                assert set(top) <= set(pre) and set(top) <= set(mid)
                # every local bit once before the swap or in MID (T positions count twice: they
                # are the leaving local bits before and the arriving shard bits in MID)
                assert sorted(pre + [b for b in mid if b not in top]) == list(range(wl, n_local))


def test_run_reference_launcher_resolves_the_drop_in(tmp_path):
    """An unmodified caller placed next to a (QuTiP-importing) dipolar_ensemble_with_rare.py, as the
    reference's sweep_sea_detuning.py is, picks up the MI355X drop-in under the launcher."""
    import subprocess
    import sys
    (tmp_path / "dipolar_ensemble_with_rare.py").write_text("import qutip  # the reference's module\n")
    (tmp_path / "caller.py").write_text(
        "from dipolar_ensemble_with_rare import DipolarRareParams, simulate_rare, "
        "get_derived_frequencies, shell_positions_with_rare_center, dipolar_couplings_from_positions\n"
        "import dipolar_ensemble_with_rare as m, sys\nprint(m.simulate_rare.__module__, sys.argv[1:])\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-m", "quantumsimulations_amd.run_reference",
                          str(tmp_path / "caller.py"), "--x", "1"], cwd=root, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split()[0] == "quantumsimulations_amd.dipolar_ensemble_with_rare"
    assert "'--x', '1'" in res.stdout


def test_evolve_groups_split_by_engine_class():
    """A batch mixing tile-sized (N <= 14) and larger registers is split so the tile-sized ones
    keep the persistent interval kernel (one larger register would demote the whole evolve)."""
    from types import SimpleNamespace

    from quantumsimulations_amd.engine import engine_class, evolve_groups

    probs = [SimpleNamespace(n_qubits=n) for n in (7, 14, 16, 13, 30, 14)]
    keys = [(1e-3, 101)] * 5 + [(2e-3, 101)]
    assert [engine_class(p) for p in probs] == [0, 0, 1, 0, 1, 0]
    g = evolve_groups(keys, probs)
    assert g == {(1e-3, 101, 0): [0, 1, 3], (1e-3, 101, 1): [2, 4], (2e-3, 101, 0): [5]}


def test_root_drop_in_shims_import():
    """The repository-root module names the reference's scripts import (`import
    sweep_sea_detuning`, `from dipolar_ensemble_with_rare import ...`) resolve, with every name
    the shims re-export (reference sweep_sea_detuning.py:324 `_safe_normalized_difference`)."""
    import importlib
    import math
    import sys
    sys.path.insert(0, str(ROOT))
    try:
        for name in ("sweep_sea_detuning", "dipolar_ensemble_with_rare"):
            sys.modules.pop(name, None)
            importlib.import_module(name)
        import sweep_sea_detuning as ssd
        assert ssd._safe_normalized_difference(1.0, 2.0) == 0.5
        assert math.isnan(ssd._safe_normalized_difference(1.0, 0.0))
        assert math.isnan(ssd._safe_normalized_difference(1.0, float("nan")))
    finally:
        sys.path.remove(str(ROOT))
