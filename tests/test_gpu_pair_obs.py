"""Two-spin correlators of every pair of register bits (option "pair_obs", dse_pair_observables,
dse_get_pair_obs) on every engine.

Reference for a state psi (pair_ref, tests/test_pair_obs_host.py): for bits i < j and
y = x ^ e_i ^ e_j, ZZ = sum |psi_x|^2 s_i s_j, ZQ = sum_{bit_i=0, bit_j=1} conj(psi_x) psi_y,
DQ = sum_{bit_i=0, bit_j=0} conj(psi_x) psi_y, all divided by ||psi||^2.

Tolerances are the project's (test_gpu_parity.py, test_gpu_site_obs.py): abs 1e-12 for a hook on a
given state, 1e-10 for traces against an exact propagation, 1e-11 between two exact propagators of
the engine; an energy is compared within that bound times W, the sum of the coefficients' sizes
(energy_weight).  Problems, grids and exact states are those of test_gpu_site_obs.py (its module
caches are shared), so no exact propagation is repeated.
"""
import numpy as np
import pytest

from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.sweep import VARIANTS, sweep_point_params
from test_gpu_parity import _rand, _random_problem
from test_gpu_site_obs import DEFAULTS as SITE_DEFAULTS, T7, _imag_problem, _p10, _p12, eigh_states, expm_states
from test_pair_obs_host import energy_weight, numpy_energy, pair_ref

pytestmark = pytest.mark.gpu

DEFAULTS = dict(SITE_DEFAULTS, pair_obs=0)


def pair_ref_traces(states, n):
    return np.stack([pair_ref(s, n) for s in states], axis=-1)  # (5, NP, n_t)


def _run(engine, probs, t, pairs=1, sites=0, **opts):
    """evolve with the given options (restored afterwards); obs, stats, pair traces per problem, site
    traces per problem (None with the option off)."""
    engine.clear()
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        engine.set_option("pair_obs", pairs)
        engine.set_option("site_obs", sites)
        for p in probs:
            engine.add(p)
        obs, st = engine.evolve(t)
        n_pair = engine.pair_obs_problems()
        tr = [engine.pair_traces(i) for i in range(len(probs))] if pairs else None
        sr = [engine.site_traces(i) for i in range(len(probs))] if sites else None
    finally:
        for k in list(opts) + ["pair_obs", "site_obs"]:
            engine.set_option(k, DEFAULTS[k])
        engine.clear()
    st = dict(st, pair_obs_problems=n_pair)
    return obs, st, tr, sr


def _check_traces(tr, ref, bound=1e-10):
    assert tr.shape == ref.shape
    err = float(np.max(np.abs(tr - ref)))
    print(f"max |pair traces - reference| = {err:.3e} (bound {bound:g})")
    assert err < bound, err


# ------------------------------------------------------------------------------ 1. the hook
@pytest.mark.parametrize("n,tile_bits", [(3, 12), (9, 6), (13, 13), (15, 12), (16, 13), (17, 9)])
def test_hook_matches_numpy(engine, n, tile_bits):
    """Tiles smaller than the workgroup, both bits register bits, register x thread, thread x thread,
    one bit above the tile, both above the tile ((17, 9): 28 such pairs)."""
    prob = _random_problem(n, 7 + n, rare_bit=n - 2)
    v = _rand(n, 3 * n) * 1.7
    engine.clear()
    engine.set_option("tile_bits", tile_bits)
    try:
        pid = engine.add(prob)
        got = engine.pair_observables(pid, v)
        sites = engine.site_observables(pid, v)
    finally:
        engine.set_option("tile_bits", 13)
        engine.clear()
    assert got.shape == (5, n * (n - 1) // 2)
    err = float(np.max(np.abs(got - pair_ref(v, n))))
    print(f"n = {n}, tile_bits = {tile_bits}: max |hook - numpy| = {err:.3e} (bound 1e-12)")
    assert err < 1e-12
    W = energy_weight(prob)
    e_err = abs(float(pb.energy_partition(prob, sites, got)["total"]) - numpy_energy(prob, v))
    print(f"|energy partition - <H>| = {e_err:.3e} (bound {1e-12 * W:.3e})")
    assert e_err <= 1e-12 * W


# ------------------------------------------------------------------------------ 2. loopback shards
@pytest.mark.parametrize("n,bits,tile", [(10, 1, 6), (12, 2, 8), (13, 3, 10)])
def test_hook_sharded_matches_unsharded(engine, n, bits, tile):
    prob = _random_problem(n, 900 + 10 * n + bits, rare_bit=n - 1)
    rng = np.random.default_rng(n * 7 + bits)
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    engine.set_option("tile_bits", tile)
    try:
        engine.clear()
        ref = engine.pair_observables(engine.add(prob), v)
        engine.clear()
        ps = engine.add_sharded(prob, bits)
        got = engine.pair_observables(ps, v)
        with pytest.raises(ValueError):  # another shard's id
            engine.pair_observables(ps + 1, v[: 1 << (n - bits)])
    finally:
        engine.clear()
        engine.set_option("tile_bits", 13)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got, pair_ref(v, n), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------ 3. evolve, per engine
@pytest.mark.parametrize("reduce", [True, False])
def test_small_engine(engine, reduce):
    """N = 7 (and 6 for the reduced center_off register), two launches of the engine (small_chunk 4 < 6
    intervals)."""
    probs = [pb.build_problem(sweep_point_params(6, 50e3, v, 1e-3, 9), order="engine", reduce=reduce)
             for v in VARIANTS]
    obs, st, tr, _ = _run(engine, probs, T7, dense=0, small_chunk=4)
    assert st["mode"] == 3 and st["pair_obs_problems"] == 3
    for i, p in enumerate(probs):
        _check_traces(tr[i], pair_ref_traces(eigh_states(("n7", i, reduce), p, T7), p.n_qubits))


def test_streaming_n12(engine):
    p = _p12()
    obs, st, tr, _ = _run(engine, [p], T7, persistent=0, wht=0, tile_bits=9, dense=0)
    assert st["mode"] == 0 and st["dense_problems"] == 0
    _check_traces(tr[0], pair_ref_traces(eigh_states("n12", p, T7), 12))


def test_walsh_hadamard_n15_default_options(engine):
    """Every Walsh-Hadamard option at its default, 3 outputs; reference at this size: the wht = 0
    streaming run (two exact propagators, 1e-11), as in test_gpu_site_obs.py."""
    p = _random_problem(15, 515, rare_bit=14)
    t = np.linspace(0.0, 1e-3, 3)
    obs, st, tr, _ = _run(engine, [p], t, span_tile=0)
    assert st["mode"] == 2 and st["span_problems"] == 0
    obs0, st0, tr0, _ = _run(engine, [p], t, wht=0, span_tile=0)
    assert st0["mode"] == 0
    _check_traces(tr[0], tr0[0], 1e-11)


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("n_t", [6, 7])
@pytest.mark.parametrize("n", [13, 14])
def test_interval_kernel(engine, n, n_t, overlap):
    """k_interval, two outputs per launch: an odd and an even number of intervals (the intermediate
    output buffer and the state buffer), observables overlapped or not."""
    p = _random_problem(n, 500 + n, rare_bit=n - 1)
    t = T7[:n_t]
    obs, st, tr, _ = _run(engine, [p], t, tile_bits=13, outputs_per_launch=2, obs_overlap=overlap, span_tile=0,
                          matrix=0, dense=0)
    assert st["mode"] == 1 and st["outputs_per_launch"] == 2 and st["span_problems"] == 0
    _check_traces(tr[0], pair_ref_traces(expm_states(f"r{n}", p, T7)[:n_t], n))


def test_span_kernel(engine):
    t = np.linspace(0.0, 1e-3, 6)
    p = _p12()
    obs, st, tr, _ = _run(engine, [p], t, span_tile=10, span_outputs=4, matrix=0, dense=0)
    assert st["mode"] == 1 and st["span_problems"] == 1
    _check_traces(tr[0], pair_ref_traces(eigh_states("n12", p, t), 12))


def test_real_kernel_n13(engine):
    p = _imag_problem(13, 613)
    obs, st, tr, _ = _run(engine, [p], T7, real=1, span_tile=0, matrix=0, dense=0)
    assert st["mode"] == 1 and st["real_problems"] == 1
    _check_traces(tr[0], pair_ref_traces(expm_states("i13", p, T7), 13))


@pytest.mark.parametrize("nufft", [0, 2])
def test_dense_engine_n7(engine, nufft):
    """The rotated frame's factor -1 on DQ, strided real / imaginary columns and the non-uniform FFT's
    interleaved blocks."""
    probs = [pb.build_problem(sweep_point_params(6, 50e3, v, 1e-3, 9), order="engine", reduce=True)
             for v in VARIANTS]
    obs, st, tr, _ = _run(engine, probs, T7, dense=2, dense_nufft=nufft)
    assert st["dense_problems"] == 3 and st["mode"] == 4
    assert st["dense_nufft_problems"] == (3 if nufft else 0)
    for i, p in enumerate(probs):
        _check_traces(tr[i], pair_ref_traces(eigh_states(("n7", i, True), p, T7), p.n_qubits))


def test_dense_engine_one_register_of_1024(engine):
    p = _p10()
    obs, st, tr, _ = _run(engine, [p], T7, dense=2)
    assert st["dense_problems"] == 1
    _check_traces(tr[0], pair_ref_traces(eigh_states("n10", p, T7), 10))


def test_matrix_mode(engine):
    p = _p10()
    t = np.linspace(0.0, 1e-3, 17)
    obs, st, tr, _ = _run(engine, [p], t, matrix=2, dense=0)
    assert st["mode"] == 5
    _check_traces(tr[0], pair_ref_traces(eigh_states("n10", p, t), 10))


# ------------------------------------------------------------------------------ 4. energy along a run
def test_energy_partition_is_conserved_along_a_streaming_run(engine):
    """Unitary evolution conserves <H>: at every output the partition's total is the same within
    1e-10 W, and at the last output it is what dse_energy computes from the final state with the H
    kernels (the observable kernels against the H kernels)."""
    p = _p12()
    W = energy_weight(p)
    engine.clear()
    try:
        for k, v in dict(persistent=0, wht=0, tile_bits=9, dense=0, pair_obs=1, site_obs=1).items():
            engine.set_option(k, v)
        pid = engine.add(p)
        engine.evolve(T7)
        part = pb.energy_partition(p, engine.site_traces(pid), engine.pair_traces(pid))
        e_final = engine.energy(pid)[0]
    finally:
        for k in ("persistent", "wht", "tile_bits", "dense", "pair_obs", "site_obs"):
            engine.set_option(k, DEFAULTS[k])
        engine.clear()
    total = part["total"]
    assert total.shape == (7,)
    drift = float(np.max(np.abs(total - total[0])))
    print(f"E = {total[0]:.6e}, W = {W:.3e}: max drift {drift:.3e}, |total - dse_energy| = "
          f"{abs(total[-1] - e_final):.3e} (bound {1e-10 * W:.3e})")
    assert drift <= 1e-10 * W
    assert abs(total[-1] - e_final) <= 1e-10 * W
    assert abs(total[0] - numpy_energy(p, eigh_states("n12", p, T7)[0])) <= 1e-10 * W


# ------------------------------------------------------------------------------ 5. bitwise
@pytest.mark.parametrize("case", ["n7", "n13", "n14", "dense"])
def test_other_results_bitwise_unchanged_and_pairs_repeatable(engine, case):
    if case in ("n7", "dense"):
        probs = [pb.build_problem(sweep_point_params(6, 50e3, v, 1e-3, 7)) for v in VARIANTS]
    else:
        probs = [pb.build_problem(sweep_point_params(13, d, "center_off" if case == "n13" else "center_on", 2e-5, 7))
                 for d in (0.0, 150e3)]
        assert probs[0].n_qubits == int(case[1:])
    t = T7 if case in ("n7", "dense") else np.linspace(0.0, 2e-5, 7)
    opts = {"dense": 2} if case == "dense" else {}
    off, st_off, _, _ = _run(engine, probs, t, pairs=0, **opts)
    on, st_on, tr, _ = _run(engine, probs, t, pairs=1, **opts)
    on2, _, tr2, _ = _run(engine, probs, t, pairs=1, **opts)
    assert np.array_equal(on, off) and np.array_equal(on2, off)
    for a, b in zip(tr, tr2):
        assert np.array_equal(a, b)
    s_off, _, _, sr_off = _run(engine, probs, t, pairs=0, sites=1, **opts)
    s_on, st_both, tr3, sr_on = _run(engine, probs, t, pairs=1, sites=1, **opts)
    assert np.array_equal(s_off, off) and np.array_equal(s_on, off)
    for a, b in zip(sr_on, sr_off):
        assert np.array_equal(a, b)
    for a, b in zip(tr3, tr):
        assert np.array_equal(a, b)
    # the option does not choose the engine
    for k in ("mode", "dense_problems", "span_problems", "real_problems", "outputs_per_launch", "tile_bits"):
        assert st_on[k] == st_off[k] == st_both[k], k
    assert st_off["pair_obs_problems"] == 0 and st_on["pair_obs_problems"] == len(probs)


# ------------------------------------------------------------------------------ 6. mixed context
def test_mixed_context_matches_lone_registers(engine):
    """A dense register, a small one and 1- and 2-tile k_interval registers in one context: each
    one's traces as from a context of its own (arena offsets, strides of the widest register)."""
    dense_p = pb.build_problem(sweep_point_params(6, 75e3, "center_on", 1e-3, 7))
    probs = [dense_p] + [_random_problem(n, 700 + n, rare_bit=n - 1) for n in (7, 12, 14)]  # complex drives: not dense
    opts = dict(dense=2, span_tile=0, matrix=0)
    obs, st, tr, _ = _run(engine, probs, T7, **opts)
    assert st["pair_obs_problems"] == 4 and st["dense_problems"] == 1
    for i, p in enumerate(probs):
        obs1, st1, tr1, _ = _run(engine, [p], T7, **opts)
        assert st1["dense_problems"] == (1 if i == 0 else 0)
        np.testing.assert_allclose(tr[i], tr1[0], rtol=0, atol=1e-11)


@pytest.mark.parametrize("case", ["mixed", "matrix"])
def test_both_options_on_bitwise_equal_each_alone(engine, case):
    """site_obs and pair_obs together: the aggregates, the site traces and the pair traces are bitwise
    those of the runs with one option on (each family its own stride, arena and slot).  The mixed
    context of test_mixed_context_matches_lone_registers and the register of test_matrix_mode."""
    if case == "mixed":
        dense_p = pb.build_problem(sweep_point_params(6, 75e3, "center_on", 1e-3, 7))
        probs = [dense_p] + [_random_problem(n, 700 + n, rare_bit=n - 1) for n in (7, 12, 14)]
        t, opts = T7, dict(dense=2, span_tile=0, matrix=0)
    else:
        probs, t, opts = [_p10()], np.linspace(0.0, 1e-3, 17), dict(matrix=2, dense=0)
    obs_p, st_p, tr_p, _ = _run(engine, probs, t, pairs=1, sites=0, **opts)
    obs_s, st_s, _, sr_s = _run(engine, probs, t, pairs=0, sites=1, **opts)
    obs_b, st_b, tr_b, sr_b = _run(engine, probs, t, pairs=1, sites=1, **opts)
    if case == "mixed":
        assert st_b["dense_problems"] == 1
    else:
        assert st_b["mode"] == 5
    for k in ("mode", "dense_problems", "span_problems", "real_problems", "outputs_per_launch", "tile_bits"):
        assert st_p[k] == st_s[k] == st_b[k], k
    assert st_b["pair_obs_problems"] == len(probs) and st_b["site_obs_problems"] == len(probs)
    assert np.array_equal(obs_b, obs_p) and np.array_equal(obs_b, obs_s)
    for i, p in enumerate(probs):
        n = p.n_qubits
        assert tr_b[i].shape == (5, n * (n - 1) // 2, len(t)) and sr_b[i].shape == (3, n, len(t))
        assert np.array_equal(tr_b[i], tr_p[i]), i
        assert np.array_equal(sr_b[i], sr_s[i]), i


# ------------------------------------------------------------------------------ 7. hand-off timeout
def test_rerun_after_handoff_timeout_overwrites(engine):
    """spin_limit = -1 fails every hand-off of the 2-tile register: the evolve re-runs on the
    streaming kernels.  Its pair traces are the re-run's; the dense register's are kept from the
    first pass like its aggregates."""
    dense_p = pb.build_problem(sweep_point_params(6, 75e3, "center_on", 1e-3, 7))
    cheb_p = _random_problem(14, 514, rare_bit=13)
    opts = dict(dense=2, span_tile=0)
    obs, st, tr, _ = _run(engine, [dense_p, cheb_p], T7, **opts)
    assert st["dense_problems"] == 1 and st["handoff_fallbacks"] == 0 and st["mode"] == 1
    obs2, st2, tr2, _ = _run(engine, [dense_p, cheb_p], T7, spin_limit=-1, **opts)
    assert st2["dense_problems"] == 1 and st2["handoff_fallbacks"] >= 1 and st2["pair_obs_problems"] == 2
    assert tr2[0].shape == tr[0].shape and tr2[1].shape == (5, 91, 7)
    assert np.array_equal(tr2[0], tr[0])
    np.testing.assert_allclose(tr2[1], tr[1], rtol=0, atol=1e-11)
    obs3, st3, tr3, _ = _run(engine, [cheb_p], T7, persistent=0, wht=0, dense=0)
    assert st3["mode"] == 0
    np.testing.assert_allclose(tr2[1], tr3[0], rtol=0, atol=1e-11)  # the streaming run


# ------------------------------------------------------------------------------ 8. errors, lifetime
def test_errors(engine):
    p = _random_problem(10, 33, rare_bit=9)
    engine.clear()
    try:
        pid = engine.add(p)
        assert engine.pair_obs_problems() == 0
        with pytest.raises(RuntimeError):      # before any evolve
            engine.pair_traces(pid)
        engine.evolve(T7)
        with pytest.raises(RuntimeError):      # after an evolve with the option off
            engine.pair_traces(pid)
        assert engine.pair_obs_problems() == 0
        with pytest.raises(ValueError):
            engine.set_option("pair_obs", 2)
        with pytest.raises(ValueError):        # bad problem ids
            engine.pair_traces(pid + 1)
        v = _rand(10, 30)
        out = np.empty((5, 45))
        from quantumsimulations_amd import _lib
        assert engine._L.dse_pair_observables(engine._h, 5, _lib.ptr(v), _lib.ptr(out)) == _lib.DSE_ERR_ARG
        assert engine._L.dse_get_pair_obs(engine._h, -1, _lib.ptr(out)) == _lib.DSE_ERR_ARG
        engine.clear()
        engine.set_option("tile_bits", 8)
        ps = engine.add_sharded(p, 1)
        engine.set_option("pair_obs", 1)
        engine.evolve(T7)
        assert engine.pair_obs_problems() == 1  # a loopback group counts once
        whole = engine.pair_traces(ps)
        assert whole.shape == (5, 45, 7)
        with pytest.raises(ValueError):        # a non-zero shard id of a loopback group
            engine.pair_traces(ps + 1)
        engine.clear()
        engine.set_option("pair_obs", 0)
        engine.set_option("tile_bits", 13)
        _, _, tr, _ = _run(engine, [p], T7, tile_bits=8)
        np.testing.assert_allclose(whole, tr[0], rtol=0, atol=1e-11)
    finally:
        engine.set_option("pair_obs", 0)
        engine.set_option("tile_bits", 13)
        engine.clear()


def test_failed_evolve_invalidates_earlier_traces(engine):
    p = _random_problem(10, 34, rare_bit=9)
    engine.clear()
    try:
        pid = engine.add(p)
        engine.set_option("pair_obs", 1)
        engine.evolve(T7)
        assert engine.pair_traces(pid).shape == (5, 45, 7) and engine.pair_obs_problems() == 1
        with pytest.raises(ValueError):
            engine.evolve(np.array([0.0, 1e-4, 1e-4]))
        with pytest.raises(RuntimeError):
            engine.pair_traces(pid)
        assert engine.pair_obs_problems() == 0
        engine.evolve(T7[:5])
        assert engine.pair_traces(pid).shape == (5, 45, 5)
        with pytest.raises(ValueError):
            engine.evolve(T7, tol=1.0)
        with pytest.raises(RuntimeError):
            engine.pair_traces(pid)
        assert engine.evolve(T7)[0].shape == (1, 7, 7)
        assert engine.pair_traces(pid).shape == (5, 45, 7)
    finally:
        engine.set_option("pair_obs", 0)
        engine.clear()


# ------------------------------------------------------------------------------ 9. Python surface
@pytest.mark.parametrize("variant", VARIANTS)
def test_simulate_rare_pairs(variant):
    from quantumsimulations_amd.dipolar_ensemble_with_rare import (_engine, simulate_rare, simulate_rare_pairs,
                                                                   simulate_rare_sites)
    params = sweep_point_params(6, 50e3, variant, 1e-3, 9)
    t, obs, sites, pairs = simulate_rare_pairs(params)
    t0, obs0, sites0 = simulate_rare_sites(params)
    np.testing.assert_array_equal(t, t0)
    for k in obs0:
        assert np.array_equal(obs[k], obs0[k]), k
    for k in sites0:
        assert np.array_equal(sites[k], sites0[k]), k
    assert list(pairs) == ["zz", "zq", "dq"]
    zz, zq, dq = pairs["zz"], pairs["zq"], pairs["dq"]
    for a in (zz, zq, dq):
        assert a.shape == (7, 7, 9)
    assert zz.dtype == np.float64 and zq.dtype == np.complex128 and dq.dtype == np.complex128
    assert np.array_equal(zz, np.swapaxes(zz, 0, 1)) and np.array_equal(dq, np.swapaxes(dq, 0, 1))
    assert np.array_equal(zq, np.conj(np.swapaxes(zq, 0, 1)))
    for k in range(7):
        assert np.all(zz[k, k] == 0.25) and np.all(dq[k, k] == 0.0)
        assert np.array_equal(zq[k, k], 0.5 + sites["Iz"][k])
    prob = pb.build_problem(params, order="engine", reduce=True)
    if prob.reduced:
        assert variant == "center_off"
        for k in range(6):
            assert np.array_equal(zz[k, 6], prob.rare_z_const * sites["Iz"][k])
            assert np.all(zq[k, 6] == 0.0) and np.all(dq[k, 6] == 0.0)
    # sum_{k != l} <Iz_k Iz_l> over the sea sites = <(sum_k Iz_k)^2> - n_sea / 4 of the exact state
    i = list(VARIANTS).index(variant)
    states = eigh_states(("n7", i, True), prob, t)
    sea_bits = [b for b in range(prob.n_qubits) if (prob.sea_mask >> b) & 1]
    sea_sites = [int(prob.site_of_bit[b]) for b in sea_bits]
    x = np.arange(1 << prob.n_qubits)
    sz = sum(0.5 - ((x >> b) & 1) for b in sea_bits)
    want = np.array([(np.abs(s) ** 2 * sz ** 2).sum() / (np.abs(s) ** 2).sum() for s in states]) - len(sea_bits) / 4.0
    sub = zz[np.ix_(sea_sites, sea_sites)]
    got = sub.sum(axis=(0, 1)) - np.trace(sub, axis1=0, axis2=1)
    err = float(np.max(np.abs(got - want)))
    print(f"{variant}: |sum_(k != l) zz - (<Sz^2> - n_sea / 4)| = {err:.3e} (bound 1e-10)")
    assert err < 1e-10
    # the cached engine has both options back at 0
    eng = _engine(0)
    eng.clear()
    try:
        pid = eng.add(prob)
        eng.evolve(t)
        with pytest.raises(RuntimeError):
            eng.pair_traces(pid)
        with pytest.raises(RuntimeError):
            eng.site_traces(pid)
    finally:
        eng.clear()
