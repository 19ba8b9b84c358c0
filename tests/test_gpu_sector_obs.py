"""Magnetisation-sector populations P_j = sum_{x : (x & cm) == cv, popcount(x & m) == j} |psi_x|^2 / <psi|psi>
(dse_set_sectors, dse_sector_values, dse_get_sectors; feature "sector_obs") on every engine.

The reference is numpy: np.bincount(popcount(x & m)[sel], |psi|^2[sel]) / ||psi||^2 (sector_ref).  States
come from the exact propagations of test_gpu_site_obs.py / test_gpu_overlap_obs.py (numpy eigh up to 12
qubits, scipy expm_multiply at 13 and 14), shared with the other observable tests.

Tolerances are the project's: abs 1e-12 for a hook on a given state, 1e-10 for traces against an exact
propagation and for a conserved quantity over the outputs, 1e-11 between two exact propagators of the
engine, bitwise where the same kernel runs the same data.  Every value is in [0, 1], so the bounds are
absolute.  The measured maxima are printed (-s).

The hook cases: a selection's bits are taken out of the counted mask (m & cm == 0 is the contract), so
"all bits" with a selection counts every other bit.  A selection that NO tile satisfies in its high part
does not exist for masks the library accepts (cv within cm names one value of the high bits, and the
tile with that index has it); the nearest case is here instead: a selection on every bit above the tile,
which one tile alone meets and every other tile answers with zeros.

Every evolve case carries evolve_sets(n): all bits counted; the low half counted with the top bit selected
down; no counted bit (one bin: the selection's probability); the bits above the middle counted with bit 0
selected up and bit 1 down.

Measured on an MI355X (worst per section): hook against numpy 1.2e-14 (K = 1 against K = 16: bitwise),
loopback shards 6.1e-16 (against unsharded: bitwise), mean / second moment against site_obs / pair_obs
8.9e-16 / 4.4e-16, bins against Ea / Eb strings 1.1e-16, conserved quantities 3.4e-15, traces against the
exact propagation 6.9e-13 (matrix mode; dense 3.9e-13, small engine 2.5e-13, tile engines 5.0e-14), between two propagators 5.6e-17, mixed
context 0, re-run 6.9e-16, simulate_rare_sectors 1.6e-13, mqc_intensities 3.6e-14.
"""
import dataclasses

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.sweep import VARIANTS, sweep_point_params
from test_gpu_op_strings import A_, B_, codes_of, evolve_set, string_ref
from test_gpu_overlap_obs import DEFAULTS, T9, IV_OPTS, _n7, basis_state, eigh_from, expm_from, make_refs
from test_gpu_parity import _rand, _random_problem
from test_gpu_site_obs import T7, _imag_problem, _p10, _p12, eigh_states, expm_states

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ the numpy reference
def popcount(x):
    x = np.asarray(x, dtype=np.uint64)
    out = np.zeros(x.shape, dtype=np.int64)
    for b in range(40):
        out += ((x >> np.uint64(b)) & np.uint64(1)).astype(np.int64)
    return out


def sector_ref(masks, states):
    """A list of (B_k, n_t) arrays: the bins of every set on every state, by bincount."""
    masks = np.asarray(masks, dtype=np.uint64).reshape(-1, 3)
    dim = len(states[0])
    x = np.arange(dim, dtype=np.uint64)
    out = []
    for m, cm, cv in masks:
        sel = (x & cm) == cv
        w = popcount(x & m)[sel]
        B = int(popcount(m)) + 1
        cols = []
        for psi in states:
            p2 = np.abs(np.asarray(psi, dtype=np.complex128)) ** 2
            cols.append(np.bincount(w, p2[sel], minlength=B) / p2.sum())
        out.append(np.stack(cols, axis=1))
    return out


def flat(parts):
    return np.concatenate([np.asarray(p).reshape(p.shape[0], -1) for p in parts], axis=0)


def evolve_sets(n):
    """Four sets for the evolve cases (n >= 5): m, cm, cv by register bit."""
    allb, h, top = (1 << n) - 1, n // 2, 1 << (n - 1)
    return np.array([
        [allb, 0, 0],
        [(1 << h) - 1, top, top],
        [0, top | 1, 1],
        [allb & ~((1 << h) - 1), 3, 2],
    ], dtype=np.uint64)


def _check(got, ref, bound, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64, (got.shape, ref.shape)
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max |value - reference| = {err:.3e} (bound {bound:g})")
    assert err < bound, err
    return err


def _run(engine, probs, t, secs, inits=None, sites=0, pairs=0, refs=None, strs=None, **opts):
    """One evolve with the given options (restored afterwards): secs[i] (K, 3) masks or None per
    problem.  Returns obs, stats and a dict of per-problem lists."""
    engine.clear()
    out = {"sec": [], "state": [], "sites": [], "pairs": [], "ov": [], "str": []}
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        engine.set_option("site_obs", sites)
        engine.set_option("pair_obs", pairs)
        for i, p in enumerate(probs):
            pid = engine.add(p)
            if inits is not None and inits[i] is not None:
                engine.set_initial_state(pid, inits[i])
            if refs is not None:
                engine.set_overlap_refs(pid, refs[i])
            if strs is not None:
                engine.set_op_strings(pid, strs[i])
            if secs is not None and secs[i] is not None:
                engine.set_sectors(pid, secs[i])
        obs, st = engine.evolve(t)
        out["problems"] = engine.sector_problems()
        for i in range(len(probs)):
            has = secs is not None and secs[i] is not None
            out["sec"].append(flat(engine.sector_traces(i)) if has else None)
            out["state"].append(engine.state(i))
            out["sites"].append(engine.site_traces(i) if sites else None)
            out["pairs"].append(engine.pair_traces(i) if pairs else None)
            out["ov"].append(engine.overlap_traces(i) if refs is not None else None)
            out["str"].append(engine.op_string_traces(i) if strs is not None else None)
    finally:
        for k in list(opts) + ["site_obs", "pair_obs"]:
            engine.set_option(k, DEFAULTS[k])
        engine.clear()
    return obs, st, out


def _engine_case(engine, prob, t, opts, stats_ok, states=None, other_opts=None, init=None):
    """One register on one engine: the traces of evolve_sets(n) against the exact states (1e-10) or
    against another exact propagator of the engine (other_opts, 1e-11); the values at t0 against numpy
    on the initial state (1e-12); the all-bits set sums to 1."""
    n = prob.n_qubits
    S = evolve_sets(n)
    inits = None if init is None else [init]
    obs, st, r = _run(engine, [prob], t, [S], inits, **opts)
    stats_ok(st)
    assert r["problems"] == 1
    tr = r["sec"][0]
    U, off = _lib.sector_layout(n, S)
    assert tr.shape == (U, len(t)) and U == (n + 1) + (n // 2 + 1) + 1 + (n - n // 2 + 1)
    if states is not None:
        _check(tr, flat(sector_ref(S, states)), 1e-10, "against the exact propagation")
    else:
        _, st0, r0 = _run(engine, [prob], t, [S], inits, **other_opts)
        assert st0["mode"] == 0
        _check(tr, r0["sec"][0], 1e-11, "against the engine's streaming propagator")
    psi0 = basis_state(prob) if init is None else init
    _check(tr[:, :1], flat(sector_ref(S, [psi0])), 1e-12, "values at t0")
    assert np.max(np.abs(tr[:n + 1].sum(axis=0) - 1.0)) < 1e-13  # (the bins and the norm: the same terms in two orders)
    return obs, st, r


# ------------------------------------------------------------------------------ 1. the hook
def _geometry(n, tile_bits):
    L = min(n, tile_bits)
    lgnt = 9 if L >= 13 else (8 if L >= 8 else 6)
    return L, min(L, lgnt)  # tile bits, thread bits (Geo<L>)


def hook_sets(n, tile_bits):
    """(name, m, cm, cv) of item 1: six kinds of counted mask, each alone and with a selection in the
    low part, in the high part and in both; the selecting bits leave the counted mask.  Thread bits are
    0 .. TB - 1, a thread's row bits TB .. L - 1, the bits above the tile L .. n - 1; a geometry without
    row bits or without bits above the tile takes the highest bit below instead."""
    L, TB = _geometry(n, tile_bits)
    allb = (1 << n) - 1
    thr, row, hi = (1 << TB) - 1, ((1 << L) - 1) & ~((1 << TB) - 1), allb & ~((1 << L) - 1)
    top = 1 << (n - 1)
    kinds = [
        ("thread bits", thr),
        ("row bits", row if row else 1 << (L - 1)),
        ("above the tile", hi if hi else top),
        ("across all three", 1 | (1 << min(6, L - 1)) | (1 << (L - 1)) | (1 << min(L, n - 1)) | top),
        ("all bits", allb),
        ("m = 0", 0),
    ]
    lo_cm, lo_cv = 2 | (1 << (L - 1)), 2                      # bit 1 down, the top tile bit up
    hi_cm, hi_cv = (hi if hi else top), (top if hi else 0)    # every bit above the tile: one tile alone meets it
    sels = [("", 0, 0), (", selection low", lo_cm, lo_cv), (", selection high", hi_cm, hi_cv),
            (", selection low and high", lo_cm | hi_cm, lo_cv | hi_cv)]
    return [(k + s, m & ~cm, cm, cv) for k, m in kinds for s, cm, cv in sels]


@pytest.mark.parametrize("n,tile_bits", [(3, 12), (9, 6), (13, 13), (15, 12), (16, 13), (17, 9)])
def test_hook_matches_numpy(engine, n, tile_bits):
    sets = hook_sets(n, tile_bits)
    assert len(sets) == 24
    S = np.array([s[1:] for s in sets], dtype=np.uint64)
    L, _ = _geometry(n, tile_bits)
    if n > L:  # the high selection leaves one tile: all others write zeros
        assert int(S[2][1]) >> L == (1 << (n - L)) - 1
    rng = np.random.default_rng(2000 + n)
    pad = []
    for _ in range(8):  # random valid sets fill the second batch to K = 16
        m = int(rng.integers(0, 1 << n))
        cm = int(rng.integers(0, 1 << n)) & ~m
        pad.append([m, cm, int(rng.integers(0, 1 << n)) & cm])
    batches = [S[:16], np.concatenate([S[16:], np.array(pad, dtype=np.uint64)])]
    prob = _random_problem(n, 7 + n, rare_bit=n - 2)
    v = _rand(n, 3 * n) * 1.7
    engine.clear()
    engine.set_option("tile_bits", tile_bits)
    try:
        pid = engine.add(prob)
        got16 = []
        for Sb in batches:
            engine.set_sectors(pid, Sb)
            assert engine.sectors(pid) == 16 and engine.sector_units(pid) == _lib.sector_layout(n, Sb)[0]
            got16 += engine.sector_values(pid, v)
        ones = []
        for k in range(len(S)):  # K = 1: every set alone
            engine.set_sectors(pid, S[k:k + 1])
            assert engine.sectors(pid) == 1
            ones.append(engine.sector_values(pid, v)[0])
    finally:
        engine.set_option("tile_bits", 13)
        engine.clear()
    ref = sector_ref(np.concatenate(batches), [v])
    worst = 0.0
    for k, (name, m, cm, cv) in enumerate(sets):
        want = ref[k][:, 0]
        assert got16[k].shape == want.shape == ones[k].shape == (bin(m).count("1") + 1,), name
        e16, e1 = np.abs(got16[k] - want).max(), np.abs(ones[k] - want).max()
        print(f"n = {n}, tile {tile_bits}, {name}: weight {want.sum():.3e}, error K = 16: {e16:.2e}, K = 1: {e1:.2e}")
        assert e16 < 1e-12 and e1 < 1e-12, name
        assert np.array_equal(ones[k], got16[k]), name  # the same sums in the same order
        worst = max(worst, e16, e1)
    for k in range(len(S), 32):
        worst = max(worst, _check(got16[k], ref[k][:, 0], 1e-12, f"random set {k}"))
    print(f"hook n = {n}, tile {tile_bits}: worst error {worst:.3e} (bound 1e-12)")


# ------------------------------------------------------------------------------ 2. loopback shards
@pytest.mark.parametrize("n,bits,tile", [(10, 1, 6), (12, 2, 8), (13, 3, 10)])
def test_hook_sharded_matches_unsharded(engine, n, bits, tile):
    """Counted and selecting bits among the shard bits (the top `bits` bits of the register)."""
    prob = _random_problem(n, 900 + 10 * n + bits, rare_bit=n - 1)
    rng = np.random.default_rng(n * 7 + bits)
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    sb = n - bits  # the lowest shard bit
    allb, shard = (1 << n) - 1, ((1 << n) - 1) & ~((1 << sb) - 1)
    S = np.array([
        [allb, 0, 0],
        [shard | 1, 0, 0],                                   # the shard bits and one thread bit counted
        [(1 << sb) - 1, shard, 1 << (n - 1)],                # all shard bits select: one shard's tiles alone
        [allb & ~(1 << sb) & ~2, (1 << sb) | 2, 1 << sb],    # one shard bit selects, the others are counted
        [1 << (n - 1), 1 << (tile - 1), 0],                  # the top shard bit counted alone
        [0, 1 << sb, 0],
    ], dtype=np.uint64)
    engine.set_option("tile_bits", tile)
    try:
        engine.clear()
        pid = engine.add(prob)
        engine.set_sectors(pid, S)
        ref = flat(engine.sector_values(pid, v))
        engine.clear()
        ps = engine.add_sharded(prob, bits)
        engine.set_sectors(ps, S)
        got = flat(engine.sector_values(ps, v))
    finally:
        engine.clear()
        engine.set_option("tile_bits", 13)
    _check(got, ref, 1e-12, "sharded against unsharded")
    _check(got, flat(sector_ref(S, [v])), 1e-12, "sharded against numpy")


# ------------------------------------------------------------------------------ 3. the existing families
@pytest.mark.parametrize("n,tile_bits", [(9, 6), (14, 13)])
def test_moments_agree_with_site_and_pair_observables(engine, n, tile_bits):
    """With M the number of counted spins down, sum_b Iz_b = popcount(m)/2 - M on the counted spins: the
    mean of the all-bits set and of a five-bit set against site_observables, the second moment of the
    all-bits set, sum_M (n/2 - M)^2 P_M, against n/4 + 2 sum_{i<j} <Iz_i Iz_j> from pair_observables
    (1e-12; both options on)."""
    prob = _random_problem(n, 40 + n, rare_bit=n - 1)
    v = _rand(n, 5 * n) * 0.9
    allb = (1 << n) - 1
    sub = 1 | (1 << 3) | (1 << 6) | (1 << (n - 2)) | (1 << (n - 1))
    engine.clear()
    engine.set_option("tile_bits", tile_bits)
    engine.set_option("site_obs", 1)
    engine.set_option("pair_obs", 1)
    try:
        pid = engine.add(prob)
        engine.set_sectors(pid, [[allb, 0, 0], [sub, 0, 0]])
        site = engine.site_observables(pid, v)
        pair = engine.pair_observables(pid, v)
        P_all, P_sub = engine.sector_values(pid, v)
    finally:
        engine.set_option("tile_bits", 13)
        engine.set_option("site_obs", 0)
        engine.set_option("pair_obs", 0)
        engine.clear()
    M = np.arange(n + 1)
    _check(np.array([n / 2 - M @ P_all]), np.array([site[2].sum()]), 1e-12, f"n = {n}: mean of all bits against site_obs")
    bits = [b for b in range(n) if sub >> b & 1]
    _check(np.array([len(bits) / 2 - np.arange(len(bits) + 1) @ P_sub]), np.array([site[2][bits].sum()]), 1e-12,
           f"n = {n}: mean of five bits against site_obs")
    second = ((n / 2 - M) ** 2) @ P_all
    _check(np.array([second]), np.array([n / 4 + 2 * pair[0].sum()]), 1e-12, f"n = {n}: second moment against pair_obs")


@pytest.mark.parametrize("n,tile_bits", [(9, 6), (14, 13)])
def test_bins_agree_with_population_strings(engine, n, tile_bits):
    """A three-bit m: each bin is the sum of the Ea / Eb strings of the configurations with that many
    spins down; the bins of a conditioned set sum to the Ea string of the selecting bit (1e-12)."""
    prob = _random_problem(n, 60 + n, rare_bit=n - 1)
    v = _rand(n, 6 * n) * 1.1
    b3 = (0, n // 2, n - 1)
    sel = 2
    m3 = sum(1 << b for b in b3)
    codes, weight = [], []
    for c in range(8):
        codes.append(codes_of(n, **{f"b{b}": (B_ if c >> i & 1 else A_) for i, b in enumerate(b3)}))
        weight.append(bin(c).count("1"))
    codes.append(codes_of(n, **{f"b{sel}": A_}))
    engine.clear()
    engine.set_option("tile_bits", tile_bits)
    try:
        pid = engine.add(prob)
        engine.set_op_strings(pid, np.stack(codes))
        engine.set_sectors(pid, [[m3, 0, 0], [((1 << n) - 1) & ~(1 << sel), 1 << sel, 0]])
        sv = engine.op_string_values(pid, v)
        P3, Pc = engine.sector_values(pid, v)
    finally:
        engine.set_option("tile_bits", 13)
        engine.clear()
    assert np.abs(sv.imag).max() == 0.0
    want = np.array([sum(sv[c].real for c in range(8) if weight[c] == j) for j in range(4)])
    _check(P3, want, 1e-12, f"n = {n}: bins of a three-bit m against the population strings")
    _check(np.array([Pc.sum()]), np.array([sv[8].real]), 1e-12, f"n = {n}: a conditioned set's total against Ea")


# ------------------------------------------------------------------------------ 4. a conserved quantity
def test_conserved_quantities_without_drive(engine):
    """B1 = 0: the rare bit's projector commutes with H and H connects only bit weights that differ by 0
    or 2 (both asserted here in numpy on problem_to_csr, so the test states its premise).  The two-bin
    set on the rare bit and the even-weight total of the all-bits set are then constant over the outputs
    (1e-10), from a state that is no eigenstate of either."""
    from quantumsimulations_amd.dipolar_ensemble_with_rare import problem_to_csr
    params = dataclasses.replace(sweep_point_params(5, 50e3, "center_on", 1e-3, 9), B1_sea=0.0, B1_rare=0.0)
    prob = pb.build_problem(params, order="engine", reduce=False)
    n = prob.n_qubits
    assert n == 6 and prob.rare_bit >= 0
    H = problem_to_csr(prob).toarray()
    x = np.arange(1 << n)
    proj = np.diag(((x >> prob.rare_bit) & 1).astype(np.float64))
    assert np.abs(H @ proj - proj @ H).max() == 0.0
    w = popcount(x)
    r, c = np.nonzero(H)
    assert set(np.abs(w[r] - w[c]).tolist()) <= {0, 2} and 2 in set(np.abs(w[r] - w[c]).tolist())
    psi0 = _rand(n, 321)
    S = np.array([[1 << prob.rare_bit, 0, 0], [(1 << n) - 1, 0, 0]], dtype=np.uint64)
    t = np.linspace(0.0, 1e-3, 9)
    for opts in (dict(dense=0), dict(dense=2)):  # the small engine and the dense engine
        _, st, r = _run(engine, [prob], t, [S], [psi0], **opts)
        tr = r["sec"][0]
        rare, full = tr[:2], tr[2:]
        assert full.shape == (n + 1, 9)
        d_rare = np.abs(rare - rare[:, :1]).max()
        even = full[0::2].sum(axis=0)
        d_even = np.abs(even - even[0]).max()
        spread = np.abs(full - full[:, :1]).max()
        print(f"mode {st['mode']}: rare-bit bins move by {d_rare:.2e}, even-weight total by {d_even:.2e} (bound 1e-10); "
              f"the bins themselves move by {spread:.2e}")
        assert d_rare < 1e-10 and d_even < 1e-10
        assert spread > 1e-6 and 0.05 < rare[0, 0] < 0.95 and 0.05 < even[0] < 0.95  # (not trivially constant)


# ------------------------------------------------------------------------------ 5. evolve, per engine
@pytest.mark.parametrize("reduce", [True, False])
def test_small_engine(engine, reduce):
    """N = 7, three launches of the engine (small_chunk 4 < 8 intervals)."""
    def ok(st):
        assert st["mode"] == 3
    for i, p in enumerate(_n7(reduce)):
        _engine_case(engine, p, T9, dict(dense=0, small_chunk=4), ok, states=eigh_states(("n7", i, reduce), p, T9))


def test_streaming_n12(engine):
    def ok(st):
        assert st["mode"] == 0 and st["dense_problems"] == 0
    p = _p12()
    _engine_case(engine, p, T7, dict(persistent=0, wht=0, tile_bits=9, dense=0), ok, states=eigh_states("n12", p, T7))


def test_walsh_hadamard_n15(engine):
    def ok(st):
        assert st["mode"] == 2 and st["span_problems"] == 0
    p = _random_problem(15, 515, rare_bit=14)
    _engine_case(engine, p, np.linspace(0.0, 1e-3, 3), dict(span_tile=0), ok, other_opts=dict(wht=0, span_tile=0))


def test_walsh_hadamard_n14_tile12_matches_expm(engine):
    def ok(st):
        assert st["mode"] == 2
    p = _random_problem(14, 514, rare_bit=13)
    _engine_case(engine, p, T7, dict(persistent=0, tile_bits=12, dense=0), ok, states=expm_states("r14", p, T7))


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("n_t", [6, 7])
@pytest.mark.parametrize("n", [13, 14])
def test_interval_kernel(engine, n, n_t, overlap):
    def ok(st):
        assert st["mode"] == 1 and st["outputs_per_launch"] == 2 and st["span_problems"] == 0
    p = _random_problem(n, 500 + n, rare_bit=n - 1)
    _engine_case(engine, p, T7[:n_t], dict(IV_OPTS, obs_overlap=overlap), ok, states=expm_states(f"r{n}", p, T7)[:n_t])


def test_interval_kernel_custom_initial_state(engine):
    def ok(st):
        assert st["mode"] == 1 and st["custom_init_problems"] == 1
    p = _random_problem(13, 513, rare_bit=12)
    psi0 = _rand(13, 77)
    t = T7[:6]
    _engine_case(engine, p, t, dict(IV_OPTS, obs_overlap=0), ok, states=expm_from("r13c", p, psi0, t), init=psi0)


@pytest.mark.parametrize("n,span_tile", [(12, 10), (14, 11)])
def test_span_kernel(engine, n, span_tile):
    def ok(st):
        assert st["mode"] == 1 and st["span_problems"] == 1
    t = np.linspace(0.0, 1e-3, 6)
    if n == 12:
        p = _p12()
        states = eigh_states("n12", p, t)
    else:
        p = _random_problem(14, 514, rare_bit=13)
        states = expm_states("r14", p, t)
    _engine_case(engine, p, t, dict(span_tile=span_tile, span_outputs=4, matrix=0, dense=0), ok, states=states)


def test_real_kernel_n13(engine):
    def ok(st):
        assert st["mode"] == 1 and st["real_problems"] == 1
    p = _imag_problem(13, 613)
    _engine_case(engine, p, T7, dict(real=1, span_tile=0, matrix=0, dense=0), ok, states=expm_states("i13", p, T7))


@pytest.mark.parametrize("nufft", [0, 2])
def test_dense_engine_n7(engine, nufft):
    def ok(st):
        assert st["dense_problems"] == 1 and st["mode"] == 4 and st["dense_nufft_problems"] == (1 if nufft else 0)
    for i, p in enumerate(_n7(True)):
        _engine_case(engine, p, T9, dict(dense=2, dense_nufft=nufft), ok, states=eigh_states(("n7", i, True), p, T9))


def test_dense_engine_custom_initial_state(engine):
    def ok(st):
        assert st["dense_problems"] == 1 and st["custom_init_problems"] == 1
    p = _n7(True)[0]
    psi0 = _rand(p.n_qubits, 78)
    _engine_case(engine, p, T9, dict(dense=2, dense_nufft=0), ok, states=eigh_from(p, psi0, T9), init=psi0)


def test_dense_engine_one_register_of_1024(engine):
    def ok(st):
        assert st["dense_problems"] == 1
    p = _p10()
    _engine_case(engine, p, T7, dict(dense=2), ok, states=eigh_states("n10", p, T7))


def test_matrix_mode(engine):
    def ok(st):
        assert st["mode"] == 5
    p = _p10()
    t = np.linspace(0.0, 1e-3, 17)  # (the mode takes a uniform grid of at least 17 outputs)
    _engine_case(engine, p, t, dict(matrix=2, dense=0), ok, states=eigh_states("n10", p, t))


# ------------------------------------------------------------------------------ 6. mixed context
def test_mixed_context_matches_lone_registers(engine):
    """Registers of 7, 12 and 14 qubits with K = 3, 0, 4 in one context (small engine, 1- and 2-tile
    k_interval): each one's traces as from a context of its own; the register without sets has none."""
    probs = [_random_problem(n, 700 + n, rare_bit=n - 1) for n in (7, 12, 14)]
    secs = [evolve_sets(7)[:3], None, evolve_sets(14)]
    opts = dict(span_tile=0, matrix=0, dense=0)
    engine.clear()
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        for p, s in zip(probs, secs):
            pid = engine.add(p)
            if s is not None:
                engine.set_sectors(pid, s)
        engine.evolve(T7)
        assert engine.sector_problems() == 2
        assert [engine.sectors(i) for i in range(3)] == [3, 0, 4]
        with pytest.raises(RuntimeError):
            engine.sector_traces(1)
        mixed = [flat(engine.sector_traces(0)), None, flat(engine.sector_traces(2))]
    finally:
        for k in opts:
            engine.set_option(k, DEFAULTS[k])
        engine.clear()
    for i in (0, 2):
        _, _, r1 = _run(engine, [probs[i]], T7, [secs[i]], **opts)
        _check(mixed[i], r1["sec"][0], 1e-12, f"register {i} mixed against alone")


# ------------------------------------------------------------------------------ 7. nothing else moves
@pytest.mark.parametrize("case", ["n7", "n13", "n14", "dense"])
def test_everything_else_bitwise_unchanged_and_sectors_repeatable(engine, case):
    if case in ("n7", "dense"):
        probs = [pb.build_problem(sweep_point_params(6, 50e3, v, 1e-3, 7)) for v in VARIANTS]
    else:
        probs = [pb.build_problem(sweep_point_params(13, d, "center_off" if case == "n13" else "center_on", 2e-5, 7))
                 for d in (0.0, 150e3)]
        assert probs[0].n_qubits == int(case[1:])
    t = T7 if case in ("n7", "dense") else np.linspace(0.0, 2e-5, 7)
    opts = {"dense": 2} if case == "dense" else {}
    refs = [make_refs(p.n_qubits, 40 + i, 2) for i, p in enumerate(probs)]
    strs = [evolve_set(p.n_qubits)[:3 + i % 2] for i, p in enumerate(probs)]
    secs = [evolve_sets(p.n_qubits)[:2 + i % 3] for i, p in enumerate(probs)]
    kw = dict(sites=1, pairs=1, refs=refs, strs=strs, **opts)
    off, st_off, r_off = _run(engine, probs, t, None, **kw)
    on, st_on, r_on = _run(engine, probs, t, secs, **kw)
    on2, _, r_on2 = _run(engine, probs, t, secs, **kw)
    off2, _, r_off2 = _run(engine, probs, t, None, **kw)  # the sets dropped again
    assert np.array_equal(on, off) and np.array_equal(on2, off) and np.array_equal(off2, off)
    for k in ("sites", "pairs", "ov", "str", "state"):
        for a, b, c in zip(r_on[k], r_off[k], r_off2[k]):
            assert np.array_equal(a, b) and np.array_equal(c, b), k
    for a, b in zip(r_on["sec"], r_on2["sec"]):
        assert np.array_equal(a, b)
    for k in ("mode", "dense_problems", "span_problems", "real_problems", "outputs_per_launch", "tile_bits"):
        assert st_on[k] == st_off[k], k
    assert r_off["problems"] == 0 and r_on["problems"] == len(probs) and r_off2["problems"] == 0


# ------------------------------------------------------------------------------ 8. hand-off re-run
def test_rerun_after_handoff_timeout_overwrites(engine):
    dense_p = pb.build_problem(sweep_point_params(6, 75e3, "center_on", 1e-3, 7))
    cheb_p = _random_problem(14, 514, rare_bit=13)  # complex drives: not dense-eligible
    probs = [dense_p, cheb_p]
    secs = [evolve_sets(p.n_qubits) for p in probs]
    opts = dict(dense=2, span_tile=0)
    _, st, r = _run(engine, probs, T7, secs, **opts)
    assert st["dense_problems"] == 1 and st["handoff_fallbacks"] == 0 and st["mode"] == 1
    _, st2, r2 = _run(engine, probs, T7, secs, spin_limit=-1, **opts)
    assert st2["dense_problems"] == 1 and st2["handoff_fallbacks"] >= 1 and r2["problems"] == 2
    assert np.array_equal(r2["sec"][0], r["sec"][0])
    assert r2["sec"][1].shape == (_lib.sector_layout(14, secs[1])[0], 7)
    _check(r2["sec"][1], r["sec"][1], 1e-11, "re-run against the persistent pass")
    _check(r2["sec"][1], flat(sector_ref(secs[1], expm_states("r14", cheb_p, T7))), 1e-10, "re-run against expm")


# ------------------------------------------------------------------------------ 9. errors and lifetime
def test_errors_and_lifetime(engine):
    n = 10
    p = _random_problem(n, 33, rare_bit=9)
    S = evolve_sets(n)[:2]
    v = _rand(n, 12)
    L = _lib.lib()
    engine.clear()
    try:
        pid = engine.add(p)
        with pytest.raises(ValueError):      # above the cap
            engine.set_sectors(pid, np.tile(S[:1], (_lib.DSE_MAX_SECTOR_SETS + 1, 1)))
        with pytest.raises(ValueError):      # a bit at n
            engine.set_sectors(pid, [[1 << n, 0, 0]])
        with pytest.raises(ValueError):      # a selecting bit at n
            engine.set_sectors(pid, [[1, 1 << n, 0]])
        with pytest.raises(ValueError):      # counted and selecting
            engine.set_sectors(pid, [[3, 2, 0]])
        with pytest.raises(ValueError):      # a value outside the selecting bits
            engine.set_sectors(pid, [[1, 2, 4]])
        with pytest.raises(ValueError):      # a bad id
            engine.set_sectors(pid + 1, S)
        with pytest.raises(ValueError):      # three masks per set
            engine.set_sectors(pid, [[1, 2]])
        assert L.dse_set_sectors(engine._h, pid, 2, None) == _lib.DSE_ERR_ARG  # null masks
        assert L.dse_set_sectors(engine._h, pid, -1, _lib.u64ptr(S)) == _lib.DSE_ERR_ARG
        assert engine.sectors(pid) == 0 and engine.sector_units(pid) == 0
        with pytest.raises(RuntimeError):    # no sets: the hook
            engine.sector_values(pid, v)
        engine.set_sectors(pid, S)
        assert engine.sector_units(pid) == (n + 1) + (n // 2 + 1)
        with pytest.raises(RuntimeError):    # before any evolve: DSE_ERR_STATE
            engine.sector_traces(pid)
        out = np.empty(64 * 8)
        assert L.dse_get_sectors(engine._h, pid, _lib.ptr(out)) == _lib.DSE_ERR_STATE
        engine.evolve(T7)
        assert flat(engine.sector_traces(pid)).shape == (17, 7)
        with pytest.raises(ValueError):      # a failed evolve ends the earlier results
            engine.evolve(np.array([0.0, 1e-4, 1e-4]))
        with pytest.raises(RuntimeError):
            engine.sector_traces(pid)
        S3 = evolve_sets(n)[1:4]
        engine.set_sectors(pid, S3)          # replaced as a set: K and the stride change
        assert engine.sectors(pid) == 3 and engine.sector_units(pid) == 6 + 1 + 6
        _check(flat(engine.sector_values(pid, v)), flat(sector_ref(S3, [v])), 1e-12, "hook after a replaced set")
        engine.evolve(T7[:5])                # the sets persist over evolves
        before = flat(engine.sector_traces(pid))
        assert before.shape == (13, 5)
        engine.set_hamiltonian(pid, p)       # ... and over dse_set_hamiltonian
        assert engine.sectors(pid) == 3
        engine.evolve(T7[:5])
        assert np.array_equal(flat(engine.sector_traces(pid)), before)
        engine.set_sectors(pid, evolve_sets(n))  # a larger U: a wider stride, the same values
        engine.evolve(T7[:5])
        wide = flat(engine.sector_traces(pid))
        assert wide.shape == (11 + 13, 5) and np.array_equal(wide[11:], before)
        engine.set_op_strings(pid, evolve_set(n))  # strings, references and sets together
        engine.set_overlap_refs(pid, make_refs(n, 5, 2))
        engine.evolve(T7[:5])
        assert np.array_equal(flat(engine.sector_traces(pid)), wide)
        assert engine.op_string_traces(pid).shape == (6, 5) and engine.overlap_traces(pid).shape == (2, 5)
        assert engine.sector_problems() == 1
        engine.set_sectors(pid, None)
        assert engine.sectors(pid) == 0
        engine.evolve(T7)
        with pytest.raises(RuntimeError):
            engine.sector_traces(pid)
        assert engine.sector_problems() == 0
        engine.set_sectors(pid, S)
        engine.clear()                       # dse_clear drops them with the problem
        pid = engine.add(p)
        assert engine.sectors(pid) == 0
        engine.clear()
        engine.set_option("tile_bits", 8)
        ps = engine.add_sharded(p, 1)
        with pytest.raises(ValueError):      # a non-zero shard id of a loopback group
            engine.set_sectors(ps + 1, S)
        engine.set_sectors(ps, S)
        engine.evolve(T7)
        whole = flat(engine.sector_traces(ps))
        with pytest.raises(ValueError):
            engine.sector_traces(ps + 1)
    finally:
        engine.set_option("tile_bits", 13)
        engine.clear()
    _, _, r = _run(engine, [p], T7, [S])
    _check(whole, r["sec"][0], 1e-11, "loopback shards against the unsharded register")


# ------------------------------------------------------------------------------ 10. Python surface
def test_simulate_rare_sectors_and_mqc_intensities():
    """n_sea = 5: the populations of the sea, of the sea given the rare spin up / down and of the rare
    spin against the exact states (1e-10); mqc_intensities of the whole register's populations against
    the brute-force sum of |psi_x|^2 |psi_y|^2 over pairs by weight difference on those states (1e-10)."""
    from quantumsimulations_amd.dipolar_ensemble_with_rare import (_engine, initial_state_rare, mqc_intensities,
                                                                   sector_masks_by_bit, sector_moments,
                                                                   simulate_rare_from, simulate_rare_sectors)
    params = sweep_point_params(5, 50e3, "center_on", 1e-3, 9)
    prob = pb.build_problem(params, order="engine", reduce=False)
    n = prob.n_qubits
    assert n == 6 and prob.rare_bit >= 0
    rare = int(prob.site_of_bit[prob.rare_bit])

    def word(sea, at_rare):
        return "".join(at_rare if s == rare else sea for s in range(n))
    sets = [word("w", "w"), word("w", "."), word("w", "a"), word("w", "b"), word(".", "w")]
    t, obs, pops = simulate_rare_sectors(params, sets)
    assert [p.shape for p in pops] == [(7, 9), (6, 9), (6, 9), (6, 9), (2, 9)]
    _, obs0 = simulate_rare_from(params, psi0=initial_state_rare(params))
    for k in obs0:
        assert np.array_equal(obs[k], obs0[k]), k
    states = eigh_states(("n6u", "center_on"), prob, t)
    masks = sector_masks_by_bit(sets, prob.site_of_bit)
    _check(flat(pops), flat(sector_ref(masks, states)), 1e-10, "simulate_rare_sectors against the exact propagation")
    _check(pops[2] + pops[3], pops[1], 1e-13, "the sea given rare up plus given rare down against the sea")
    w = popcount(np.arange(1 << n))
    brute = np.zeros((9, 2 * n + 1))
    for j, psi in enumerate(states):
        p2 = np.abs(psi) ** 2 / np.vdot(psi, psi).real
        for q in range(-n, n + 1):
            brute[j, q + n] = sum(p2[w == M].sum() * p2[w == M - q].sum() for M in range(n + 1) if 0 <= M - q <= n)
    I = mqc_intensities(pops[0].T)
    _check(I, brute, 1e-10, "mqc_intensities against the brute force")
    mom = sector_moments(pops[1].T, 2)
    _check(mom[:, 1], 0.5 * params.n_sea - obs["Iz_sea"], 1e-10, "the sea's mean spins down against the aggregate Iz_sea")
    eng = _engine(0)   # the cached engine is left without sets
    eng.clear()
    try:
        pid = eng.add(prob)
        assert eng.sectors(pid) == 0
        eng.evolve(t)
        with pytest.raises(RuntimeError):
            eng.sector_traces(pid)
    finally:
        eng.clear()
