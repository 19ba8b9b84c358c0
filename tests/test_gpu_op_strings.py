"""Expectation values of operator strings, v = <psi| prod_b O_b |psi> / <psi|psi> with one factor out of
1, Ix, Iy, Iz, I+, I-, Ea, Eb per register bit (dse_set_op_strings, dse_op_string_values,
dse_get_op_strings; feature "op_strings") on every engine.

The reference is numpy and does not share the kernels' mask formulation: the eight 2 x 2 matrices are
applied bit by bit with tensordot on the reshaped state (string_ref).  States come from the exact
propagations of test_gpu_site_obs.py / test_gpu_overlap_obs.py (numpy eigh up to 12 qubits, scipy
expm_multiply at 13 and 14).

Tolerances are the project's (test_gpu_parity.py, test_gpu_overlap_obs.py): abs 1e-12 for a hook on a
given state, 1e-10 for traces against an exact propagation, 1e-11 between two exact propagators of the
engine, bitwise where the same kernel runs the same data.  Every value is bounded by 1, so the bounds
are absolute.  The energy check sums values with the coefficients of H: its bound is 1e-12 times the
sum of their magnitudes.  The measured maxima are printed (-s).

Every evolve case carries evolve_set(n): it holds a string with an odd number of Iy and strings with an odd
number of flips, so a wrong rotated-frame factor of the dense engine cannot cancel.

Measured on an MI355X (worst per section): hook against numpy 1.1e-16, loopback shards 1.1e-16 (sharded
against unsharded: bitwise), site / pair hooks 1.4e-17 / 0, energy 2.3e-13 (bound 5.9e-8), traces against
the exact propagation 1.8e-13 (dense n = 10; tile engines 2.2e-16), between two propagators 2.8e-17,
mixed context 0, re-run 1.4e-16, three-spin reduced density matrix 1.1e-13.

The hook tests against k_obs_strings with one path broken in a scratch copy (test_hook_matches_numpy
stops a case at its first failing class, so that class is what is listed):
  the tile's sign dropped (zm >> L ignored)        "diagonal" at (15, 12), (17, 9); "flips on both sides of
      L" at (9, 6), (16, 13); (3, 12) and (13, 13) have no bit above the tile and pass; all three shard
      cases fail
  bit 0 of xm_lo dropped from the partner index    "flips on thread bits" in all six cases; all three shard
      cases fail
  the selection dropped where a partner is read    "I+ below and I- above the tile" at the four cases with
      bits above the tile, "I+- selected above the tile (none here: the top bit)" at (3, 12) and (13, 13);
      all three shard cases fail
"""
import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.sweep import VARIANTS, sweep_point_params
from test_gpu_overlap_obs import DEFAULTS, T9, IV_OPTS, _n7, basis_state, eigh_from, expm_from, make_refs
from test_gpu_parity import _rand, _random_problem
from test_gpu_site_obs import T7, _imag_problem, _p10, _p12, eigh_states, expm_states

pytestmark = pytest.mark.gpu

I_, X_, Y_, Z_, P_, M_, A_, B_ = range(8)
OPS = np.array([
    [[1, 0], [0, 1]], [[0, 0.5], [0.5, 0]], [[0, -0.5j], [0.5j, 0]], [[0.5, 0], [0, -0.5]],
    [[0, 1], [0, 0]], [[0, 0], [1, 0]], [[1, 0], [0, 0]], [[0, 0], [0, 1]],
], dtype=np.complex128)  # basis (up, down) = bit value (0, 1); I+ = |up><down|


# ------------------------------------------------------------------------------ the numpy reference
def string_ref(codes, states):
    """(K, n_t) complex: <psi| prod_b O_b |psi> / <psi|psi>, the factors applied one bit at a time."""
    codes = np.atleast_2d(codes)
    n = codes.shape[1]
    out = np.empty((codes.shape[0], len(states)), dtype=np.complex128)
    for j, psi in enumerate(states):
        psi = np.asarray(psi, dtype=np.complex128)
        t0 = psi.reshape([2] * n)  # bit b is axis n - 1 - b
        n2 = np.vdot(psi, psi).real
        for k, c in enumerate(codes):
            phi = t0
            for b in range(n):
                if c[b]:
                    phi = np.moveaxis(np.tensordot(OPS[c[b]], phi, axes=([1], [n - 1 - b])), 0, n - 1 - b)
            out[k, j] = np.vdot(t0, phi) / n2
    return out


def codes_of(n, **ops):
    """A string of n codes: codes_of(5, b0=X_, b4=Z_)."""
    c = np.zeros(n, dtype=np.uint8)
    for k, v in ops.items():
        c[int(k[1:])] = v
    return c


def evolve_set(n):
    """Six strings for the evolve cases (n >= 5)."""
    h = n // 2
    return np.stack([
        codes_of(n, b0=Y_, **{f"b{n - 1}": Z_}),                    # one Iy (imaginary prefactor), one flip
        codes_of(n, b0=X_, b1=Z_, **{f"b{n - 1}": X_}),             # two flips, the top and the bottom bit
        codes_of(n, b0=M_, **{f"b{h}": Y_, f"b{n - 1}": P_}),       # I+ I- and one Iy: three flips
        codes_of(n, b0=Z_, b1=Z_, **{f"b{n - 1}": Z_}),             # three-spin order, diagonal
        codes_of(n, b0=A_, b2=X_, **{f"b{n - 1}": B_}),             # a population on two bits times Ix
        np.zeros(n, dtype=np.uint8),                                # the identity
    ])


def _check(got, ref, bound, what):
    assert got.shape == ref.shape and got.dtype == np.complex128, (got.shape, ref.shape)
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max |value - reference| = {err:.3e} (bound {bound:g})")
    assert err < bound, err


def _run(engine, probs, t, strs, inits=None, sites=0, pairs=0, refs=None, **opts):
    """One evolve with the given options (restored afterwards): strs[i] (K, n) codes or None per
    problem.  Returns obs, stats and a dict of per-problem lists."""
    engine.clear()
    out = {"str": [], "state": [], "sites": [], "pairs": [], "ov": []}
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
            if strs is not None and strs[i] is not None:
                engine.set_op_strings(pid, strs[i])
        obs, st = engine.evolve(t)
        out["problems"] = engine.op_string_problems()
        for i in range(len(probs)):
            has = strs is not None and strs[i] is not None
            out["str"].append(engine.op_string_traces(i) if has else None)
            out["state"].append(engine.state(i))
            out["sites"].append(engine.site_traces(i) if sites else None)
            out["pairs"].append(engine.pair_traces(i) if pairs else None)
            out["ov"].append(engine.overlap_traces(i) if refs is not None else None)
    finally:
        for k in list(opts) + ["site_obs", "pair_obs"]:
            engine.set_option(k, DEFAULTS[k])
        engine.clear()
    return obs, st, out


def _engine_case(engine, prob, t, opts, stats_ok, states=None, other_opts=None, init=None):
    """One register on one engine: the traces of evolve_set(n) against the exact states (1e-10) or
    against another exact propagator of the engine (other_opts, 1e-11); the values at t0 against numpy
    on the initial state (1e-12); the identity's value 1."""
    n = prob.n_qubits
    S = evolve_set(n)
    inits = None if init is None else [init]
    obs, st, r = _run(engine, [prob], t, [S], inits, **opts)
    stats_ok(st)
    assert r["problems"] == 1
    tr = r["str"][0]
    assert tr.shape == (len(S), len(t))
    if states is not None:
        _check(tr, string_ref(S, states), 1e-10, "against the exact propagation")
    else:
        _, st0, r0 = _run(engine, [prob], t, [S], inits, **other_opts)
        assert st0["mode"] == 0
        _check(tr, r0["str"][0], 1e-11, "against the engine's streaming propagator")
    psi0 = basis_state(prob) if init is None else init
    _check(tr[:, :1], string_ref(S, [psi0]), 1e-12, "values at t0")
    assert np.max(np.abs(tr[-1] - 1.0)) < 1e-14  # (the identity's sum and the norm's: two roundings of the same terms)
    return obs, st, r


# ------------------------------------------------------------------------------ 1. the hook
def _geometry(n, tile_bits):
    L = min(n, tile_bits)
    lgnt = 9 if L >= 13 else (8 if L >= 8 else 6)
    return L, min(L, lgnt)  # tile bits, thread bits (Geo<L>)


def string_classes(n, tile_bits):
    """The fixed classes of item 1 for an n-bit register at this tile size, each with the predicate its
    compiled masks (xm, zm, cm, cv, pre) must satisfy.  Thread bits are 0 .. TB - 1, a thread's row bits
    TB .. L - 1, the bits above the tile L .. n - 1; a geometry without row bits (L = TB) or without
    bits above the tile (L = n) takes the highest bit below instead and its predicate says so."""
    L, TB = _geometry(n, tile_bits)
    lo, thr, row, hi = (1 << L) - 1, (1 << TB) - 1, ((1 << L) - 1) & ~((1 << TB) - 1), ((1 << n) - 1) & ~((1 << L) - 1)
    top = n - 1
    out = []
    c = np.array([(Z_, A_, B_, I_)[b % 4] for b in range(n)], dtype=np.uint8)
    c[top] = B_
    out.append(("diagonal", c, lambda m: m[0] == 0 and m[1] and m[2] and m[3] and m[2] & (1 << top)))
    out.append(("flips on thread bits", codes_of(n, b0=X_, **{f"b{TB - 1}": X_}),
                lambda m: m[0] and not (m[0] & ~thr) and not m[1] and not m[2]))
    if row:
        c = np.zeros(n, dtype=np.uint8)
        c[TB:L] = X_
        out.append(("flips on row bits", c, lambda m: m[0] == row and not m[2]))
    else:
        out.append(("flips on row bits (none here: the top tile bit)", codes_of(n, **{f"b{L - 1}": X_}),
                    lambda m: L == TB and m[0] == 1 << (L - 1)))
    if hi:
        c = codes_of(n, **{f"b{L}": X_})
        c[top] = X_
        out.append(("flips above the tile", c, lambda m: m[0] and not (m[0] & lo) and m[0] & (1 << L)))
        c = codes_of(n, b0=X_, **{f"b{L - 1}": X_})
        c[L], c[top] = Y_, (X_ if top > L else Y_)
        out.append(("flips on both sides of L", c, lambda m: m[0] & lo and m[0] & hi and m[0] & 1 and m[0] & (1 << (L - 1))))
        c = codes_of(n, **{f"b{top}": P_})
        if L < top:
            c[L] = M_
        out.append(("I+- selected above the tile", c, lambda m: m[2] and not (m[2] & lo) and m[0] == m[2] and m[3] != m[2]))
        out.append(("I+ below and I- above the tile", codes_of(n, b1=P_, **{f"b{top}": M_}),
                    lambda m: m[2] & lo and m[2] & hi and m[3] == 1 << top))
    else:
        assert L == n
        out.append(("flips above the tile (none here: the top bit)", codes_of(n, **{f"b{top}": X_}), lambda m: m[0] == 1 << top))
        out.append(("flips on both sides of L (none here: bits 0 and top)", codes_of(n, b0=X_, **{f"b{top}": Y_}),
                    lambda m: m[0] == (1 | 1 << top)))
        out.append(("I+- selected above the tile (none here: the top bit)", codes_of(n, **{f"b{top}": P_}),
                    lambda m: m[2] == 1 << top and m[3] == 0))
        out.append(("I+ below and I- on the top bit", codes_of(n, b1=P_, **{f"b{top}": M_}), lambda m: m[3] == 1 << top))
    out.append(("I+- selected below the tile", codes_of(n, b1=P_, **{f"b{L - 1}": M_}) if L > 2 else codes_of(n, b1=P_, b0=M_),
                lambda m: m[2] and not (m[2] & ~lo) and m[0] == m[2] and m[3] and m[3] != m[2]))
    c = codes_of(n, b0=Y_, **{f"b{top}": Y_})
    c[n // 2] = Y_
    out.append(("an odd number of Iy", c, lambda m: bin(m[1]).count("1") % 2 == 1 and m[4].real == 0 and m[4].imag != 0))
    c = np.array([1 + (3 * b + 1) % 7 for b in range(n)], dtype=np.uint8)
    out.append(("a factor on every bit", c, lambda m: (m[0] | m[1] | m[2]) == (1 << n) - 1))
    out.append(("the identity", np.zeros(n, dtype=np.uint8), lambda m: m[:4] == (0, 0, 0, 0) and m[4] == 1))
    return out


@pytest.mark.parametrize("n,tile_bits", [(3, 12), (9, 6), (13, 13), (15, 12), (16, 13), (17, 9)])
def test_hook_matches_numpy(engine, n, tile_bits):
    classes = string_classes(n, tile_bits)
    for name, c, pred in classes:
        assert pred(_lib.op_string_masks(c)), (name, c)
    S = np.stack([c for _, c, _ in classes])
    rng = np.random.default_rng(1000 + n)
    S64 = np.concatenate([S, rng.integers(0, 8, (64 - len(S), n)).astype(np.uint8)])
    S64[len(S):][rng.random((64 - len(S), n)) < 0.5] = 0   # (half the random factors the identity: values of size)
    prob = _random_problem(n, 7 + n, rare_bit=n - 2)
    v = _rand(n, 3 * n) * 1.7
    engine.clear()
    engine.set_option("tile_bits", tile_bits)
    try:
        pid = engine.add(prob)
        engine.set_op_strings(pid, S64)
        assert engine.op_strings(pid) == 64
        got64 = engine.op_string_values(pid, v)
        ones = []
        for k in range(len(S)):  # K = 1: every class alone
            engine.set_op_strings(pid, S[k])
            assert engine.op_strings(pid) == 1
            ones.append(engine.op_string_values(pid, v))
    finally:
        engine.set_option("tile_bits", 13)
        engine.clear()
    ref = string_ref(S64, [v])
    for k, (name, _, _) in enumerate(classes):
        e64, e1 = abs(got64[k] - ref[k, 0]), abs(ones[k][0] - ref[k, 0])
        print(f"n = {n}, tile {tile_bits}, {name}: |v| = {abs(ref[k, 0]):.3e}, error K = 64: {e64:.2e}, K = 1: {e1:.2e}")
        assert e64 < 1e-12 and e1 < 1e-12, name
        assert ones[k].shape == (1,) and ones[k][0] == got64[k], name  # the same sums in the same order
    assert abs(got64[len(S) - 1] - 1.0) <= 1e-15
    _check(got64[:, None], ref, 1e-12, f"hook n = {n}, tile {tile_bits}, K = 64")


# ------------------------------------------------------------------------------ 2. loopback shards
@pytest.mark.parametrize("n,bits,tile", [(10, 1, 6), (12, 2, 8), (13, 3, 10)])
def test_hook_sharded_matches_unsharded(engine, n, bits, tile):
    """Strings that flip and select across the shard bits (the top `bits` bits of the register)."""
    prob = _random_problem(n, 900 + 10 * n + bits, rare_bit=n - 1)
    rng = np.random.default_rng(n * 7 + bits)
    v = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    sb = n - bits  # the lowest shard bit
    S = np.stack([
        codes_of(n, b0=X_, **{f"b{n - 1}": X_}),                       # a flip on a shard bit and one in the tile
        codes_of(n, b1=Y_, **{f"b{sb}": P_}),                          # I+ on a shard bit
        codes_of(n, **{f"b{min(tile, sb - 1)}": X_, f"b{tile - 2}": Z_, f"b{sb}": M_}),  # I- on a shard bit, a flip below it
        codes_of(n, b0=Z_, **{f"b{n - 1}": B_, f"b{sb}": Z_}),         # selection and sign on shard bits, diagonal
        codes_of(n, **{f"b{n - 1}": Y_, f"b{sb - 1}": A_}),
        np.array([1 + (5 * b + 2) % 7 for b in range(n)], dtype=np.uint8),
        np.zeros(n, dtype=np.uint8),
    ])
    for c in S[:5]:
        m = _lib.op_string_masks(c)
        assert (m[0] | m[1] | m[2]) >> sb, c
    engine.set_option("tile_bits", tile)
    try:
        engine.clear()
        pid = engine.add(prob)
        engine.set_op_strings(pid, S)
        ref = engine.op_string_values(pid, v)
        engine.clear()
        ps = engine.add_sharded(prob, bits)
        engine.set_op_strings(ps, S)
        got = engine.op_string_values(ps, v)
    finally:
        engine.clear()
        engine.set_option("tile_bits", 13)
    _check(got, ref, 1e-12, "sharded against unsharded")
    _check(got[:, None], string_ref(S, [v]), 1e-12, "sharded against numpy")


# ------------------------------------------------------------------------------ 3. the existing families
@pytest.mark.parametrize("n,tile_bits", [(9, 6), (14, 13)])
def test_agrees_with_site_and_pair_observables(engine, n, tile_bits):
    """One-factor strings are the site observables, Iz Iz / I+ I- / I+ I+ the pair correlators (i < j:
    ZQ = <I+_i I-_j>), on the same state through the existing hooks (1e-12)."""
    prob = _random_problem(n, 40 + n, rare_bit=n - 1)
    v = _rand(n, 5 * n) * 0.9
    one = np.stack([codes_of(n, **{f"b{b}": c}) for c in (X_, Y_, Z_) for b in range(n)])
    pairs = [(i, j) for j in range(1, n) for i in range(j)]
    two = np.stack([codes_of(n, **{f"b{i}": a, f"b{j}": b}) for a, b in ((Z_, Z_), (P_, M_), (P_, P_)) for i, j in pairs])
    engine.clear()
    engine.set_option("tile_bits", tile_bits)
    try:
        pid = engine.add(prob)
        site = engine.site_observables(pid, v)
        pair = engine.pair_observables(pid, v)
        got = []
        for S in (one, two):
            for k0 in range(0, len(S), 64):
                engine.set_op_strings(pid, S[k0:k0 + 64])
                got.append(engine.op_string_values(pid, v))
    finally:
        engine.set_option("tile_bits", 13)
        engine.clear()
    got = np.concatenate(got)
    g1, g2 = got[:3 * n].reshape(3, n), got[3 * n:].reshape(3, len(pairs))
    for i, j in pairs:
        assert pb.pair_index(i, j) == pairs.index((i, j))
    _check(g1, site.astype(np.complex128), 1e-12, f"n = {n}: Ix, Iy, Iz against site_observables")
    want = np.stack([pair[0], pair[1] + 1j * pair[2], pair[3] + 1j * pair[4]])
    _check(g2, want, 1e-12, f"n = {n}: Iz Iz, I+ I-, I+ I+ against pair_observables")


def test_strings_of_h_sum_to_the_energy(engine):
    """n = 12: H = shift + sum field Iz + sum zz Iz Iz + sum (c0 I+ + c1 I-) + sum g (I+ I+ + I- I-)
    (problem_to_csr); the values of its 234 strings on the final state of an evolve, added with the
    problem's coefficients, against Engine.energy.  Each value is within 1e-12, so the bound is 1e-12
    times the sum of the coefficients' magnitudes."""
    n = 12
    prob = _random_problem(n, 52, rare_bit=n - 1)
    S, coef = [], []
    for b in range(n):
        S.append(codes_of(n, **{f"b{b}": Z_})), coef.append(prob.field[b])
        f = prob.flip[b]
        S.append(codes_of(n, **{f"b{b}": P_})), coef.append(f[0] + 1j * f[1])
        S.append(codes_of(n, **{f"b{b}": M_})), coef.append(f[2] + 1j * f[3])
        for c in range(b + 1, n):
            S.append(codes_of(n, **{f"b{b}": Z_, f"b{c}": Z_})), coef.append(prob.zz[b, c])
            S.append(codes_of(n, **{f"b{b}": P_, f"b{c}": P_})), coef.append(prob.pair[b, c])
            S.append(codes_of(n, **{f"b{b}": M_, f"b{c}": M_})), coef.append(prob.pair[b, c])
    S, coef = np.stack(S), np.array(coef, dtype=np.complex128)
    assert len(S) == 3 * n + 3 * n * (n - 1) // 2
    engine.clear()
    try:
        pid = engine.add(prob)
        engine.set_op_strings(pid, S[:64])
        engine.evolve(T7)
        e, n2 = engine.energy(pid)
        psi = engine.state(pid)
        first = engine.op_string_traces(pid)[:, -1]
        vals = []
        for k0 in range(0, len(S), 64):
            engine.set_op_strings(pid, S[k0:k0 + 64])
            vals.append(engine.op_string_values(pid, psi))
    finally:
        engine.clear()
    vals = np.concatenate(vals)
    assert np.array_equal(vals[:64], first)  # the hook on the final state: the evolve's kernel on the same data
    total = prob.shift + np.sum(coef * vals)
    bound = 1e-12 * float(np.sum(np.abs(coef)))
    print(f"energy {e:.6e}, sum of strings {total.real:.6e}{total.imag:+.1e}j: difference {abs(total - e):.3e} (bound {bound:.3e})")
    assert abs(total - e) < bound


# ------------------------------------------------------------------------------ 4. evolve, per engine
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


# ------------------------------------------------------------------------------ 5. mixed context
def test_mixed_context_matches_lone_registers(engine):
    """Registers of 7, 12 and 14 qubits with K = 3, 0, 5 in one context (small engine, 1- and 2-tile
    k_interval): each one's traces as from a context of its own; the register without strings has none."""
    probs = [_random_problem(n, 700 + n, rare_bit=n - 1) for n in (7, 12, 14)]
    strs = [evolve_set(7)[:3], None, evolve_set(14)[:5]]
    opts = dict(span_tile=0, matrix=0, dense=0)
    engine.clear()
    try:
        for k, v in opts.items():
            engine.set_option(k, v)
        for p, s in zip(probs, strs):
            pid = engine.add(p)
            if s is not None:
                engine.set_op_strings(pid, s)
        engine.evolve(T7)
        assert engine.op_string_problems() == 2
        assert [engine.op_strings(i) for i in range(3)] == [3, 0, 5]
        with pytest.raises(RuntimeError):
            engine.op_string_traces(1)
        mixed = [engine.op_string_traces(0), None, engine.op_string_traces(2)]
    finally:
        for k in opts:
            engine.set_option(k, DEFAULTS[k])
        engine.clear()
    for i in (0, 2):
        _, _, r1 = _run(engine, [probs[i]], T7, [strs[i]], **opts)
        _check(mixed[i], r1["str"][0], 1e-12, f"register {i} mixed against alone")


# ------------------------------------------------------------------------------ 6. nothing else moves
@pytest.mark.parametrize("case", ["n7", "n13", "n14", "dense"])
def test_everything_else_bitwise_unchanged_and_strings_repeatable(engine, case):
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
    off, st_off, r_off = _run(engine, probs, t, None, sites=1, pairs=1, refs=refs, **opts)
    on, st_on, r_on = _run(engine, probs, t, strs, sites=1, pairs=1, refs=refs, **opts)
    on2, _, r_on2 = _run(engine, probs, t, strs, sites=1, pairs=1, refs=refs, **opts)
    assert np.array_equal(on, off) and np.array_equal(on2, off)
    for k in ("sites", "pairs", "ov", "state"):
        for a, b in zip(r_on[k], r_off[k]):
            assert np.array_equal(a, b), k
    for a, b in zip(r_on["str"], r_on2["str"]):
        assert np.array_equal(a, b)
    for k in ("mode", "dense_problems", "span_problems", "real_problems", "outputs_per_launch", "tile_bits"):
        assert st_on[k] == st_off[k], k
    assert r_off["problems"] == 0 and r_on["problems"] == len(probs)


# ------------------------------------------------------------------------------ 7. hand-off re-run
def test_rerun_after_handoff_timeout_overwrites(engine):
    dense_p = pb.build_problem(sweep_point_params(6, 75e3, "center_on", 1e-3, 7))
    cheb_p = _random_problem(14, 514, rare_bit=13)  # complex drives: not dense-eligible
    probs = [dense_p, cheb_p]
    strs = [evolve_set(p.n_qubits) for p in probs]
    opts = dict(dense=2, span_tile=0)
    _, st, r = _run(engine, probs, T7, strs, **opts)
    assert st["dense_problems"] == 1 and st["handoff_fallbacks"] == 0 and st["mode"] == 1
    _, st2, r2 = _run(engine, probs, T7, strs, spin_limit=-1, **opts)
    assert st2["dense_problems"] == 1 and st2["handoff_fallbacks"] >= 1 and r2["problems"] == 2
    assert np.array_equal(r2["str"][0], r["str"][0])
    assert r2["str"][1].shape == (6, 7)
    _check(r2["str"][1], r["str"][1], 1e-11, "re-run against the persistent pass")
    _check(r2["str"][1], string_ref(strs[1], expm_states("r14", cheb_p, T7)), 1e-10, "re-run against expm")


# ------------------------------------------------------------------------------ 8. errors and lifetime
def test_errors_and_lifetime(engine):
    n = 10
    p = _random_problem(n, 33, rare_bit=9)
    S = evolve_set(n)[:2]
    v = _rand(n, 12)
    engine.clear()
    try:
        pid = engine.add(p)
        with pytest.raises(ValueError):      # above the cap
            engine.set_op_strings(pid, np.tile(S[:1], (_lib.DSE_MAX_OP_STRINGS + 1, 1)))
        bad = S.copy()
        bad[1, 5] = 8
        with pytest.raises(ValueError):      # a code above 7
            engine.set_op_strings(pid, bad)
        with pytest.raises(ValueError):      # a bad id
            engine.set_op_strings(pid + 1, S)
        with pytest.raises(ValueError):      # one code per register bit
            engine.set_op_strings(pid, S[:, :9])
        assert engine.op_strings(pid) == 0
        with pytest.raises(RuntimeError):    # no strings: the hook
            engine.op_string_values(pid, v)
        engine.set_op_strings(pid, S)
        with pytest.raises(RuntimeError):    # before any evolve
            engine.op_string_traces(pid)
        engine.evolve(T7)
        assert engine.op_string_traces(pid).shape == (2, 7)
        with pytest.raises(ValueError):      # a failed evolve ends the earlier results
            engine.evolve(np.array([0.0, 1e-4, 1e-4]))
        with pytest.raises(RuntimeError):
            engine.op_string_traces(pid)
        S3 = evolve_set(n)[2:5]
        engine.set_op_strings(pid, S3)       # replaced as a set
        assert engine.op_strings(pid) == 3
        with pytest.raises(ValueError):      # the hook reads the new set, whatever became of the evolve between
            engine.evolve(T7, tol=1.0)
        _check(engine.op_string_values(pid, v)[:, None], string_ref(S3, [v]), 1e-12, "hook after a replaced set")
        engine.evolve(T7[:5])                # the strings persist over evolves
        assert engine.op_string_traces(pid).shape == (3, 5)
        before = engine.op_string_traces(pid)
        engine.set_hamiltonian(pid, p)       # ... and over dse_set_hamiltonian
        assert engine.op_strings(pid) == 3
        engine.evolve(T7[:5])
        assert np.array_equal(engine.op_string_traces(pid), before)
        engine.set_op_strings(pid, None)
        assert engine.op_strings(pid) == 0
        engine.evolve(T7)
        with pytest.raises(RuntimeError):
            engine.op_string_traces(pid)
        assert engine.op_string_problems() == 0
        engine.set_op_strings(pid, S)
        engine.clear()                       # dse_clear drops them with the problem
        pid = engine.add(p)
        assert engine.op_strings(pid) == 0
        engine.clear()
        engine.set_option("tile_bits", 8)
        ps = engine.add_sharded(p, 1)
        with pytest.raises(ValueError):      # a non-zero shard id of a loopback group
            engine.set_op_strings(ps + 1, S)
        engine.set_op_strings(ps, S)
        engine.evolve(T7)
        whole = engine.op_string_traces(ps)
        with pytest.raises(ValueError):
            engine.op_string_traces(ps + 1)
    finally:
        engine.set_option("tile_bits", 13)
        engine.clear()
    _, _, r = _run(engine, [p], T7, [S])
    _check(whole, r["str"][0], 1e-11, "loopback shards against the unsharded register")


# ------------------------------------------------------------------------------ 9. Python surface
def test_simulate_rare_strings_reduced_density_matrix():
    """N = 7: the 63 strings of (rare, two sea sites) give the three-spin reduced density matrix of
    every output; against the partial trace of the exact states (1e-10), eigenvalues in [0, 1] to 1e-10."""
    from quantumsimulations_amd.dipolar_ensemble_with_rare import (_engine, engine_to_reference_state, initial_state_rare,
                                                                   rdm_from_string_values, rdm_strings, simulate_rare_from,
                                                                   simulate_rare_strings)
    params = sweep_point_params(6, 50e3, "center_on", 1e-3, 9)
    prob = pb.build_problem(params, order="engine", reduce=False)
    n = prob.n_qubits
    assert n == 7 and prob.rare_bit >= 0
    rare = int(prob.site_of_bit[prob.rare_bit])
    sea = [s for s in range(n) if s != rare]
    sites = (rare, sea[1], sea[-1])
    strings = rdm_strings(sites, n)
    assert len(strings) == 63
    t, obs, vals = simulate_rare_strings(params, strings)
    assert vals.shape == (63, 9) and vals.dtype == np.complex128
    _, obs0 = simulate_rare_from(params, psi0=initial_state_rare(params))
    for k in obs0:
        assert np.array_equal(obs[k], obs0[k]), k
    print("max |Im value| of the Hermitian strings: %.2e" % np.abs(vals.imag).max())
    assert np.abs(vals.imag).max() < 1e-12
    rho = rdm_from_string_values(vals)
    assert rho.shape == (9, 8, 8)
    states = eigh_states(("n7u", "center_on"), prob, t)
    worst, lo, hi = 0.0, 0.0, 1.0
    for j, psi in enumerate(states):
        ref = engine_to_reference_state(psi, prob.site_of_bit).reshape([2] * n)
        rest = [s for s in range(n) if s not in sites]
        m = np.transpose(ref, list(sites) + rest).reshape(8, -1)
        want = m @ m.conj().T / np.vdot(psi, psi).real
        worst = max(worst, float(np.abs(rho[j] - want).max()))
        w = np.linalg.eigvalsh(rho[j])
        lo, hi = min(lo, w[0]), max(hi, w[-1])
    print(f"max |rho - partial trace| = {worst:.3e} (bound 1e-10); eigenvalues in [{lo:.2e}, 1 + {hi - 1:.2e}]")
    assert worst < 1e-10 and lo >= -1e-10 and hi <= 1 + 1e-10
    eng = _engine(0)   # the cached engine is left without strings
    eng.clear()
    try:
        pid = eng.add(prob)
        assert eng.op_strings(pid) == 0
        eng.evolve(t)
        with pytest.raises(RuntimeError):
            eng.op_string_traces(pid)
    finally:
        eng.clear()
