"""Host-side checks of the operator strings (no device): the header / EXPORTED entries,
dse_has_feature, the compiler from operator codes to masks (dse_op_string_masks) against Kronecker
products of the eight 2 x 2 matrices, the site-order mapping, the reduced-density-matrix helpers and the
compiler's resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd.dipolar_ensemble_with_rare import (op_strings_by_bit, rdm_from_string_values,
                                                               rdm_strings, simulate_rare_strings)
from quantumsimulations_amd.sweep import sweep_point_params
from test_pair_obs_host import _compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("dse_set_op_strings", "dse_op_strings", "dse_op_string_values", "dse_get_op_strings",
               "dse_op_string_outputs", "dse_op_string_problems", "dse_op_string_masks")

# the eight one-spin operators by code, basis (up, down) = bit value (0, 1)
OPS = np.array([
    [[1, 0], [0, 1]],          # 1
    [[0, 0.5], [0.5, 0]],      # Ix
    [[0, -0.5j], [0.5j, 0]],   # Iy
    [[0.5, 0], [0, -0.5]],     # Iz
    [[0, 1], [0, 0]],          # I+ = |up><down|
    [[0, 0], [1, 0]],          # I- = |down><up|
    [[1, 0], [0, 0]],          # Ea
    [[0, 0], [0, 1]],          # Eb
], dtype=np.complex128)


def kron_of(codes):
    """The matrix of a string, codes by register bit (bit 0 the least significant index bit)."""
    m = np.ones((1, 1), dtype=np.complex128)
    for c in codes:  # bit b ends up the b-th factor from the right
        m = np.kron(OPS[c], m)
    return m


def mask_sum(codes, psi):
    """The masks-and-prefactor sum of include/dse.h, straight from the formula."""
    xm, zm, cm, cv, pre = _lib.op_string_masks(codes)
    x = np.arange(psi.size, dtype=np.int64)
    sel = (x & cm) == cv
    par = np.zeros(psi.size, dtype=np.int64)
    for b in range(len(codes)):
        par ^= ((x & zm) >> b) & 1
    return pre * np.sum(np.where(sel, (1 - 2 * par) * np.conj(psi) * psi[x ^ xm], 0.0))


# ------------------------------------------------------------------------------ ABI surface
def test_header_declares_and_lib_exports_the_entries():
    with open(os.path.join(ROOT, "include", "dse.h")) as f:
        text = f.read()
    L = _lib.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in _lib.EXPORTED, name
        assert hasattr(L, name), name
    assert '"op_strings"' in text and "enum dse_site_op" in text
    assert re.search(r"#define DSE_MAX_OP_STRINGS 64\b", text) and _lib.DSE_MAX_OP_STRINGS == 64
    for code, name in enumerate(("DSE_OP_1", "DSE_OP_X", "DSE_OP_Y", "DSE_OP_Z", "DSE_OP_P", "DSE_OP_M", "DSE_OP_EA",
                                 "DSE_OP_EB")):
        assert re.search(name + r" = %d\b" % code, text) and getattr(_lib, name) == code
    # the version numbers and dse_stats did not move: the addition is discovered by name
    assert "#define DSE_ABI_VERSION 14" in text and "#define DSE_ABI_MINOR 1" in text
    assert _lib.DseStats._fields_[-1][0] == "custom_init_problems"


def test_has_feature():
    L = _lib.lib()
    assert L.dse_has_feature(b"op_strings") == 1
    assert L.dse_has_feature(b"overlap_obs") == 1 and L.dse_has_feature(b"pair_obs") == 1
    assert L.dse_has_feature(b"op_string") == 0 and L.dse_has_feature(ctypes.c_char_p(None)) == 0
    assert _lib.has_feature("op_strings")


def test_null_context_and_bad_ids_are_refused():
    L = _lib.lib()
    assert L.dse_set_op_strings(None, 0, 0, None) == _lib.DSE_ERR_ARG
    assert L.dse_op_strings(None, 0) == _lib.DSE_ERR_ARG
    assert L.dse_op_string_outputs(None) == _lib.DSE_ERR_ARG and L.dse_op_string_problems(None) == _lib.DSE_ERR_ARG
    assert L.dse_get_op_strings(None, 0, None) == _lib.DSE_ERR_ARG
    assert L.dse_op_string_values(None, 0, None, None) == _lib.DSE_ERR_ARG
    masks = (ctypes.c_uint64 * 4)()
    pre = (ctypes.c_double * 2)()
    ok = np.zeros(3, dtype=np.uint8)
    assert L.dse_op_string_masks(3, _lib.u8ptr(ok), masks, pre) == 0
    assert (list(masks), list(pre)) == ([0, 0, 0, 0], [1.0, 0.0])  # the identity
    assert L.dse_op_string_masks(0, _lib.u8ptr(ok), masks, pre) == _lib.DSE_ERR_ARG
    assert L.dse_op_string_masks(35, _lib.u8ptr(ok), masks, pre) == _lib.DSE_ERR_ARG
    assert L.dse_op_string_masks(3, None, masks, pre) == _lib.DSE_ERR_ARG
    assert L.dse_op_string_masks(3, _lib.u8ptr(ok), None, pre) == _lib.DSE_ERR_ARG
    assert L.dse_op_string_masks(3, _lib.u8ptr(ok), masks, None) == _lib.DSE_ERR_ARG
    bad = np.array([0, 8, 0], dtype=np.uint8)
    assert L.dse_op_string_masks(3, _lib.u8ptr(bad), masks, pre) == _lib.DSE_ERR_ARG
    with pytest.raises(ValueError):
        _lib.op_string_masks(bad)


# ------------------------------------------------------------------------------ the compiler
def test_masks_of_every_three_bit_string():
    """All 8^3 strings at n = 3: the mask sum equals <psi| kron |psi> on a random psi (1e-14); the masks
    are what the header says of each code."""
    rng = np.random.default_rng(3)
    psi = rng.standard_normal(8) + 1j * rng.standard_normal(8)
    psi /= np.linalg.norm(psi)
    worst = 0.0
    for s in range(8 ** 3):
        codes = [(s >> (3 * b)) & 7 for b in range(3)]
        xm, zm, cm, cv, pre = _lib.op_string_masks(codes)
        assert xm == sum(1 << b for b, c in enumerate(codes) if c in (1, 2, 4, 5))
        assert zm == sum(1 << b for b, c in enumerate(codes) if c in (2, 3))
        assert cm == sum(1 << b for b, c in enumerate(codes) if c in (4, 5, 6, 7))
        assert cv == sum(1 << b for b, c in enumerate(codes) if c in (5, 7))
        assert pre == 0.5 ** sum(c in (1, 2, 3) for c in codes) * (-1j) ** sum(c == 2 for c in codes)
        want = np.vdot(psi, kron_of(codes) @ psi)
        worst = max(worst, abs(mask_sum(codes, psi) - want))
    print("n = 3, all 512 strings: max |mask sum - <psi|kron|psi>| = %.2e" % worst)
    assert worst <= 1e-14


def test_masks_of_random_six_bit_strings():
    rng = np.random.default_rng(6)
    psi = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    psi /= np.linalg.norm(psi)
    worst = 0.0
    for _ in range(200):
        codes = rng.integers(0, 8, 6)
        want = np.vdot(psi, kron_of(codes) @ psi)
        worst = max(worst, abs(mask_sum(codes, psi) - want))
    print("n = 6, 200 random strings: max |mask sum - <psi|kron|psi>| = %.2e" % worst)
    assert worst <= 1e-14


def test_masks_of_the_widest_register():
    codes = np.zeros(34, dtype=np.uint8)
    codes[33], codes[32], codes[0] = _lib.DSE_OP_M, _lib.DSE_OP_Y, _lib.DSE_OP_Z
    xm, zm, cm, cv, pre = _lib.op_string_masks(codes)
    assert (xm, zm, cm, cv) == ((1 << 33) | (1 << 32), (1 << 32) | 1, 1 << 33, 1 << 33) and pre == -0.25j


# ------------------------------------------------------------------------------ Python helpers
def test_op_strings_by_bit_under_a_permutation():
    sob = np.array([2, 0, 3, 1])  # bit b holds site sob[b]
    out = op_strings_by_bit(["1x+b", "zy-a"], sob)
    assert out.dtype == np.uint8 and out.shape == (2, 4)
    # "1x+b": site 0 '1', site 1 'x', site 2 '+', site 3 'b'
    np.testing.assert_array_equal(out[0], [4, 0, 7, 1])
    np.testing.assert_array_equal(out[1], [5, 3, 6, 2])
    np.testing.assert_array_equal(op_strings_by_bit("1111", sob), np.zeros((1, 4), dtype=np.uint8))
    for bad in (["1x+"], ["1x+q"], [b"1x+b"]):
        with pytest.raises(ValueError):
            op_strings_by_bit(bad, sob)
    with pytest.raises(ValueError):
        op_strings_by_bit(["1x+b"], [0, 0, 1, 2])


def _partial_trace(psi, sites, n):
    """rho of `sites` (first the most significant) of a ket whose site 0 is the most significant bit."""
    t = psi.reshape([2] * n)
    rest = [s for s in range(n) if s not in sites]
    t = np.transpose(t, list(sites) + rest).reshape(1 << len(sites), -1)
    return t @ t.conj().T


@pytest.mark.parametrize("sites", [(3,), (0,), (1, 4), (4, 1), (2, 0, 3), (4, 3, 0)])
def test_rdm_helpers_against_the_partial_trace(sites):
    n = 5
    rng = np.random.default_rng(50 + len(sites))
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    psi /= np.linalg.norm(psi)
    strings = rdm_strings(sites, n)
    m = len(sites)
    assert len(strings) == 4 ** m - 1 and len(set(strings)) == len(strings)
    assert all(len(w) == n and set(w) <= set("1xyz") and w != "1" * n for w in strings)
    assert all(all(w[s] == "1" for s in range(n) if s not in sites) for w in strings)
    # site s of the ket is index bit n - 1 - s
    codes = op_strings_by_bit(strings, np.arange(n)[::-1])
    vals = np.array([np.vdot(psi, kron_of(c) @ psi) for c in codes])
    rho = rdm_from_string_values(vals)
    assert rho.shape == (1, 1 << m, 1 << m)
    want = _partial_trace(psi, sites, n)
    err = np.abs(rho[0] - want).max()
    print("m = %d sites %s: max |rho - partial trace| = %.2e" % (m, sites, err))
    assert err <= 1e-14
    assert abs(np.trace(rho[0]) - 1.0) <= 1e-14 and np.abs(rho[0] - rho[0].conj().T).max() <= 1e-14
    two = rdm_from_string_values(np.stack([vals, vals], axis=1))
    assert two.shape == (2, 1 << m, 1 << m) and np.array_equal(two[0], rho[0]) and np.array_equal(two[1], rho[0])


def test_rdm_helper_argument_checks():
    for bad in ((), (0, 1, 2, 3), (1, 1), (5,), (-1,)):
        with pytest.raises(ValueError):
            rdm_strings(bad, 5)
    with pytest.raises(ValueError):
        rdm_from_string_values(np.zeros(4))
    with pytest.raises(ValueError):
        rdm_from_string_values(np.zeros((16, 3)))


def test_simulate_rare_strings_argument_checks():
    """Refused before a device is touched (this test runs without one)."""
    params = sweep_point_params(2, 25e3, "center_on", 1e-3, 5)
    with pytest.raises(ValueError):
        simulate_rare_strings(params, ["1x"])            # one letter per site
    with pytest.raises(ValueError):
        simulate_rare_strings(params, ["1xq"])           # outside the alphabet
    with pytest.raises(ValueError):
        simulate_rare_strings(params, [])
    with pytest.raises(ValueError):
        simulate_rare_strings(params, ["zzz"] * 65)      # above the cap
    with pytest.raises(ValueError):
        simulate_rare_strings(params, ["zzz"], psi0=np.ones(8), spins=np.ones((3, 2)))
    with pytest.raises(ValueError):
        simulate_rare_strings(params, ["zzz"], psi0=np.ones(4))


# ------------------------------------------------------------------------------ compiler resources
def test_string_kernels_use_no_scratch(tmp_path):
    """k_obs_strings<L> keeps its rows and |psi|^2 in registers and finds every in-tile partner in LDS
    (the table is read at run time: nothing indexed by it is a per-thread array); k_dense_obs_strings:
    13 tile sizes + 1, none with scratch or spills."""
    rows = _compile_resources(tmp_path, "dse_strings.hip")
    tiled = [k for k in rows if "k_obs_strings" in k[0]]
    dense = [k for k in rows if "k_dense_obs_strings" in k[0]]
    assert len(tiled) == 13 and len(dense) == 1, rows
    print(tiled + dense)
    assert all(sp == 0 and sc == 0 for _, sp, sc in tiled + dense), tiled + dense


def test_small_engine_string_variants_use_no_scratch(tmp_path):
    """k_small_str<N, *, *> and k_small_obs0_str<N, *, *>, N = 1..9: no spills, no scratch.  The kernels
    without the strings keep their names and their count."""
    rows = _compile_resources(tmp_path, "dse_small.hip")
    new = [k for k in rows if re.search(r"k_small(_obs0)?_strILi\d+ELb[01]ELb[01]EE", k[0])]
    ovl = [k for k in rows if re.search(r"k_small(_obs0)?_ovlILi\d+ELb[01]ELb[01]EE", k[0])]
    old = [k for k in rows if re.search(r"k_small(_obs0)?ILi\d+ELb[01]ELb[01]EE", k[0])]
    assert len(new) == 2 * 4 * 9 and len(ovl) == 2 * 4 * 9 and len(old) == 2 * 4 * 9, [k[0] for k in rows]
    bad = [k for k in new if k[1] != 0 or k[2] != 0]
    print("string variants with spills or scratch:", bad)
    assert not bad, bad
