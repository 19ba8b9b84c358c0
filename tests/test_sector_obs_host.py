"""Magnetisation-sector populations (feature "sector_obs"): everything that needs no device.  The ABI
surface, the layout and its refusals, the Python helpers (sector_masks_by_bit, mqc_intensities,
sector_moments, the argument checks of simulate_rare_sectors) and the compiler's resource report for
the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd.dipolar_ensemble_with_rare import (mqc_intensities, sector_masks_by_bit, sector_moments,
                                                               simulate_rare_sectors)
from quantumsimulations_amd.sweep import sweep_point_params
from test_pair_obs_host import _compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("dse_sector_layout", "dse_set_sectors", "dse_sectors", "dse_sector_units", "dse_sector_values",
               "dse_get_sectors", "dse_sector_outputs", "dse_sector_problems")


def _layout(n, masks, k=None, offsets=True):
    x = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, 3)
    k = x.shape[0] if k is None else k
    off = (ctypes.c_int * (max(k, 0) + 1))()
    rc = _lib.lib().dse_sector_layout(n, k, _lib.u64ptr(x), off if offsets else None)
    return rc, list(off)


# ------------------------------------------------------------------------------ ABI surface
def test_header_declares_and_lib_exports_the_entries():
    with open(os.path.join(ROOT, "include", "dse.h")) as f:
        text = f.read()
    L = _lib.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in _lib.EXPORTED and hasattr(L, name), name
    assert "#define DSE_MAX_SECTOR_SETS 16" in text and _lib.DSE_MAX_SECTOR_SETS == 16
    assert "#define DSE_ABI_VERSION 14" in text or _lib.DSE_ABI_VERSION == L.dse_abi_version()
    assert L.dse_abi_version() == _lib.DSE_ABI_VERSION and L.dse_abi_minor() == 1
    assert _lib.DseStats._fields_[-1][0] == "custom_init_problems"


def test_has_feature():
    L = _lib.lib()
    assert L.dse_has_feature(b"sector_obs") == 1 and L.dse_has_feature(b"sector") == 0
    assert L.dse_has_feature(b"op_strings") == 1 and L.dse_has_feature(b"overlap_obs") == 1
    assert _lib.has_feature("sector_obs")


def test_null_context_is_refused():
    L = _lib.lib()
    m = np.array([[1, 0, 0]], dtype=np.uint64)
    out = np.zeros(4)
    assert L.dse_set_sectors(None, 0, 1, _lib.u64ptr(m)) == _lib.DSE_ERR_ARG
    assert L.dse_sectors(None, 0) == _lib.DSE_ERR_ARG and L.dse_sector_units(None, 0) == _lib.DSE_ERR_ARG
    assert L.dse_sector_values(None, 0, _lib.ptr(out), _lib.ptr(out)) == _lib.DSE_ERR_ARG
    assert L.dse_get_sectors(None, 0, _lib.ptr(out)) == _lib.DSE_ERR_ARG
    assert L.dse_sector_outputs(None) == _lib.DSE_ERR_ARG and L.dse_sector_problems(None) == _lib.DSE_ERR_ARG


# ------------------------------------------------------------------------------ the layout
def test_layout_offsets():
    rc, off = _layout(5, [[0b00011, 0b00100, 0b00100], [0, 0, 0], [0b11111, 0, 0], [0, 0b10001, 0b10000]])
    assert rc == 11 and off == [0, 3, 4, 10, 11]
    assert _layout(5, [[0b11111, 0, 0]], offsets=False)[0] == 6           # offsets may be null
    rc, off = _layout(34, [[(1 << 34) - 1, 0, 0]] * 16)                    # the widest register, the cap
    assert rc == 16 * 35 and off == [35 * k for k in range(17)]
    assert _layout(1, [[1, 0, 0]])[0] == 2 and _layout(1, [[0, 1, 1]])[0] == 1
    u, o = _lib.sector_layout(5, [[3, 4, 4], [0, 0, 0]])
    assert u == 4 and o.tolist() == [0, 3, 4]
    assert _lib.sector_layout(3, [7, 0, 0])[0] == 4                        # one set as three numbers


def test_layout_refusals():
    ok = [[1, 2, 2]]
    assert _layout(4, ok)[0] == 2
    for n in (0, -1, 35):                                  # n outside 1..DSE_MAX_QUBITS
        assert _layout(n, ok)[0] == _lib.DSE_ERR_ARG, n
    assert _layout(4, ok, k=0)[0] == _lib.DSE_ERR_ARG      # k outside 1..16
    assert _layout(4, ok, k=-1)[0] == _lib.DSE_ERR_ARG
    assert _layout(4, ok * 17)[0] == _lib.DSE_ERR_ARG
    assert _layout(4, [[1 << 4, 0, 0]])[0] == _lib.DSE_ERR_ARG       # a counted bit at n
    assert _layout(4, [[1, 1 << 4, 0]])[0] == _lib.DSE_ERR_ARG       # a selecting bit at n
    assert _layout(4, [[1, 2, 1 << 63]])[0] == _lib.DSE_ERR_ARG      # a value bit far above n
    assert _layout(4, [[3, 2, 0]])[0] == _lib.DSE_ERR_ARG            # m & cm != 0
    assert _layout(4, [[1, 2, 4]])[0] == _lib.DSE_ERR_ARG            # cv & ~cm != 0
    assert _layout(4, ok + [[3, 2, 0]])[0] == _lib.DSE_ERR_ARG       # in a later set
    assert _lib.lib().dse_sector_layout(4, 1, None, None) == _lib.DSE_ERR_ARG  # null masks
    for bad in ([[1, 2]], [[3, 2, 0]], [[-1, 0, 0]], []):
        with pytest.raises(ValueError):
            _lib.sector_layout(4, bad)


# ------------------------------------------------------------------------------ Python helpers
def test_sector_masks_by_bit_under_a_permutation():
    sob = np.array([2, 0, 3, 1])  # bit b holds site sob[b]
    out = sector_masks_by_bit(["w.ab", "wwww", "....", "bawa"], sob)
    assert out.dtype == np.uint64 and out.shape == (4, 3)
    # "w.ab": site 0 counted (bit 1), site 2 up (bit 0), site 3 down (bit 2)
    assert out[0].tolist() == [0b0010, 0b0101, 0b0100]
    assert out[1].tolist() == [0b1111, 0, 0] and out[2].tolist() == [0, 0, 0]
    # "bawa": site 0 down (bit 1), site 1 up (bit 3), site 2 counted (bit 0), site 3 up (bit 2)
    assert out[3].tolist() == [0b0001, 0b1110, 0b0010]
    assert sector_masks_by_bit("w.ab", sob).tolist() == [out[0].tolist()]
    assert _lib.sector_layout(4, out)[0] == 2 + 5 + 1 + 2
    with pytest.raises(ValueError):
        sector_masks_by_bit(["w.a"], sob)            # a wrong length
    with pytest.raises(ValueError):
        sector_masks_by_bit(["w.az"], sob)           # a letter outside the alphabet
    with pytest.raises(ValueError):
        sector_masks_by_bit(["wwww"] * 17, sob)      # 17 sets
    with pytest.raises(ValueError):
        sector_masks_by_bit([], sob)                 # an empty list
    with pytest.raises(ValueError):
        sector_masks_by_bit(["wwww"], np.array([0, 0, 1, 2]))


def _weights(n):
    return np.array([bin(x).count("1") for x in range(1 << n)])


def test_mqc_intensities_against_brute_force():
    """n = 6, a random state: I_q = sum over pairs (x, y) with w(x) - w(y) = q of |psi_x|^2 |psi_y|^2."""
    n = 6
    rng = np.random.default_rng(66)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    psi /= np.linalg.norm(psi)
    p2, w = np.abs(psi) ** 2, _weights(n)
    P = np.bincount(w, p2, minlength=n + 1)
    brute = np.zeros(2 * n + 1)
    for x in range(1 << n):
        for y in range(1 << n):
            brute[w[x] - w[y] + n] += p2[x] * p2[y]
    I = mqc_intensities(P[None, :])
    assert I.shape == (1, 2 * n + 1)
    err = np.abs(I[0] - brute).max()
    print(f"mqc_intensities against the brute force: {err:.2e} (bound 1e-14)")
    assert err < 1e-14
    assert abs(I.sum() - 1.0) < 1e-14 and np.abs(I[0] - I[0, ::-1]).max() < 1e-16
    assert mqc_intensities(P).shape == (1, 2 * n + 1)       # one time
    two = mqc_intensities(np.stack([P, P[::-1]]))
    assert two.shape == (2, 2 * n + 1) and np.array_equal(two[0], I[0])
    with pytest.raises(ValueError):
        mqc_intensities(np.zeros((2, 3, 4)))


def test_sector_moments_against_numpy():
    """The mean of M under the bins of a mask m equals popcount(m)/2 - sum_{b in m} <Iz_b>; the higher
    columns are the central moments of popcount(x & m) under |psi_x|^2."""
    n = 7
    rng = np.random.default_rng(77)
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    p2 = np.abs(psi) ** 2 / np.vdot(psi, psi).real
    x = np.arange(1 << n)
    for m in ((1 << n) - 1, 0b1010011):
        bits = [b for b in range(n) if m >> b & 1]
        M = sum((x >> b) & 1 for b in bits)
        P = np.bincount(M, p2, minlength=len(bits) + 1)
        iz = sum(np.sum(p2 * (0.5 - ((x >> b) & 1))) for b in bits)
        mom = sector_moments(P, 4)
        assert mom.shape == (1, 5)
        assert abs(mom[0, 0] - 1.0) < 1e-14 and abs(mom[0, 1] - (len(bits) / 2 - iz)) < 1e-14
        mean = np.sum(p2 * M)
        for r in (2, 3, 4):
            assert abs(mom[0, r] - np.sum(p2 * (M - mean) ** r)) < 1e-13, r
    half = sector_moments(0.25 * P, 2)                       # a conditioned set: the weight, then means given it
    assert abs(half[0, 0] - 0.25) < 1e-15 and abs(half[0, 1] - mom[0, 1]) < 1e-14 and abs(half[0, 2] - mom[0, 2]) < 1e-14
    assert sector_moments(np.zeros((3, 4)), 2).tolist() == [[0.0, 0.0, 0.0]] * 3
    with pytest.raises(ValueError):
        sector_moments(P, 0)


def test_simulate_rare_sectors_argument_checks():
    """Refused before a device is touched (this test runs without one)."""
    params = sweep_point_params(2, 25e3, "center_on", 1e-3, 5)
    with pytest.raises(ValueError):
        simulate_rare_sectors(params, ["www"], psi0=np.ones(8), spins=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        simulate_rare_sectors(params, [])
    with pytest.raises(ValueError):
        simulate_rare_sectors(params, ["www"] * 17)
    with pytest.raises(ValueError):
        simulate_rare_sectors(params, ["ww"])
    with pytest.raises(ValueError):
        simulate_rare_sectors(params, ["wxw"])


# ------------------------------------------------------------------------------ compiler resources
def test_sector_kernels_use_no_scratch(tmp_path):
    """k_obs_sectors<L> keeps |psi|^2 of its rows in registers and merges bins under compile-time
    indices; k_dense_obs_sectors adds to a register vector under compile-time indices: 13 tile sizes + 1,
    none with scratch or spills."""
    rows = _compile_resources(tmp_path, "dse_sectors.hip")
    tiled = [k for k in rows if "k_obs_sectors" in k[0]]
    dense = [k for k in rows if "k_dense_obs_sectors" in k[0]]
    assert len(tiled) == 13 and len(dense) == 1, rows
    print(tiled + dense)
    assert all(sp == 0 and sc == 0 for _, sp, sc in tiled + dense), tiled + dense


def test_small_engine_sector_variants_use_no_scratch(tmp_path):
    """k_small_sec<N, *, *> and k_small_obs0_sec<N, *, *>, N = 1..9: no spills, no scratch.  The three
    older forms keep their names and their count."""
    rows = _compile_resources(tmp_path, "dse_small.hip")
    new = [k for k in rows if re.search(r"k_small(_obs0)?_secILi\d+ELb[01]ELb[01]EE", k[0])]
    strs = [k for k in rows if re.search(r"k_small(_obs0)?_strILi\d+ELb[01]ELb[01]EE", k[0])]
    ovl = [k for k in rows if re.search(r"k_small(_obs0)?_ovlILi\d+ELb[01]ELb[01]EE", k[0])]
    old = [k for k in rows if re.search(r"k_small(_obs0)?ILi\d+ELb[01]ELb[01]EE", k[0])]
    assert len(new) == 72 and len(strs) == 72 and len(ovl) == 72 and len(old) == 72, [k[0] for k in rows]
    bad = [k for k in new if k[1] != 0 or k[2] != 0]
    print("sector variants with spills or scratch:", bad)
    assert not bad, bad
