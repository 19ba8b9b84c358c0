"""Host-side checks of the overlaps with reference states (no device): the header / EXPORTED entries,
dse_has_feature, the reference-order <-> engine-order mapping that simulate_rare_overlaps applies to
its references, and the compiler's resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.dipolar_ensemble_with_rare import engine_to_reference_state, reference_to_engine_state
from quantumsimulations_amd.sweep import sweep_point_params
from test_pair_obs_host import _compile_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("dse_set_overlap_refs", "dse_overlap_refs", "dse_overlaps", "dse_get_overlaps",
               "dse_overlap_outputs", "dse_overlap_problems")


# ------------------------------------------------------------------------------ ABI surface
def test_header_declares_and_lib_exports_the_entries():
    with open(os.path.join(ROOT, "include", "dse.h")) as f:
        text = f.read()
    L = _lib.lib()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in _lib.EXPORTED, name
        assert hasattr(L, name), name
    assert '"overlap_obs"' in text
    assert re.search(r"#define DSE_MAX_OVERLAP_REFS 16\b", text) and _lib.DSE_MAX_OVERLAP_REFS == 16
    # the version numbers and dse_stats did not move: the addition is discovered by name
    assert "#define DSE_ABI_VERSION 14" in text and "#define DSE_ABI_MINOR 1" in text
    assert _lib.DseStats._fields_[-1][0] == "custom_init_problems"


def test_has_feature():
    L = _lib.lib()
    assert L.dse_has_feature(b"overlap_obs") == 1
    assert L.dse_has_feature(b"pair_obs") == 1 and L.dse_has_feature(b"site_obs") == 1
    assert L.dse_has_feature(b"overlap") == 0 and L.dse_has_feature(ctypes.c_char_p(None)) == 0
    assert _lib.has_feature("overlap_obs")


def test_null_context_and_bad_ids_are_refused():
    L = _lib.lib()
    assert L.dse_set_overlap_refs(None, 0, 0, None) == _lib.DSE_ERR_ARG
    assert L.dse_overlap_refs(None, 0) == _lib.DSE_ERR_ARG
    assert L.dse_overlap_outputs(None) == _lib.DSE_ERR_ARG and L.dse_overlap_problems(None) == _lib.DSE_ERR_ARG
    assert L.dse_get_overlaps(None, 0, None) == _lib.DSE_ERR_ARG and L.dse_overlaps(None, 0, None, None) == _lib.DSE_ERR_ARG


# ------------------------------------------------------------------------------ reference order <-> engine order
def _numpy_map(psi_ref, sob):
    """Amplitude by amplitude: reference index r has site s at bit n - 1 - s; the register index holds
    site sob[b] at bit b."""
    n = len(sob)
    out = np.empty_like(psi_ref)
    for x in range(1 << n):
        r = 0
        for b in range(n):
            r |= ((x >> b) & 1) << (n - 1 - int(sob[b]))
        out[x] = psi_ref[r]
    return out


@pytest.mark.parametrize("n_sea", [2, 5])
@pytest.mark.parametrize("variant", ["center_off", "center_on", "shell_off"])
def test_reference_to_engine_mapping_of_refs(n_sea, variant):
    """N = 3 and 6 spins: a (K, 2^N) set of reference kets row by row, against the index arithmetic; the
    overlap of two kets does not depend on the order they are written in."""
    prob = pb.build_problem(sweep_point_params(n_sea, 25e3, variant, 1e-3, 5), order="engine", reduce=False)
    n = prob.n_qubits
    assert n == n_sea + 1
    rng = np.random.default_rng(10 * n_sea + len(variant))
    refs = rng.standard_normal((3, 1 << n)) + 1j * rng.standard_normal((3, 1 << n))
    psi = rng.standard_normal(1 << n) + 1j * rng.standard_normal(1 << n)
    refs_eng = np.stack([reference_to_engine_state(v, prob.site_of_bit) for v in refs])
    for k in range(3):
        np.testing.assert_array_equal(refs_eng[k], _numpy_map(refs[k], prob.site_of_bit))
        np.testing.assert_array_equal(engine_to_reference_state(refs_eng[k], prob.site_of_bit), refs[k])
    psi_eng = reference_to_engine_state(psi, prob.site_of_bit)
    a = np.array([np.vdot(v, psi) for v in refs])
    b = np.array([np.vdot(v, psi_eng) for v in refs_eng])
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-13)


def test_simulate_rare_overlaps_argument_checks():
    from quantumsimulations_amd.dipolar_ensemble_with_rare import simulate_rare_overlaps
    params = sweep_point_params(2, 25e3, "center_on", 1e-3, 5)
    with pytest.raises(ValueError):
        simulate_rare_overlaps(params, "final")
    with pytest.raises(ValueError):
        simulate_rare_overlaps(params, np.ones((2, 4)))
    with pytest.raises(ValueError):
        simulate_rare_overlaps(params, "initial", psi0=np.ones(8), spins=np.ones((3, 2)))


def test_problem_bytes_counts_the_references():
    from quantumsimulations_amd.engine import problem_bytes
    prob = pb.build_problem(sweep_point_params(6, 25e3, "center_on", 1e-3, 5), order="engine", reduce=False)
    assert problem_bytes(prob, overlap_refs=3) - problem_bytes(prob) == 3 * 16.0 * (1 << prob.n_qubits)
    assert problem_bytes(prob, True, 1) - problem_bytes(prob, True) == 16.0 * (1 << prob.n_qubits)


# ------------------------------------------------------------------------------ compiler resources
def test_tile_overlap_kernel_uses_no_scratch(tmp_path):
    """k_obs_overlap<L> keeps psi's rows in registers and streams the references past them: 13 tile
    sizes, none with scratch or spills."""
    rows = _compile_resources(tmp_path, "dse_overlap.hip")
    tiled = [k for k in rows if "k_obs_overlap" in k[0]]
    assert len(tiled) == 13, rows
    print(tiled)
    assert all(sp == 0 and sc == 0 for _, sp, sc in tiled), tiled


def test_dense_overlap_kernel_uses_no_scratch(tmp_path):
    rows = _compile_resources(tmp_path, "dse_dense.hip")
    dense = [k for k in rows if "k_dense_obs_overlap" in k[0]]
    assert len(dense) == 1, rows
    assert all(sp == 0 and sc == 0 for _, sp, sc in dense), dense


def test_small_engine_overlap_variants_use_no_scratch(tmp_path):
    """k_small_ovl<N, *, *> and k_small_obs0_ovl<N, *, *>, N = 1..9: no spills, no scratch (they take the
    prologue of the pair-sum variants: the state loaded in a loop of its own).  The kernels without the
    overlaps keep their names and their count."""
    rows = _compile_resources(tmp_path, "dse_small.hip")
    new = [k for k in rows if re.search(r"k_small(_obs0)?_ovlILi\d+ELb[01]ELb[01]EE", k[0])]
    old = [k for k in rows if re.search(r"k_small(_obs0)?ILi\d+ELb[01]ELb[01]EE", k[0])]
    assert len(new) == 2 * 4 * 9 and len(old) == 2 * 4 * 9, [k[0] for k in rows]
    bad = [k for k in new if k[1] != 0 or k[2] != 0]
    print("overlap variants with spills or scratch:", bad)
    assert not bad, bad
