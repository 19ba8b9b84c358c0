"""Host-side checks of the site-resolved observables (no device): the bit -> site mapping of
problem.site_traces_from_bits, the ABI version, and the ctypes mirror of dse_stats (whose
reserved13 became site_obs_problems in ABI 14)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from quantumsimulations_amd import _lib
from quantumsimulations_amd import problem as pb
from quantumsimulations_amd.sweep import sweep_point_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(n, n_t=4):
    """bit_traces[c, b, j] = 100 c + 10 b + j / 8: every entry names its own place."""
    c, b, j = np.meshgrid(np.arange(3), np.arange(n), np.arange(n_t), indexing="ij")
    return 100.0 * c + 10.0 * b + j / 8.0


@pytest.mark.parametrize("order", ["engine", "reference"])
def test_bits_to_sites_full_register(order):
    n = 5
    site_of_bit = np.arange(n) if order == "engine" else np.arange(n)[::-1]
    bt = _bits(n)
    out = pb.site_traces_from_bits(bt, site_of_bit, n, False, 0.0)
    assert out.shape == (3, n, 4) and out.dtype == np.float64
    for b in range(n):
        np.testing.assert_array_equal(out[:, site_of_bit[b]], bt[:, b])


@pytest.mark.parametrize("order", ["engine", "reference"])
@pytest.mark.parametrize("rare_z", [0.5, -0.5])
def test_bits_to_sites_reduced_register_fills_rare_row(order, rare_z):
    n_sites = 5
    n = n_sites - 1
    site_of_bit = np.arange(n) if order == "engine" else np.arange(n)[::-1]
    bt = _bits(n)
    out = pb.site_traces_from_bits(bt, site_of_bit, n_sites, True, rare_z)
    assert out.shape == (3, n_sites, 4)
    for b in range(n):
        np.testing.assert_array_equal(out[:, site_of_bit[b]], bt[:, b])
    assert np.all(out[2, n_sites - 1] == rare_z)
    assert np.all(out[0, n_sites - 1] == 0.0) and np.all(out[1, n_sites - 1] == 0.0)


def test_bits_to_sites_hook_shape_and_errors():
    out = pb.site_traces_from_bits(np.arange(9.0).reshape(3, 3), [2, 0, 1], 3, False, 0.0)  # (3, n)
    np.testing.assert_array_equal(out[:, 2], [0.0, 3.0, 6.0])
    with pytest.raises(ValueError):
        pb.site_traces_from_bits(np.zeros((3, 3, 2)), [0, 1], 3, False, 0.0)
    with pytest.raises(ValueError):
        pb.site_traces_from_bits(np.zeros((3, 3, 2)), [0, 1, 1], 3, False, 0.0)
    with pytest.raises(ValueError):  # a reduced register holds n_sites - 1 bits
        pb.site_traces_from_bits(np.zeros((3, 3, 2)), [0, 1, 2], 3, True, 0.5)


@pytest.mark.parametrize("order", ["engine", "reference"])
@pytest.mark.parametrize("variant,reduce", [("center_off", True), ("center_off", False), ("shell_off", True)])
def test_bits_to_sites_with_built_problems(order, variant, reduce):
    """Problem.site_of_bit of both register orders: bit b lands on the site it was built from."""
    prob = pb.build_problem(sweep_point_params(6, 25e3, variant, 1e-3, 5), order=order, reduce=reduce)
    assert prob.reduced == (variant == "center_off" and reduce)
    bt = _bits(prob.n_qubits, 5)
    out = pb.site_traces_from_bits(bt, prob.site_of_bit, prob.n_sites, prob.reduced, prob.rare_z_const)
    assert out.shape == (3, 7, 5)
    for b in range(prob.n_qubits):
        s = b if order == "engine" else prob.n_qubits - 1 - b
        np.testing.assert_array_equal(out[:, s], bt[:, b])
    if prob.reduced:
        assert np.all(out[2, 6] == prob.rare_z_const) and prob.rare_z_const in (0.5, -0.5)
        assert np.all(out[:2, 6] == 0.0)


def test_abi_version_is_14():
    assert _lib.DSE_ABI_VERSION == 14
    with open(os.path.join(ROOT, "include", "dse.h")) as f:
        assert "#define DSE_ABI_VERSION 14" in f.read()
    assert "dse_site_observables" in _lib.EXPORTED and "dse_get_site_obs" in _lib.EXPORTED


def _host_cc():
    for c in (os.environ.get("CC"), "cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        path = shutil.which(c) if c else None
        if path:
            return path
    pytest.fail("no host C compiler found (cc, gcc, clang)")


def test_dse_stats_ctypes_mirror_has_the_c_size(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dse.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(dse_stats), offsetof(dse_stats, site_obs_problems)); return 0; }\n')
    exe = tmp_path / "sz"
    res = subprocess.run([_host_cc(), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    size, off = (int(x) for x in run.stdout.split())
    assert ctypes.sizeof(_lib.DseStats) == size
    assert _lib.DseStats.site_obs_problems.offset == off
    assert "reserved13" not in dict(_lib.DseStats._fields_)


def test_site_kernel_keeps_its_rows_out_of_scratch(tmp_path):
    """k_obs_sites<L> reads a register bit's partner row from the thread's own registers with the
    rows chosen at compile time: the bit loop must unroll around the wave shuffles (a loop with an
    early exit did not, and put the 16 rows in scratch).  13 tile sizes, none with scratch or spills."""
    from test_build import CSRC, _hipcc, _resources
    res = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
         "--cuda-device-only", "-c", os.path.join(CSRC, "dse_kernels.hip"), "-o",
         str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    kernels = [k for k in _resources(res.stderr) if "k_obs_sites" in k[0]]
    assert len(kernels) == 13, kernels
    assert all(sp == 0 and sc == 0 for _, sp, sc in kernels), kernels
