"""Build-level check of the leap path's kernels (CPU only: hipcc cross-compiles for gfx950), in the manner of
tests/test_build.py: k_leap_real, the real_body instantiation with the LEAP flag (component 0 alone, its own
rows and degree; the register file is as full as k_real<0>'s, and its row degrees sit in scalar registers to
fit), and the path's two small kernels k_leap_combine and k_leap_init must not spill or use scratch."""
import os
import subprocess

from test_build import CSRC, ROOT, _hipcc, _resources


def test_leap_kernels_do_not_spill(tmp_path):
    res = subprocess.run(
        [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "--cuda-device-only",
         "-c", os.path.join(CSRC, "dse_real.hip"), "-o", str(tmp_path / "real.o"), "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = _resources(res.stderr)
    for name in ("k_leap_real", "k_leap_combine", "k_leap_init"):
        kernels = [k for k in rows if name in k[0]]
        assert len(kernels) == 1, (name, rows)
        assert all(sp == 0 and sc == 0 for _, sp, sc in kernels), kernels
