#!/usr/bin/env python3
"""Hard pulses (dse_apply_pulse) against a device-to-device copy of the same buffer size.

    python tools/bench_pulse.py [--n 28] [--n-host 24] [--reps 10] [--out FILE]

One pass of k_pulse reads and writes the state once, 32 B per amplitude: what a device-to-device
copy of the state moves.  For a register of --n qubits the tool times that copy with torch (HIP
events, same device, same process) and four pulses with the engine's own HIP events
(Engine.pulse_stats): one spin on bit 0, one spin on the top bit, z rotations of every spin
(diagonal matrices: one pass, no LDS traffic) and a rotation of every spin.  It prints one JSON
line per pulse with the passes, the time per pass, its GB/s and the fraction of the copy's rate,
then the wall time of the host round trip the call replaces at --n-host qubits: the state to the
host, numpy's per-bit contraction, the state back (Engine.initial_state, numpy,
Engine.set_initial_state), beside the device pulse at the same size.  --out also writes the
lines to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from quantumsimulations_amd import problem as pb  # noqa: E402
from quantumsimulations_amd.dipolar_ensemble_with_rare import rotation_matrices  # noqa: E402
from quantumsimulations_amd.engine import Engine  # noqa: E402


def register(n):
    """Tables of an n-qubit register (the pulse reads none of them)."""
    return pb.Problem(n, np.linspace(1e3, 2e3, n), np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, 4)), 0.0, 0,
                      (1 << (n - 1)) - 1, n - 1, 0.0, np.arange(n), n, False, "engine")


def flat_state(n):
    v = np.empty(1 << n, dtype=np.complex128)
    v[:] = (0.6 + 0.8j) * 2.0 ** (-0.5 * n)
    return v


def pulses(n):
    rng = np.random.default_rng(7)
    rot = rng.standard_normal((n, 3))
    one = np.zeros((n, 3))
    eye = np.tile(np.eye(2, dtype=complex), (n, 1, 1))
    bit0, top = eye.copy(), eye.copy()
    bit0[0] = rotation_matrices(rot[:1])[0]
    top[n - 1] = rotation_matrices(rot[1:2])[0]
    one[:, 2] = rot[:, 2]
    return {"one spin, bit 0": bit0, f"one spin, bit {n - 1}": top, "z rotation of every spin": rotation_matrices(one),
            "rotation of every spin": rotation_matrices(rot)}


def np_pulse(psi, mats):
    n = len(mats)
    for b in range(n):
        if np.array_equal(mats[b], np.eye(2)):
            continue
        v = psi.reshape(1 << (n - 1 - b), 2, 1 << b)
        psi = np.tensordot(mats[b], v, axes=(1, 1)).transpose(1, 0, 2).reshape(-1)
    return psi


def copy_rate(n, reps):
    """GB/s of torch's device-to-device copy of 2^n complex128 (read + write counted)."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_pulse needs a GPU")
    src = torch.zeros(1 << n, dtype=torch.complex128, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    del src, dst
    torch.cuda.empty_cache()
    med = float(np.median(ms))
    return 32.0 * (1 << n) / (med * 1e-3) / 1e9, med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=28)
    ap.add_argument("--n-host", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    copy_gbs, copy_ms = copy_rate(a.n, a.reps)
    emit({"what": "device-to-device copy (torch)", "qubits": a.n, "ms": copy_ms, "gbs": copy_gbs})
    with Engine(0) as eng:
        pid = eng.add(register(a.n))
        eng.set_initial_state(pid, flat_state(a.n))
        for name, mats in pulses(a.n).items():
            for _ in range(2):
                eng.apply_pulse(pid, mats)
            ms, passes = [], 0
            for _ in range(a.reps):
                eng.apply_pulse(pid, mats)
                st = eng.pulse_stats()
                passes = st["passes"]
                ms.append(st["ms"] / max(passes, 1))
            med = float(np.median(ms))
            gbs = 32.0 * (1 << a.n) / (med * 1e-3) / 1e9
            emit({"what": name, "qubits": a.n, "passes": passes, "ms_per_pass": med, "ms_per_pass_min": float(np.min(ms)),
                  "ms_per_pass_max": float(np.max(ms)), "gbs_per_pass": gbs, "fraction_of_copy": gbs / copy_gbs})
        # the host round trip a pulse replaces
        eng.clear()
        n = a.n_host
        pid = eng.add(register(n))
        eng.set_initial_state(pid, flat_state(n))
        for name, mats in pulses(n).items():
            if name not in ("one spin, bit 0", "rotation of every spin"):
                continue
            t0 = time.perf_counter()
            v = eng.initial_state(pid)
            t1 = time.perf_counter()
            v = np_pulse(v, mats)
            t2 = time.perf_counter()
            eng.set_initial_state(pid, v)
            t3 = time.perf_counter()
            eng.apply_pulse(pid, mats)  # warm
            t4 = time.perf_counter()
            eng.apply_pulse(pid, mats)
            t5 = time.perf_counter()
            emit({"what": "host round trip: " + name, "qubits": n, "to_host_s": t1 - t0, "numpy_s": t2 - t1,
                  "to_device_s": t3 - t2, "round_trip_s": t3 - t0, "apply_pulse_wall_s": t5 - t4,
                  "apply_pulse_kernel_ms": eng.pulse_stats()["ms"]})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
