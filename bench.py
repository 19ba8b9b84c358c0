#!/usr/bin/env python3
"""Benchmark: N = 14 sea-detuning sweep on MI355X (BASELINE.json metric, config 3).

One "step" = one full batch of the hot path: the 64-detuning x 3-variant sweep
(192 independent evolutions, n_sea = 13 + 1 rare = 14 qubits) propagated over the
head-to-head grid t_final = 1e-3 s, 101 output times, with all seven observable
traces computed.  Problem tables are uploaded before the timed region (inputs
resident in HBM); each timed step resets every state to psi0 and runs the whole
evolution (Chebyshev interval kernels + observable reductions) to t_final.

value = detuning-points / hour over the whole job (points of all ranks / max rank time).
Multi-GPU (torchrun, one process per GPU), no data-path collective (evolutions are independent):
  --scaling strong (default; BASELINE config 3 as stated: ONE 64-point sweep over the N GPUs):
      rank r of N takes the detunings j = r (mod N) of linspace(0, 150 kHz, 64) -- 64/N points each;
  --scaling weak: rank r takes j = r (mod N) of linspace(0, 150 kHz, 64 N) -- 64 points per rank.

A plain run (no --full) sets up, warms up, times the --steps steps, writes --dump-outputs if given
and prints the line: the contract's fields, `config` and `roofline` (both from the timed steps' own
counters and HIP events, no run of their own).  Every other leg below runs only with --full, where
the --no-* options still drop single legs.
  --dump-outputs DIR  after the timed steps: DIR/observables.npy, what the last timed step returned
                 to its caller (float64 [evolution, 7 observables, 101 output times]; with N > 1 ranks
                 observables_rank<r>.npy each); the inputs are the same from run to run

Extra fields of the JSON line:
  roofline       the dominant kernel (k_interval, HIP events around every launch on its own
                 stream inside the timed region) priced as SURVEY.md §8(d) prices a fused
                 Chebyshev term: 80 B per amplitude per term against the 8 TB/s HBM peak; FP64
                 rate alongside; "traffic" = the counter-measured bytes per launch
                 (profiles/<round>/bench_pmc_traffic.json)
  full_sweep     the reference's own grid (t_final 30 s, 20000 outputs, sweep_sea_detuning.py:
                 1223-1224) on the same 64 x 3 evolutions: BASELINE's "(full sweep)" figure (`value`
                 is the 1 ms head-to-head grid), by the fastest engine whose stated accuracy at
                 t = 30 s meets north_star's 1e-8 -- the dense eigen-propagator timed on the whole
                 sweep; the Chebyshev kernels (16 intervals x 3, extrapolated) beside it
  cpu_baseline   rank 0, N = 1 only: the QuTiP-5 sesolve equivalent (oracle/cpu_bench.py) on
                 the host cores, 1 core, this job's CPU share and a node-wide estimate, run
                 before the GPU is touched
  config2        rank 0, N = 1 only: BASELINE config 2 (one N = 12 evolution, 2 ms / 201 outputs)
                 through the drop-in simulate_rare, and the unmodified caller's three serial
                 calls per point at N = 14
  reference_default  rank 0, N = 1 only: the reference's own default run (N = 7, 13 detunings x
                 3 variants, 30 s / 20 000 outputs) timed whole on the dense eigen-propagator
  large_register rank 0, N = 1 only: config 5 on one GPU (N = 30, Walsh-Hadamard engine) against
                 the HBM roofline, with exact-invariant checks (norm, energy); --no-large skips it
  strong_split   rank 0, N = 1 only: the 2-, 4- and 8-GPU strong splits predicted on one GPU -- each
                 of the ranks' shards (64/N points) timed alone on this GPU; the heaviest shard's
                 wall time is the N-GPU step time (ms/ODE-step beside it)
The stdout line is a compact summary (< 4 KB: the driver keeps the tail of stdout); the full record,
per-shard arrays and tolerance detail included, goes to --detail (default gpurun_out/bench_detail.json).
roofline.on_chip also carries the clock measured under this load (profiles/<round>/clock_under_load.json,
tools/clock_probe.sh).  DSE_BENCH_SET=key=value,... sets engine options on the sweep's context (A/Bs).
  partitioned    N = 2, 4, 8 only, after the timed sweep: config 5 with the N = 30 register split
                 over the N ranks (tools/bench_partitioned.py as a child process per rank, RCCL
                 index-swap all-to-all over xGMI): ms per H application, exchanged bytes per rank,
                 norm check; bounded by a timeout, reported (never raised) on failure
"""
from __future__ import annotations

import argparse
import json
import os
import re
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0           # MI355X HBM3E spec (MI355X_MICROARCH.md)
FP64_PEAK_TFLOPS = 78.6         # MI355X FP64 vector spec
N_SEA = 13
N_DET = 64
T_FINAL = 1e-3
STEPS_T = 101
DELTA_MAX = 150_000.0


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beside the timed sweep (CPU baseline, 30 s grid, strong-split "
                    "predictions, config 2, reference default, config 5; N > 1: the partitioned register)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the observables the last timed step returned to DIR/observables.npy")
    ap.add_argument("--tile-bits", type=int, default=int(os.environ.get("DSE_TILE_BITS", "13")))
    ap.add_argument("--streams", type=int, default=int(os.environ.get("DSE_STREAMS", "4")))
    ap.add_argument("--cpu-fraction", type=float, default=float(os.environ.get("DSE_CPU_FRACTION", "0.25")),
                    help="share of the 1 ms grid each CPU-baseline evolution integrates")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--streaming", action="store_true", help="per-term streaming kernels instead of "
                    "the persistent interval kernel")
    ap.add_argument("--outputs-per-launch", type=int, default=int(os.environ.get("DSE_OUTPUTS_PER_LAUNCH", "2")),
                    help="persistent mode: output times propagated per launch from one Chebyshev series")
    ap.add_argument("--mixed-launch", type=int, default=int(os.environ.get("DSE_MIXED_LAUNCH", "1")),
                    help="persistent mode: 1- and 2-tile problems in one launch per interval (1, default) "
                    "or one stream each (0)")
    ap.add_argument("--real", type=int, default=int(os.environ.get("DSE_REAL", "0")),
                    help="real-component mode (dse_real.hip) for the 13/14-qubit registers (0: k_interval)")
    ap.add_argument("--span-tile", type=int, default=int(os.environ.get("DSE_SPAN_TILE", "-1")),
                    help="k_span tile bits for the sweep's registers (-1 auto: only when all tiles fit at once; 0 never)")
    ap.add_argument("--obs-overlap", type=int, default=int(os.environ.get("DSE_OBS_OVERLAP", "0")),
                    help="persistent mode: observables on a second stream per lane (1)")
    ap.add_argument("--n-sea", type=int, default=N_SEA)
    ap.add_argument("--n-det", type=int, default=N_DET)
    ap.add_argument("--scaling", choices=("strong", "weak"), default=os.environ.get("DSE_BENCH_SCALING", "strong"),
                    help="strong: one n-det sweep split over the ranks (BASELINE config 3); weak: n-det per rank")
    ap.add_argument("--no-shard8", action="store_true", help="skip the 8-GPU strong-split prediction leg")
    ap.add_argument("--no-large", action="store_true", help="skip the config-5 single-GPU leg")
    ap.add_argument("--no-full", action="store_true", help="skip the reference-grid (30 s) leg")
    ap.add_argument("--full-intervals", type=int, default=16,
                    help="output intervals of the 30 s reference grid timed by the full-sweep leg")
    ap.add_argument("--full-repeats", type=int, default=3,
                    help="timed runs of those intervals (their spread is reported)")
    ap.add_argument("--no-config2", action="store_true", help="skip the config-2 / serial-caller leg")
    ap.add_argument("--no-refdefault", action="store_true",
                    help="skip the reference-default (N = 7, 30 s grid) leg")
    ap.add_argument("--partitioned-timeout", type=float, default=180.0,
                    help="N > 1: seconds allowed for the config-5 partitioned leg (child processes)")
    ap.add_argument("--detail", default=os.environ.get("DSE_BENCH_DETAIL", os.path.join("gpurun_out", "bench_detail.json")),
                    help="file for the full record (per-shard arrays, tolerance detail); '' for none -- the "
                    "stdout JSON line is its compact summary")
    ap.add_argument("--cpu-cores", type=int, default=int(os.environ.get("DSE_CPU_CORES", "0")),
                    help="worker processes of the all-core CPU leg (0: this process's CPU share)")
    return ap.parse_args(argv)


# rocprofv3 FETCH_SIZE / WRITE_SIZE passes over this bench command (tools/gpu.sh traffic +
# tools/pmc_summary.py), newest round first
PMC_TRAFFIC = [os.path.join(ROOT, "profiles", r, f) for r, f in
               (("r06", "bench_pmc_traffic.json"), ("r05", "bench_pmc_traffic.json"), ("r04", "bench_pmc_traffic.json"), ("r03", "bench_pmc_traffic.json"), ("r02", "bench_pmc_traffic.json"),
                ("r01", "v9_pmc_traffic.json"))]


def pmc_traffic(kernel: str):
    """HBM-side bytes per launch of ``kernel`` from the committed rocprofv3 counter passes of this
    bench command (FETCH_SIZE doubled per the gfx950 correction, plus WRITE_SIZE), or None."""
    for path in PMC_TRAFFIC:
        try:
            with open(path) as f:
                rec = json.load(f)["kernels"][kernel]
            return rec["traffic_bytes_per_launch"], os.path.relpath(path, ROOT)
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def flops_per_amp(prob) -> float:
    """Algorithmic flops per amplitude of one H application:
    diagonal 4, each drive flip 8, each pair 4 on half the rows (= 2 per amp)."""
    n_pairs = int(np.count_nonzero(np.triu(prob.pair, 1)))
    n_flips = int(np.count_nonzero(np.any(prob.flip != 0.0, axis=1)))
    return 4.0 + 8.0 * n_flips + 2.0 * n_pairs


def cpu_baseline(fraction: float, cores: int):
    """QuTiP-5 sesolve equivalent on the host cores (oracle/cpu_bench.py), run as a child process
    before this process touches the GPU (its worker pool forks a process without a GPU context)."""
    import subprocess
    if cores <= 0:  # this process's CPU share: the affinity set, capped by the box's thread budget
        cores = len(os.sched_getaffinity(0))
        for key in ("OMP_NUM_THREADS", "MAX_JOBS"):
            if os.environ.get(key, "").isdigit():
                cores = min(cores, int(os.environ[key]))
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    res = subprocess.run([sys.executable, "-m", "oracle.cpu_bench", "--fraction", str(fraction),
                          "--cores", str(cores)], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900.0)
    if res.returncode != 0:
        raise RuntimeError(f"oracle.cpu_bench failed: {res.stderr[-2000:]}")
    return json.loads(res.stdout.strip().splitlines()[-1])


WHT_PMC_N30 = next((q for q in (os.path.join(ROOT, "profiles", r, "wht_n30_pmc_traffic.json")
                                 for r in ("r06", "r05", "r04", "r01")) if os.path.exists(q)),
                   os.path.join(ROOT, "profiles", "r01", "wht_n30_pmc_traffic.json"))


def diag_energy(prob) -> float:
    """<psi0|H|psi0> = D(x0) of the basis state psi0 (include/dse.h conventions)."""
    x = prob.psi0_index
    sv = np.array([0.5 - ((x >> b) & 1) for b in range(prob.n_qubits)])
    return float(prob.shift + prob.field @ sv + np.sum(np.triu(prob.zz, 1) * np.outer(sv, sv)))


def large_register(device: int, n_sea: int = 29):
    """Config 5 on one GPU (N = n_sea + 1 = 30, center_on, 50 kHz, t_final 5e-6 s, 6 outputs): the
    Walsh-Hadamard engine's H|psi> passes against the HBM roofline.  Bytes per amplitude and H
    application are the passes' algorithmic traffic: FWD/MID/INV 64 each, FINAL 80 + acc 32 every
    third term, and the next term's A and B (32) written by the same pass (option wht_fuse, the
    default; FIRST's 48 once per interval, not counted); "traffic" is the rocprofv3 FETCH/WRITE count
    of the same passes (profiles/<round>/wht_n30_pmc_traffic.json, tools/gpu.sh traffic_large).  Kernel time per H application from HIP events
    (excludes the first call's device allocation of 5 x 16 GiB).  "check": exact invariants of the
    unitary evolution on the 2^30 state (no reference state exists at this size): ||psi(t)|| = 1 at
    every output and <H> of the final state = <psi0|H|psi0> (dse_energy, on the device)."""
    from quantumsimulations_amd import problem as pb
    from quantumsimulations_amd.engine import Engine
    from quantumsimulations_amd.sweep import sweep_point_params
    t_final, steps = 5e-6, 6
    p = sweep_point_params(n_sea, 50e3, "center_on", t_final, steps)
    prob = pb.build_problem(p)
    n = prob.n_qubits
    wl = 13
    groups = 1 + -(-(n - wl) // (wl - 2))
    bpa = 64.0 * (2 * groups - 3) + 80.0 + 32.0 / 3.0 + 32.0
    with Engine(device) as eng:
        pid = eng.add(prob)
        t0 = time.perf_counter()
        obs, st = eng.evolve(np.linspace(0.0, t_final, steps))
        wall = time.perf_counter() - t0
        energy, norm2 = eng.energy(pid)
    e0 = diag_energy(prob)
    per_term_ms = st["step_kernel_ms"] / max(st["timed_launches"], 1)
    gbs = bpa * (1 << n) / (per_term_ms * 1e-3) / 1e9
    s8d = 80.0 * (1 << n) / (per_term_ms * 1e-3) / 1e9
    fpa = flops_per_amp(prob)
    fl = fpa * (1 << n)
    # HBM-side bytes per H application: the MODE_GEN (2) launches of the five passes in the counter
    # record (template keys k_wht<13, pass, 2[, vectors]>, one launch per pass and H application);
    # a missing record or pass is an explicit error, never a silent null
    traffic, traffic_error = None, None
    try:
        with open(WHT_PMC_N30) as f:
            k = json.load(f)["kernels"]
        if n != 30:
            traffic_error = f"counter record is for N = 30, this register is N = {n}"
        else:
            # MODE_GEN launches of FWD (1), MID (2), INV (3) (k_wht or the half-LDS k_wht_h) and of
            # FINAL_NEXT (5, the fused default) or FIRST (0) + FINAL (4) in a record of the unfused passes
            per_pass = {}
            for name, rec in k.items():
                m = re.fullmatch(r"k_wht(?:_h)?<13, (\d), 2(?:, \d+)?>", name)
                if m:
                    per_pass[int(m.group(1))] = per_pass.get(int(m.group(1)), 0.0) + rec["traffic_bytes_per_launch"]
            need = (1, 2, 3, 5) if 5 in per_pass else (0, 1, 2, 3, 4)
            missing = [ps for ps in need if ps not in per_pass]
            if missing:
                traffic_error = f"passes {missing} missing from {os.path.relpath(WHT_PMC_N30, ROOT)}"
            else:
                traffic = sum(per_pass[ps] for ps in need)
    except (OSError, KeyError, ValueError) as exc:
        traffic_error = f"counter record unreadable: {exc!r}"
    check = {"max_norm_error": float(np.max(np.abs(obs[0, 6] - 1.0))),
             "energy_rel_error": abs(energy - e0) / abs(e0), "energy": energy, "energy_t0": e0,
             "final_norm2": norm2}
    check["ok"] = bool(check["max_norm_error"] < 1e-12 and check["energy_rel_error"] < 1e-11)
    return {
        "workload": f"config 5 on one GPU: N={n} center_on, 50 kHz, t_final {t_final} s, {steps} outputs",
        "engine_mode": st["mode"], "tile_bits": wl, "passes_per_h": 2 * groups - 1,
        "h_applications": st["h_applications"],
        "kernel_ms_per_h_application": per_term_ms,
        "wall_ms_per_h_application_incl_setup": wall / st["h_applications"] * 1e3,
        # SURVEY.md §8(d)'s pricing of a fused Chebyshev term (80 B/amp: the bytes a one-pass
        # streaming term would move) and the FP64 rate of the algorithmic flops: at N = 30 the
        # arithmetic intensity 1072 flop / 80 B = 13.4 is past the FP64 ridge (78.6 / 8 = 9.8), so
        # FP64 is §8(d)'s binding bound; the pass-traffic figure prices the engine's own passes
        "roofline": {"bound": "fp64", "achieved": fl / (per_term_ms * 1e-3) / 1e12, "peak": FP64_PEAK_TFLOPS,
                     "unit": "TFLOP/s", "frac": fl / (per_term_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
                     "flops_per_amp_per_h": fpa,
                     "s8d_hbm": {"achieved": s8d, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": s8d / HBM_PEAK_GBS,
                                 "bytes_per_amp_per_h": 80.0},
                     "passes_hbm": {"achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": gbs / HBM_PEAK_GBS, "bytes_per_amp_per_h": bpa},
                     "traffic": traffic, "traffic_per_amp": traffic / (1 << n) if traffic else None,
                     "traffic_source": os.path.relpath(WHT_PMC_N30, ROOT) if traffic else None,
                     **({"traffic_error": traffic_error} if traffic_error else {})},
        "check": check,
    }


def full_sweep(eng, probs, n_points: int, intervals: int, repeats: int, sync, dist=None):
    """BASELINE's "(full sweep)" figure: the reference's grid (sweep_sea_detuning.py:1223-1224:
    t_final 30 s, 20000 outputs) on the bench's own evolutions (this rank's share of the 64-point
    sweep, 3 variants per point).  Two engines, each with its stated accuracy at t = 30 s
    (tolerance_at_t_final); the quoted one is the fastest whose stated accuracy meets north_star's
    1e-8, the other is reported beside it.
      dense      the dense eigen-propagator (libdse's cost model picks it for this grid) on the
                 WHOLE sweep: one evolve of all the rank's registers over all 20000 outputs, timed
                 whole (barrier + device sync around, max over ranks) -- measured, not extrapolated;
      chebyshev  the Chebyshev kernels on the first `intervals` output intervals (`repeats` timed
                 runs, spread reported), extrapolated linearly to all 19999 (every interval has the
                 same length, so the same work; dt = 1.5 ms: alpha dt ~ 3e3..1e4 terms each)."""
    t_ref = np.linspace(0.0, 30.0, 20000)
    eng.set_option("dense", 0)
    try:
        eng.evolve(t_ref[:2])
        stats, per = [], []
        for _ in range(max(1, repeats)):
            dt = timed_steps(lambda: stats.append(eng.evolve(t_ref[:intervals + 1])[1]), 1, 0, sync, dist)
            per.append(dt / intervals)
    finally:
        eng.set_option("dense", 1)
    st = stats[-1]
    per_interval = float(np.mean(per))
    cheb_s = per_interval * (len(t_ref) - 1)
    h_per_ev = st["h_applications"] / len(probs) / intervals     # H applications per evolution
    k_ms = st["step_kernel_ms"]
    gbs = 80.0 * st["timed_amp_terms"] / (k_ms * 1e-3) / 1e9 if k_ms > 0 else None
    cheb = {
        "engine": "chebyshev",
        "intervals_timed": intervals, "repeats": len(per), "s_per_interval": per_interval,
        "s_per_interval_min": float(np.min(per)), "s_per_interval_max": float(np.max(per)),
        "spread_rel": float((np.max(per) - np.min(per)) / per_interval),
        "full_sweep_s": cheb_s, "timing": "extrapolated from the first intervals",
        "value": n_points * 3600.0 / cheb_s, "unit": "detuning-points/hour",
        "ms_per_ode_step": per_interval * 1e3 / h_per_ev,
        "h_applications_per_evolution_per_interval": h_per_ev,
        "max_degree": st["max_degree"], "outputs_per_launch": st["outputs_per_launch"],
        "engine_mode": {1: "persistent", 2: "walsh-hadamard"}.get(st["mode"], "streaming"),
        "kernel_gbs_80B_per_amp_term": gbs,
        "kernel_frac_hbm": gbs / HBM_PEAK_GBS if gbs else None,
        "tolerance_at_t_final": tolerance_at_t_final(probs, False, t_ref[-1], len(t_ref) - 1),
    }
    dense = {"engine": "dense eigen-propagator"}
    try:
        dstats = []
        dt = timed_steps(lambda: dstats.append(eng.evolve(t_ref)[1]), 1, 0, sync, dist)
        dst = dstats[-1]
        dense.update({
            "full_sweep_s": dt, "timing": "the whole sweep timed (one evolve of every register over all 20000 outputs)",
            "value": n_points * 3600.0 / dt, "unit": "detuning-points/hour",
            "s_per_point": dt / (len(probs) / 3), "dense_problems": dst["dense_problems"],
            "eig_fallbacks": dst.get("eig_fallbacks"),
            "dense_ms": dst["dense_ms"], "eig_ms": dst["dense_eig_ms"],
            "output_ms": dst.get("dense_output_ms"), "nufft_problems": dst.get("dense_nufft_problems"),
            "tolerance_at_t_final": tolerance_at_t_final(probs, True, t_ref[-1], len(t_ref) - 1),
        })
        if dst["dense_problems"] != len(probs):
            dense["error"] = f"{dst['dense_problems']} of {len(probs)} registers on the dense engine"
    except Exception as exc:  # report, never hide
        dense["error"] = repr(exc)
    ok = [e for e in (dense, cheb) if "error" not in e and e.get("full_sweep_s")
          and e["tolerance_at_t_final"]["value"] <= NORTH_STAR_TOL]
    best = min(ok, key=lambda e: e["full_sweep_s"]) if ok else None
    out = {"grid": "t_final 30 s, 20000 outputs (sweep_sea_detuning.py:1223-1224)", "north_star_tol": NORTH_STAR_TOL}
    if best is None:
        out["error"] = "no engine meets north_star's 1e-8 at t = 30 s"
    else:
        out.update({"engine": best["engine"], "full_sweep_s": best["full_sweep_s"], "timing": best["timing"],
                    "value": best["value"], "unit": "detuning-points/hour",
                    "tolerance_at_t_final": best["tolerance_at_t_final"]})
    out["dense"], out["chebyshev"] = dense, cheb
    out["note"] = ("BASELINE's '(full sweep)' figure: the reference grid on the bench's 64 x 3 evolutions by "
                   "the fastest engine whose stated accuracy at t = 30 s meets north_star's 1e-8; headline "
                   "`value` is the 1 ms head-to-head grid; the reference's own ZVODE trace of this grid "
                   "takes ~430-1530 h per N=14 evolution on one core (SURVEY.md §6)")
    return out


NORTH_STAR_TOL = 1e-8
# -m gpu records of the accuracy on the 30 s grid (tools/gpu.sh tests with DSE_TEST_RECORD), newest first
def _newest(name):
    for r in ("r06", "r05"):
        q = os.path.join(ROOT, "profiles", r, name)
        if os.path.exists(q):
            return q
    return os.path.join(ROOT, "profiles", "r06", name)


ORACLE_N14_DENSE = _newest("grid30_n14_oracle_dense.json")     # tests/test_gpu_grid30_n14.py
ORACLE_N14_CHEB = _newest("grid30_n14_oracle_chebyshev.json")
DENSE_SOLVERS_N14 = _newest("dense_solvers_n14_30s.json")
GRID30_N7 = _newest("grid30_n7_errors.json")
CHEB_DRIFT_N14 = _newest("dense_growth_n14.json")
DENSE_TOL_ASSERTED = 1e-8   # tests/test_gpu_grid30_n14.py: every pinned output to 30 s vs the N = 14 oracle


def _record(path):
    try:
        with open(path) as f:
            return json.load(f), os.path.relpath(path, ROOT)
    except (OSError, ValueError):
        return None, None


def tolerance_at_t_final(probs, dense: bool, t_final: float, intervals: int) -> dict:
    """The stated accuracy of <O>(t_final) on the reference grid, from the -m gpu records against
    the N = 14 oracle of this grid (tests/golden/grid30_n14.npz: LAPACK eigenvectors of the
    reference-built H, double-double Rayleigh-quotient eigenvalues, 40-digit phases; 3 variants at
    150 kHz, the sweep's stiffest point; tests/test_gpu_grid30_n14.py).
    Dense engine: the measured maximum distance over the pinned outputs (t = 1.5 ms ... 30 s) of the
    bench's own registers from the reference-H fixture, and of the unreduced registers from the
    tables-H fixture (asserted <= 1e-8 in -m gpu); without the record, the asserted 1e-8.
    Chebyshev: 1e-14 truncation per interval, summed, plus its fp64 drift (~1e4 fp64 H applications
    per interval are the exact evolution of an H perturbed by ~eps ||H||): the envelope rate of its
    distance from the oracle over the grid's first 0.15 s, extrapolated to t_final."""
    from quantumsimulations_amd import problem as pb
    eps = float(np.finfo(float).eps)
    hnorm = max(max(abs(a) for a in pb.spectral_bounds(p)) for p in probs)
    out = {"engine": "dense" if dense else "chebyshev", "t_final_s": float(t_final), "hnorm_bound": hnorm,
           "north_star": NORTH_STAR_TOL}
    if dense:
        rec, src = _record(ORACLE_N14_DENSE)
        if rec:
            meas = max(rec["max_bench_registers_vs_ref"], rec["max_unreduced_vs_tables"])
            out.update({"value": meas, "basis": "measured vs the N=14 30 s oracle (grid30_n14.npz), max over "
                                               "t = 1.5 ms ... 30 s; asserted <= 1e-8 in -m gpu",
                        "at_30s": rec["at_30s_unreduced_vs_tables"],
                        "fixtures_ref_vs_tables": rec["fixtures_ref_vs_tables"], "source": src})
        else:
            out.update({"value": DENSE_TOL_ASSERTED, "basis": "asserted in -m gpu (no measured record found)"})
        rec, src = _record(DENSE_SOLVERS_N14)
        if rec:
            out["two_solvers_n14"] = {"max": rec["max"], "source": src}
        rec, src = _record(GRID30_N7)
        if rec:
            out["n7_vs_40_digits"] = {"max": rec["max_vs_tables"], "source": src}
    else:
        drift, basis = None, None
        rec, src = _record(ORACLE_N14_CHEB)
        if rec:
            drift, basis = rec["rate_envelope_per_s"] * t_final, "oracle"
        else:
            rec, src = _record(CHEB_DRIFT_N14)
            if rec:
                drift, basis = rec["rate_envelope_per_s"] * t_final, "vs the dense engine"
        if rec:
            out["measured_drift_n14"] = {"rate_per_s": rec["rate_envelope_per_s"], "against": basis, "source": src}
        out.update({"value": 1e-14 * intervals + (drift if drift is not None else 1.5 * eps * hnorm * t_final),
                    "formula": "1e-14 per interval x intervals + fp64 drift rate x t_final"})
    return out


LDS_PEAK_TBS = 256 * 2.4e9 * 256 / 1e12   # 256 B/clk/CU for ds_read_b128 (MI355X_MICROARCH.md §LDS) x 2.4 GHz x 256 CUs
# ds_read_b128 / ds_write_b128 per thread and Chebyshev term of k_interval<13> (16 amplitudes per
# thread): 9 fused iterations x (16 sweep rows + 4 thread pairs x 16 rows + 8 table granules),
# phase 1's own rows + diagonal constants (19), phase 5's own rows (16), w_k -> LDS (16 writes);
# the shell registers' u pre-pass adds 16 + 6 x 16 + 3 x 16 / 2 = 136
LDS_B_PER_AMP_TERM = 16.0 * (9 * (16 + 64 + 8) + 19 + 16 + 16) / 16.0


CLOCK_UNDER_LOAD = _newest("clock_under_load.json")  # tools/clock_probe.sh (GRBM_GUI_ACTIVE passes)


def clock_under_load():
    """The GPU clock measured under the bench's full sweep and under one GPU's 2-GPU share (committed
    counter record; None without one)."""
    try:
        c = json.load(open(CLOCK_UNDER_LOAD))["cases"]
        return {"full_sweep_ghz": c["full"]["clock_ghz_median"], "share2_ghz": c["share2"]["clock_ghz_median"],
                "nominal_ghz": 2.4, "source": os.path.relpath(CLOCK_UNDER_LOAD, ROOT)}
    except (OSError, KeyError, ValueError):
        return None


def on_chip_roofline(amp_terms, k_ms, fp64_tflops) -> dict:
    """The resources that bind the persistent kernel (the terms stay on chip, so HBM does not): the
    LDS array (the kernel's own ds_read/ds_write bytes per amplitude-term against 256 B/clk/CU) and
    FP64 issue (algorithmic flops against the FP64 peak), both priced at the nominal 2.4 GHz; and the
    clock the chip actually runs this kernel at (power-capped below 2.4 GHz with every CU busy)."""
    if not k_ms:
        return {}
    lds = LDS_B_PER_AMP_TERM * amp_terms / (k_ms * 1e-3) / 1e12
    out = {"lds": {"achieved": lds, "peak": LDS_PEAK_TBS, "unit": "TB/s", "frac": lds / LDS_PEAK_TBS,
                   "bytes_per_amp_term": LDS_B_PER_AMP_TERM},
           "fp64": {"achieved": fp64_tflops, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": fp64_tflops / FP64_PEAK_TFLOPS if fp64_tflops else None},
           "note": "neither pipe saturated at the nominal clock: the chip runs the full sweep at ~2.0 GHz "
                   "(power cap; one GPU's 2-GPU share at 2.28), and the fused loop's LDS reads and FP64 "
                   "FMAs serialise at two waves per SIMD (DESIGN.md §4.1, §9)"}
    clk = clock_under_load()
    if clk:
        out["clock"] = clk
    return out


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def _round(x, sig=5):
    """floats to `sig` significant digits (the compact line), recursively"""
    if isinstance(x, float):
        return float(f"{x:.{sig}g}")
    if isinstance(x, dict):
        return {k: _round(v, sig) for k, v in x.items()}
    if isinstance(x, list):
        return [_round(v, sig) for v in x]
    return x


def compact_line(line: dict, detail_path) -> dict:
    """The stdout line: the contract's fields, the headline roofline and CPU baseline, and one
    summary per leg (the driver keeps only the tail of stdout); the full record goes to detail_path."""
    c = _pick(line, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                     "scaling", "vs_baseline", "dtype", "data"))
    c["config"] = _pick(line["config"], ("workload", "global_points_per_step", "evolutions_per_step_per_gpu",
                                         "propagator", "engine_mode", "outputs_per_launch", "ms_per_ode_step",
                                         "h_applications_per_step", "parallelism", "span_problems"))
    r = line.get("roofline", {})
    c["roofline"] = _pick(r, ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source",
                              "avg_launch_us", "algorithmic_bytes_per_launch", "bytes_per_amp_term"))
    c["roofline"]["kernel"] = r.get("kernel", "").split(" (")[0]
    if "fp64" in r:
        c["roofline"]["fp64_frac"] = r["fp64"].get("frac")
    if "chip_level" in r:
        c["roofline"]["chip_level_frac"] = r["chip_level"].get("frac")
    if r.get("on_chip"):
        c["roofline"]["on_chip"] = {"lds_frac": r["on_chip"]["lds"]["frac"], "fp64_frac": r["on_chip"]["fp64"]["frac"],
                                    "lds_bytes_per_amp_term": r["on_chip"]["lds"]["bytes_per_amp_term"]}
        if r["on_chip"].get("clock"):
            c["roofline"]["on_chip"]["clock_ghz_under_load"] = r["on_chip"]["clock"]["full_sweep_ghz"]
    if "cpu_baseline" in line:
        c["cpu_baseline"] = _pick(line["cpu_baseline"], ("value", "unit", "cores", "kind", "sample", "value_all_cores",
                                                         "cores_all", "value_full_node_estimate", "error"))
    fs = line.get("full_sweep")
    if fs:
        c["full_sweep"] = _pick(fs, ("engine", "value", "unit", "full_sweep_s", "timing", "error"))
        c["full_sweep"]["grid"] = "30 s / 20000 outputs (sweep_sea_detuning.py:1223-1224)"
        tol = fs.get("tolerance_at_t_final", {})
        c["full_sweep"]["tolerance_at_t_final"] = _pick(tol, ("value", "basis", "at_30s"))
        d = fs.get("dense", {})
        c["full_sweep"]["dense"] = _pick(d, ("s_per_point", "eig_ms", "dense_ms", "output_ms", "nufft_problems",
                                             "eig_fallbacks", "error"))
        ch = fs.get("chebyshev", {})
        c["full_sweep"]["chebyshev"] = {**_pick(ch, ("value", "full_sweep_s", "timing")),
                                        "tolerance_at_t_final": ch.get("tolerance_at_t_final", {}).get("value")}
    ss = line.get("strong_split")
    if ss:
        c["strong_split"] = {"note": "each rank's shard of the one 64-point sweep timed alone on this GPU; "
                                     "heaviest shard = predicted step"} if "error" not in ss else ss
        for w, leg in ss.items():
            if isinstance(leg, dict):
                c["strong_split"][w] = _pick(leg, ("step_ms", "value", "ms_per_ode_step", "span_problems", "error"))
    if "config2" in line:
        c2 = line["config2"]
        c["config2"] = _pick(c2, ("wall_ms", "max_abs_err_vs_exact", "tolerance", "error"))
        if isinstance(c2.get("matrix_mode"), dict) and c2["matrix_mode"].get("roofline"):
            c["config2"]["matrix_product_frac"] = c2["matrix_mode"]["roofline"]["frac"]
        if "unmodified_caller_n14" in c2:
            c["config2"]["n14_ms_per_call"] = c2["unmodified_caller_n14"]["ms_per_call"]
    if "reference_default" in line:
        c["reference_default"] = _pick(line["reference_default"], ("wall_s", "value", "max_norm_error", "error"))
    if "large_register" in line:
        lr = line["large_register"]
        c["large_register"] = _pick(lr, ("kernel_ms_per_h_application", "error"))
        if "roofline" in lr:
            rr = lr["roofline"]
            c["large_register"].update({"fp64_frac": rr.get("frac"), "passes_hbm_frac": rr["passes_hbm"]["frac"],
                                        "traffic_per_amp": rr.get("traffic_per_amp")})
        if "check" in lr:
            c["large_register"]["check_ok"] = lr["check"]["ok"]
    if "partitioned" in line:
        c["partitioned"] = _pick(line["partitioned"], ("ms_per_h_application", "xgmi_gbs_per_link", "exchange_ms", "norm_error",
                                                      "error", "child_wall_s"))
    if detail_path:
        c["detail"] = detail_path
    if isinstance(c.get("cpu_baseline", {}).get("sample"), str) and len(c["cpu_baseline"]["sample"]) > 320:
        c["cpu_baseline"]["sample"] = c["cpu_baseline"]["sample"][:317] + "..."
    head = {k: c[k] for k in ("value", "ms_per_step")}   # the headline at full precision
    c = _round(c)
    c.update(head)
    return c


def matrix_kernels(st) -> dict:
    """Propagator-matrix mode's device time (HIP events in libdse): the column build of U (k_ucols)
    and the n_t - 2 products psi_{j+1} = U psi_j (k_symv + k_symv_reduce).  A product reads U's
    stored 64 x 64 tiles on and above the diagonal once (complex symmetric U: 130 MiB at N = 12, held
    in the 256 MiB Infinity Cache between products) plus x; priced against the HBM peak, which the
    MALL-resident stream may exceed."""
    if st.get("mode") != 5 or not st.get("matrix_products"):
        return {"used": False}
    per = st["matrix_products_ms"] / st["matrix_products"]
    gbs = st["matrix_bytes_per_product"] / (per * 1e-3) / 1e9
    return {"used": True, "build_ms": st["matrix_build_ms"], "products": st["matrix_products"],
            "products_ms": st["matrix_products_ms"], "us_per_product": per * 1e3,
            "roofline": {"kernel": "k_symv + k_symv_reduce (half-matrix symmetric product)", "bound": "hbm",
                         "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                         "bytes_per_product": st["matrix_bytes_per_product"],
                         "note": "U's stored tiles are Infinity-Cache resident across the products"}}


def config2_leg(device: int):
    """BASELINE config 2 through the drop-in surface: one N = 12 center_on evolution (n_sea = 11,
    50 kHz, 2 ms / 201 outputs) by simulate_rare (dipolar_ensemble_with_rare.py:611 replaced), wall
    time per call after a warm-up call, and its distance to the exact-eigh fixture of the
    reference-built H (tests/golden/traces_n12.npz, data only).  Then the unmodified caller's
    pattern at N = 14 (sweep_sea_detuning.py:671-702: three serial simulate_rare calls per point,
    1 ms / 101 outputs, 75 kHz)."""
    os.environ.setdefault("DSE_DEVICE", str(device))
    from quantumsimulations_amd import dipolar_ensemble_with_rare as dse
    from quantumsimulations_amd import problem as pb
    from quantumsimulations_amd.engine import Engine
    from quantumsimulations_amd.sweep import VARIANTS, sweep_point_params
    p = sweep_point_params(11, 50e3, "center_on", 2e-3, 201)
    dse.simulate_rare(p)
    walls, res = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        res = dse.simulate_rare(p)
        walls.append((time.perf_counter() - t0) * 1e3)
    err = None
    try:
        tr = np.load(os.path.join(ROOT, "tests", "golden", "traces_n12.npz"), allow_pickle=False)
        err = max(float(np.max(np.abs(res[1][k] - tr[f"exact_{k}"]))) for k in res[1])
    except (OSError, KeyError):
        pass
    with Engine(device) as eng:   # the engine's own counters for the same evolution
        eng.add(pb.build_problem(p))
        eng.evolve(pb.time_grid(p))
        _, st = eng.evolve(pb.time_grid(p))
    ps = [sweep_point_params(13, 75e3, v, 1e-3, 101) for v in VARIANTS]
    for q in ps:
        dse.simulate_rare(q)
    t0 = time.perf_counter()
    for q in ps:
        dse.simulate_rare(q)
    serial14 = (time.perf_counter() - t0) * 1e3
    return {
        "workload": "config 2: N=12 (n_sea=11) center_on, 50 kHz, t_final 2 ms, 201 outputs, one "
                    "simulate_rare call",
        "wall_ms": float(np.median(walls)), "wall_ms_runs": walls,
        "max_abs_err_vs_exact": err, "tolerance": 1e-8,
        "engine": {"mode": st["mode"], "max_degree": st["max_degree"],
                   "h_applications": st["h_applications"], "launches": st["step_launches"],
                   "kernel_ms": st["step_kernel_ms"], "dense_problems": st["dense_problems"],
                   "span_problems": st["span_problems"]},
        "matrix_mode": matrix_kernels(st),
        "ms_per_h_application": float(np.median(walls)) / max(st["h_applications"], 1),
        "unmodified_caller_n14": {"calls": 3, "grid": "1 ms / 101 outputs, 75 kHz",
                                  "wall_ms": serial14, "ms_per_call": serial14 / 3},
    }


def reference_default_leg(device: int, k_cheb: int = 20):
    """The reference's own default run (sweep_sea_detuning.py:1223-1240: n_sea = 6 -> N = 7, 13
    detunings in [0, 150 kHz] x 3 variants, t_final 30 s, 20 000 outputs), all 39 evolutions in one
    evolve: the engine's cost model takes the dense eigen-propagator (every output exact at any
    time).  Timed whole (after one untimed call), no extrapolation.  Beside it, the Chebyshev
    small-register engine (option dense = 0) on the first `k_cheb` intervals, extrapolated."""
    from quantumsimulations_amd import problem as pb
    from quantumsimulations_amd.engine import Engine
    from quantumsimulations_amd.sweep import VARIANTS, sweep_point_params
    t_ref = np.linspace(0.0, 30.0, 20000)
    dets = np.linspace(0.0, 150e3, 13)
    probs = [pb.build_problem(sweep_point_params(6, float(d), v, 30.0, 20000)) for d in dets for v in VARIANTS]
    with Engine(device) as eng:
        for q in probs:
            eng.add(q)
        eng.evolve(t_ref)
        t0 = time.perf_counter()
        obs, st = eng.evolve(t_ref)
        wall = time.perf_counter() - t0
        eng.set_option("dense", 0)
        eng.evolve(t_ref[:2])
        t1 = time.perf_counter()
        _, st2 = eng.evolve(t_ref[:k_cheb + 1])
        wall2 = time.perf_counter() - t1
    cheb_full = wall2 / k_cheb * (len(t_ref) - 1)
    return {
        "workload": "reference default: n_sea=6 (N=7), 13 detunings x 3 variants, t_final 30 s, "
                    "20000 outputs (sweep_sea_detuning.py:1223-1240)",
        "engine_mode": st["mode"], "dense_problems": st["dense_problems"],
        "wall_s": wall, "eig_ms": st["dense_eig_ms"], "dense_ms": st["dense_ms"],
        "value": len(dets) * 3600.0 / wall, "unit": "detuning-points/hour (measured, whole grid)",
        "max_norm_error": float(np.max(np.abs(obs[:, 6] - 1.0))),
        "chebyshev_small_engine": {
            "intervals_timed": k_cheb, "s_per_interval": wall2 / k_cheb,
            "full_s_extrapolated": cheb_full, "value": len(dets) * 3600.0 / cheb_full,
            "max_degree": st2["max_degree"], "launches": st2["step_launches"]},
        "cpu_reference_note": "ZVODE at the reference tolerances: ~3-16 h per N=7 evolution on one "
                              "core for this grid (SURVEY.md §6, P2/P5, extrapolated)",
    }


def shard_detunings(n_det: int, rank: int, world: int, scaling: str = "strong") -> np.ndarray:
    """strong: rank r takes detunings j = r (mod world) of linspace(0, 150 kHz, n_det) (one sweep
    split over the ranks); weak: j = r (mod world) of linspace(0, 150 kHz, n_det * world)."""
    total = n_det if scaling == "strong" else n_det * world
    return np.linspace(0.0, DELTA_MAX, total)[rank::world]


def strong_shard_leg(eng, n_sea: int, n_det: int, world_pred: int = 8, reps: int = 3) -> dict:
    """The world_pred-GPU strong split of the n_det-point sweep, predicted on this GPU: every rank's
    shard (n_det / world_pred points x 3 variants) evolved alone in this context, reps times
    (minimum kept); the step time of the split is the heaviest shard's.  One GPU per shard, no
    collective: the prediction omits only the ranks' barrier."""
    import torch

    from quantumsimulations_amd import problem as pb
    from quantumsimulations_amd.sweep import sweep_params
    t = np.linspace(0.0, T_FINAL, STEPS_T)
    shards = []
    for r in range(world_pred):
        dets = shard_detunings(n_det, r, world_pred, "strong")
        eng.clear()
        for p in sweep_params(n_sea, dets, T_FINAL, STEPS_T):
            eng.add(pb.build_problem(p))
        eng.evolve(t)  # warm-up
        walls = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, st = eng.evolve(t)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        ode = st["h_applications"] / (3 * len(dets))
        shards.append({"rank": r, "points": len(dets), "wall_ms": min(walls), "kernel_ms": st["step_kernel_ms"],
                       "span_problems": st["span_problems"], "max_degree": st["max_degree"],
                       "ms_per_ode_step": min(walls) / ode})
    eng.clear()
    worst = max(shards, key=lambda x: x["wall_ms"])
    return {"gpus": world_pred, "points": n_det, "step_ms": worst["wall_ms"],
            "value": n_det / (worst["wall_ms"] * 1e-3) * 3600.0, "unit": "detuning-points/hour",
            "ms_per_ode_step": worst["ms_per_ode_step"], "heaviest_rank": worst["rank"],
            "span_problems": worst["span_problems"], "shards": shards,
            "note": (f"each of the {world_pred} ranks' shards of the {n_det}-point sweep timed alone on this GPU "
                     "(min of reps); the split's step time is the heaviest shard's")}


def strong_split_legs(eng, n_sea: int, n_det: int, worlds=(2, 4, 8)) -> dict:
    """BASELINE's "1/2/4/8 GPUs": the strong split of the one 64-point sweep predicted on this GPU
    for every world size (N = 1 is the timed headline itself)."""
    return {str(w): strong_shard_leg(eng, n_sea, n_det, w) for w in worlds}


def timed_steps(step, steps: int, warmup: int, sync, dist=None) -> float:
    """W untimed steps, then K steps bracketed by barrier + device sync on both sides; returns
    the maximum over ranks of the timed wall time."""
    import torch

    def barrier():
        sync()
        if dist is not None:
            dist.barrier()
    for _ in range(warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    barrier()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64)
        if dist.get_backend() == "nccl":
            tt = tt.cuda()
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    return dt


class Heartbeat:
    """A progress line on stderr every `every` seconds while the bench runs (a long leg -- the whole
    30 s-grid sweep on the dense engine is minutes of device work in one call -- is not a hang)."""

    def __init__(self, every: float = 45.0):
        import threading
        self.phase, self.t0 = "start", time.time()
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, args=(every,), daemon=True)
        self._th.start()

    def _run(self, every):
        while not self._stop.wait(every):
            print(f"[bench] {self.phase}: {time.time() - self.t0:.0f} s", file=sys.stderr, flush=True)

    def stop(self):
        self._stop.set()


HEARTBEAT = None


def phase(name: str) -> None:
    if HEARTBEAT is not None:
        HEARTBEAT.phase = name
    print(f"[bench] {name}", file=sys.stderr, flush=True)


def note(msg: str) -> None:
    """Progress on stderr (the JSON line is the only stdout)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(path: str, obs: np.ndarray, rank: int = 0, world: int = 1) -> str:
    """--dump-outputs: the observables of the last timed step as float64 [evolution, 7, n_t] in
    path/observables.npy (observables_rank<r>.npy with several ranks).  Above DUMP_MAX_BYTES (per
    rank: its share of them) a fixed, seeded sample of the evolutions, in their order, is kept."""
    os.makedirs(path, exist_ok=True)
    a = np.ascontiguousarray(obs, dtype=np.float64)
    keep = max(1, (DUMP_MAX_BYTES // world) // max(a[0].nbytes, 1)) if len(a) else 0
    if len(a) > keep:
        a = a[np.sort(np.random.default_rng(0).choice(len(a), keep, replace=False))]
    name = os.path.join(path, "observables.npy" if world == 1 else f"observables_rank{rank}.npy")
    np.save(name, a)
    return name


def partitioned_leg(rank: int, world: int, local: int, dist, timeout: float, cmd=None) -> dict:
    """Config 5 across the job's ranks: every rank starts tools/bench_partitioned.py as a child
    process (its own gloo bootstrap on a fresh port, libdse's RCCL communicator for the data path)
    and waits for it with a timeout; rank 0's child prints the JSON line.  A failure or a hang
    ends in a report, never in an exception or a hung bench."""
    box = [None]
    if rank == 0:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        box[0] = s.getsockname()[1]
        s.close()
    dist.broadcast_object_list(box, src=0)
    # torchrun's elastic variables (TORCHELASTIC_USE_AGENT_STORE, ...) would make the child's
    # init_process_group a client of the agent's store instead of starting its own on the new port
    env = {k: v for k, v in os.environ.items() if not k.startswith(("TORCHELASTIC_", "TORCH_ELASTIC_"))}
    env.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(local), MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(box[0]))
    transport = os.environ.get("DSE_PARTITIONED_TRANSPORT", "rccl")
    if cmd is None:
        n_sea = os.environ.get("DSE_PARTITIONED_NSEA", "29")  # smaller registers only in a rehearsal
        cmd = [sys.executable, "-u", os.path.join(ROOT, "tools", "bench_partitioned.py"), "--n-sea", n_sea,
               "--t-final", "5e-6", "--steps", "6", "--transport", transport]
    dist.barrier()
    note(f"rank {rank}: partitioned leg child started ({' '.join(cmd[2:])})")
    t0 = time.perf_counter()
    try:
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
        rc, out, err = res.returncode, res.stdout, res.stderr
    except subprocess.TimeoutExpired as exc:
        rc, out, err = "timeout", exc.stdout or "", exc.stderr or ""
        out = out.decode() if isinstance(out, bytes) else out
        err = err.decode() if isinstance(err, bytes) else err
    wall = time.perf_counter() - t0
    note(f"rank {rank}: partitioned leg child ended rc={rc} after {wall:.1f} s")
    if rank != 0:
        return {}
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    if rc == 0 and lines:
        rep = json.loads(lines[-1])
        rep["child_wall_s"] = wall
        return rep
    return {"error": f"child rc={rc}", "child_wall_s": wall, "stderr_tail": err[-1500:]}


def main(argv=None):
    global HEARTBEAT
    args = parse(argv)
    HEARTBEAT = Heartbeat()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:  # before any GPU work: the CPU leg forks worker processes
            phase("cpu_baseline")
            cpu = cpu_baseline(args.cpu_fraction, args.cpu_cores)
        except Exception as exc:  # report, never hide
            cpu = {"value": None, "error": repr(exc)}
    import torch
    local = local % max(torch.cuda.device_count(), 1)  # several ranks per GPU only in a rehearsal
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        # RCCL carries only the barrier and the max-time reduction: the evolutions are independent
        backend = os.environ.get("DSE_BENCH_BACKEND", "nccl")  # gloo: a rehearsal on one GPU
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)

    from quantumsimulations_amd import problem as pb
    from quantumsimulations_amd.engine import Engine
    from quantumsimulations_amd.sweep import sweep_params

    my_det = shard_detunings(args.n_det, rank, world, args.scaling)
    params = sweep_params(args.n_sea, my_det, T_FINAL, STEPS_T)
    probs = [pb.build_problem(p) for p in params]
    t = np.linspace(0.0, T_FINAL, STEPS_T)

    if world > 1:
        note(f"rank {rank}/{world}: device {local}, {len(probs)} evolutions")
    eng = Engine(local, tile_bits=args.tile_bits)
    eng.set_option("streams", args.streams)
    eng.set_option("persistent", 0 if args.streaming else 1)
    eng.set_option("outputs_per_launch", args.outputs_per_launch)
    eng.set_option("mixed_launch", args.mixed_launch)
    eng.set_option("obs_overlap", args.obs_overlap)
    eng.set_option("real", args.real)
    eng.set_option("span_tile", args.span_tile)
    if os.environ.get("DSE_CORESIDENT"):  # diagnostics: workgroups per 2-tile interval launch chunk
        eng.set_option("coresident", float(os.environ["DSE_CORESIDENT"]))
    for kv in filter(None, os.environ.get("DSE_BENCH_SET", "").split(",")):  # A/Bs: key=value,...
        key, val = kv.split("=")
        eng.set_option(key, float(val))
    for p in probs:
        eng.add(p)

    stats = []
    warm = [args.warmup]
    last_obs = [None]

    def step():
        last_obs[0], st = eng.evolve(t)
        if warm[0] > 0:
            warm[0] -= 1
        else:
            stats.append(st)
    phase("sweep (timed steps)")
    dt = timed_steps(step, args.steps, args.warmup, torch.cuda.synchronize, dist)
    if args.dump_outputs:
        note(f"rank {rank}: outputs of the last timed step -> "
             f"{dump_outputs(args.dump_outputs, last_obs[0], rank, world)}")

    if world > 1:
        note(f"rank {rank}: timed steps done ({dt:.3f} s)")
    points = (args.n_det if args.scaling == "strong" else len(my_det) * world) * args.steps
    value = points / dt * 3600.0
    h_apps = sum(s["h_applications"] for s in stats)
    mode = stats[-1]["mode"]
    k_ms = sum(s["step_kernel_ms"] for s in stats)            # HIP-event time of timed launches
    k_launches = sum(s["timed_launches"] for s in stats)
    k_flops = sum(s["timed_flops"] for s in stats)             # their algorithmic flops
    k_bytes = sum(s["timed_bytes"] for s in stats)             # their algorithmic HBM bytes (streaming)
    all_flops = sum(s["h_flops"] for s in stats)
    all_bytes = sum(s["step_bytes"] for s in stats)
    fpa = sum(flops_per_amp(p) * (1 << p.n_qubits) for p in probs) / sum(1 << p.n_qubits for p in probs)
    amp_terms = sum(s["timed_amp_terms"] for s in stats)       # their amplitudes x terms
    all_amp_terms = sum(s["amplitude_updates"] for s in stats)
    def by_stream(stats):
        # the same launches split by stream: lane 0 holds the 2-tile registers (the stream whose
        # launches set the step time) and, with mixed_launch (default), the 1-tile ones in the same
        # launches; without it the other lane holds the 1-tile ones, whose launch durations include
        # the time their workgroups wait for CUs held by lane 0's launch
        l0_ms = sum(s_["lane0_kernel_ms"] for s_ in stats)
        l0_n = sum(s_["lane0_launches"] for s_ in stats)
        l0_amps = sum(s_["lane0_amp_terms"] for s_ in stats)
        out = []
        for name, ms, n, amps in (("lane 0 (2-tile registers; mixed launches: all)", l0_ms, l0_n, l0_amps),
                                  ("other lanes (1-tile registers)", k_ms - l0_ms, k_launches - l0_n,
                                   amp_terms - l0_amps)):
            if n <= 0 or ms <= 0:
                continue
            gbs = 80.0 * amps / (ms * 1e-3) / 1e9
            out.append({"stream": name, "launches": n, "avg_launch_us": ms / n * 1e3,
                        "achieved": gbs, "frac": gbs / HBM_PEAK_GBS})
        return out

    if mode == 1:
        # persistent interval kernel, priced as SURVEY.md §8(d) prices a fused Chebyshev term:
        # 80 B per amplitude (read w_{k-1}, w_{k-2}, acc; write w_k, acc) against the HBM peak
        achieved = 80.0 * amp_terms / (k_ms * 1e-3) / 1e9 if k_ms > 0 else None
        real = stats[-1].get("real_problems", 0) > 0
        name = "k_real" if real else f"k_interval<{args.tile_bits}, true>"
        traffic, traffic_src = pmc_traffic(name) if (real or args.tile_bits == 13) else (None, None)
        fp64 = k_flops / (k_ms * 1e-3) / 1e12 if k_ms > 0 else None
        roof = {
            "kernel": (f"{name} (real-component Chebyshev interval in the rotated frame: one workgroup per "
                       "real component of a whole register, all K terms of M outputs on chip)" if real else
                       f"{name} (persistent Chebyshev interval: all K terms of M outputs on chip)"),
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic,
            "traffic_source": traffic_src,
            "bytes_per_amp_term": 80.0,
            "avg_launch_us": k_ms / k_launches * 1e3 if k_launches else None,
            "algorithmic_bytes_per_launch": 80.0 * amp_terms / k_launches if k_launches else None,
            "amp_terms_per_launch": amp_terms / k_launches if k_launches else None,
            "chip_level": {"achieved": 80.0 * all_amp_terms / dt / 1e9,
                           "frac": 80.0 * all_amp_terms / dt / 1e9 / HBM_PEAK_GBS,
                           "note": "all launches of the step (all streams) / step wall time"},
            "by_stream": by_stream(stats),
            "fp64": {"achieved_tflops": fp64, "peak_tflops": FP64_PEAK_TFLOPS,
                     "frac": fp64 / FP64_PEAK_TFLOPS if fp64 else None,
                     "algorithmic_flops_per_amp": fpa,
                     "chip_level_tflops": all_flops / dt / 1e12},
            "on_chip": on_chip_roofline(amp_terms, k_ms, fp64),
            "note": ("achieved = 80 B x (amplitudes x Chebyshev terms) of the HIP-event-timed launches / "
                     "their summed durations (SURVEY.md §8(d)); the terms stay on chip (LDS + "
                     "registers), so the kernel is bounded by LDS and FP64 issue, not HBM; traffic = "
                     "L2<->fabric bytes per launch from rocprofv3 FETCH_SIZE/WRITE_SIZE passes "
                     "(mostly the 2-tile problems' per-term hand-off)"),
        }
    else:
        achieved = k_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else None
        roof = {
            "kernel": ("k_wht passes (Walsh-Hadamard engine: one Chebyshev term = FIRST, MID, FINAL)"
                       if mode == 2 else
                       "k_step_rb<13,MODE_GEN> (Chebyshev step: H|w>, recurrence, accumulation)"),
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": None,
            "algorithmic_bytes_per_amp": 58.7,
            "avg_launch_us": k_ms / k_launches * 1e3 if k_launches else None,
            "bytes_per_launch": k_bytes / k_launches if k_launches else None,
            "achieved_fp64_tflops": k_flops / (k_ms * 1e-3) / 1e12 if k_ms > 0 else None,
            "aggregate_step_gbs": all_bytes / dt / 1e9,
            "note": ("per-launch HIP-event durations; launches of different streams overlap, so "
                     "per-launch GB/s understates the aggregate (aggregate_step_gbs)"),
        }
    line = {
        "metric": "detuning-points/hour (N=14 sea-detuning sweep, 3 variants per point)",
        "value": value,
        "unit": "detuning-points/hour",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "f64 (complex128 state)",
        "data": "synthetic (reference physical constants, deterministic; no external data)",
        "config": {
            "workload": (f"config 3: n_sea={args.n_sea}+1 rare (N=14 qubits), "
                         + (f"one {args.n_det}-point sweep split over {world} GPU(s)" if args.scaling == "strong"
                            else f"{args.n_det} points per GPU") +
                         f" ({len(my_det)} detunings in [0,150 kHz] x 3 variants = {3 * len(my_det)} evolutions"
                         f" on rank 0), t_final={T_FINAL}s, {STEPS_T} outputs, 7 observables"),
            "global_points_per_step": args.n_det if args.scaling == "strong" else len(my_det) * world,
            "evolutions_per_step_per_gpu": len(probs),
            "propagator": "exact Chebyshev (tol 1e-14)",
            "engine_mode": ({1: "persistent", 2: "walsh-hadamard"}.get(mode, "streaming")
                            + (" real-component (k_real)" if stats[-1].get("real_problems", 0) else "")),
            "real_problems": stats[-1].get("real_problems"),
            "tile_bits": args.tile_bits,
            "streams": args.streams,
            "outputs_per_launch": stats[-1].get("outputs_per_launch"),
            "ms_per_ode_step": (dt / args.steps) / (h_apps / args.steps / len(probs)) * 1e3,
            "h_applications_per_step": h_apps / args.steps,
            "parallelism": f"evolution-sharded x{world} ({args.scaling} scaling, no collectives)",
            "span_problems": stats[-1].get("span_problems"),
        },
        "roofline": roof,
    }
    if args.full and not args.no_full:
        phase("full_sweep (30 s grid)")
        try:
            line["full_sweep"] = full_sweep(eng, probs, len(my_det) * world if args.scaling == "weak" else args.n_det,
                                            args.full_intervals, args.full_repeats, torch.cuda.synchronize, dist)
        except Exception as exc:  # report, never hide
            line["full_sweep"] = {"error": repr(exc)}
    if cpu is not None:
        line["cpu_baseline"] = cpu
    if args.full and rank == 0 and world == 1 and not args.no_shard8:
        try:
            phase("strong split predictions (2/4/8 GPUs)")
            line["strong_split"] = strong_split_legs(eng, args.n_sea, args.n_det)
        except Exception as exc:  # report, never hide
            line["strong_split"] = {"error": repr(exc)}
    eng.close()
    if args.full and rank == 0 and world == 1 and not args.no_config2:
        try:
            phase("config2")
            line["config2"] = config2_leg(local)
        except Exception as exc:  # report, never hide
            line["config2"] = {"error": repr(exc)}
    if args.full and rank == 0 and world == 1 and not args.no_refdefault:
        try:
            phase("reference_default")
            line["reference_default"] = reference_default_leg(local)
        except Exception as exc:  # report, never hide
            line["reference_default"] = {"error": repr(exc)}
    if args.full and rank == 0 and world == 1 and not args.no_large:
        try:
            phase("large_register")
            line["large_register"] = large_register(local)
        except Exception as exc:  # report, never hide
            line["large_register"] = {"error": repr(exc)}
    if args.full and world in (2, 4, 8) and not args.no_large:
        try:
            rep = partitioned_leg(rank, world, int(os.environ.get("LOCAL_RANK", "0")), dist,
                                  args.partitioned_timeout)
        except Exception as exc:  # report, never hide
            rep = {"error": repr(exc)}
        if rank == 0:
            line["partitioned"] = rep
    HEARTBEAT.stop()
    if rank == 0:
        detail = args.detail or None
        if detail:
            try:
                os.makedirs(os.path.dirname(os.path.abspath(detail)), exist_ok=True)
                with open(detail, "w") as f:
                    json.dump(line, f, indent=1)
            except OSError as exc:
                note(f"detail record not written: {exc!r}")
                detail = None
        print(json.dumps(compact_line(line, detail)), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
