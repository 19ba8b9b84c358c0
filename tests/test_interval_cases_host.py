"""Host side of tests/test_gpu_interval_cases.py: the registers of its cases, a Python mirror of what
dse_runtime.hip build_tables sorts a pb.Problem into for k_interval (tile size L >= 10), and the
Chebyshev degrees a time grid gives (dse_host.cpp cheb_series / cheb_rows), with the CPU tests that
every case's register has the table its class names and that the section-3 grids have the series
edges they are chosen for.  No device is touched: the degree prediction calls the host-only library
functions dse_spectral_bounds and dse_bessel_j (as tests/test_host.py does).

Layout of a k_interval tile (dse_interval.hip): TB = L - 4 thread bits b < TB, register bits TB <= b <
L, and for a 2-tile register (n = L + 1) the top bit L.
"""
import dataclasses
import math

import numpy as np
import pytest

from quantumsimulations_amd.engine import bessel_native, spectral_bounds_native
from test_gpu_parity import _random_problem
from test_gpu_site_obs import _imag_problem

TILES = (10, 11, 12, 13)
REG_BITS = 4


# ------------------------------------------------------------------------------ the tables k_interval reads
def kernel_flip(p):
    """p.flip as build_tables keeps it: a real part of at most 1e-15 of the coefficient's modulus (the
    rounding residue of cos(pi / 2)) is dropped."""
    f = np.array(p.flip, dtype=float)
    for c in (0, 2):
        drop = np.abs(f[:, c]) <= 1e-15 * np.hypot(f[:, c], f[:, c + 1])
        f[drop, c] = 0.0
    return f


def interval_table(p, L):
    """What build_tables sorts p into at tile size L (10 <= L <= 13, n = L or L + 1)."""
    n = p.n_qubits
    TB = L - REG_BITS
    assert L in TILES and n in (L, L + 1), (n, L)
    two = n == L + 1
    g = np.triu(np.asarray(p.pair, dtype=float), 1)
    f = kernel_flip(p)
    drive = [bool(np.any(f[b] != 0.0)) for b in range(n)]
    n_pairs_tt = int(np.count_nonzero(g[:TB, :TB]))
    assert n_pairs_tt <= 4 * TB, (n_pairs_tt, TB)   # S.it holds four thread pairs per iteration
    cross = g[:L, L] if two else np.zeros(L)
    n_pairs_hi = int(np.count_nonzero(cross))
    return {
        "n_pairs_tt": n_pairs_tt,
        "it_padding": 4 * TB - n_pairs_tt,   # zero slots of S.it past the list
        "thread_drives": [b for b in range(TB) if drive[b]],
        "sweep_pairs": int(np.count_nonzero(g[:TB, TB:L])),   # (thread bit, register bit)
        "rr_g": sorted((a, b) for a in range(REG_BITS) for b in range(a + 1, REG_BITS) if g[TB + a, TB + b] != 0.0),
        "rflip_mask": sum(1 << (b - TB) for b in range(TB, L) if drive[b]),
        "n_pairs_hi": n_pairs_hi,
        "n_flips_hi": int(two and drive[L]),
        "xg": [i for i in range(REG_BITS) if cross[TB + i] != 0.0],
        "xq": [j for j in range(TB) if cross[j] != 0.0],
        "xgen": bool(two and n_pairs_hi > 0),
        "xraw": bool(two and n_pairs_hi == 0),
        "imag": bool(np.all(f[:, 0] == 0.0) and np.all(f[:, 2] == 0.0)),
    }


def full_table(n, L, imag):
    """interval_table of a register with every coupling and every drive non-zero."""
    TB, two = L - REG_BITS, n == L + 1
    return {"n_pairs_tt": TB * (TB - 1) // 2, "it_padding": 4 * TB - TB * (TB - 1) // 2,
            "thread_drives": list(range(TB)), "sweep_pairs": TB * REG_BITS,
            "rr_g": [(a, b) for a in range(REG_BITS) for b in range(a + 1, REG_BITS)], "rflip_mask": 15,
            "n_pairs_hi": L if two else 0, "n_flips_hi": int(two), "xg": list(range(REG_BITS)) if two else [],
            "xq": list(range(TB)) if two else [], "xgen": two, "xraw": False, "imag": imag}


# ------------------------------------------------------------------------------ section 1 registers
#         L, tiles, form, seed
CASES1 = [(10, 1, "complex", 5111), (10, 1, "imag", 5112), (10, 2, "complex", 5113), (10, 2, "imag", 5114),
          (11, 1, "complex", 5211), (11, 1, "imag", 5212), (11, 2, "complex", 5213), (11, 2, "imag", 5214),
          (12, 1, "complex", 5311), (12, 1, "imag", 5312), (12, 2, "complex", 5313), (12, 2, "imag", 5314),
          (13, 1, "complex", 5411), (13, 1, "imag", 5412), (13, 2, "complex", 5413), (13, 2, "imag", 5414)]
SEED1 = {c[:3]: c[3] for c in CASES1}
assert len(set(SEED1.values())) == len(CASES1) == 16


def tile_bits_for(L, tiles):
    """Option tile_bits that gives a register of n = L + tiles - 1 qubits tiles of 2^L amplitudes."""
    return 13 if tiles == 1 else L


def problem1(L, tiles, form):
    """The section-1 register of a case and its reference key; rare_bit = n - 1."""
    n, seed = L + tiles - 1, SEED1[L, tiles, form]
    p = _random_problem(n, seed, rare_bit=n - 1) if form == "complex" else _imag_problem(n, seed)
    assert p.rare_bit == n - 1
    return p, (form, n, seed)


# ------------------------------------------------------------------------------ section 2 registers
CLASSES = ["flip_only", "decoupled", "pairs_no_drive", "cross_reg012", "cross_reg3", "cross_lanes", "cross_waves",
           "sparse", "no_drives", "residue", "above_residue"]
ALSO_L10 = ["flip_only", "pairs_no_drive", "cross_lanes"]
ONE_TILE = ["sparse", "no_drives", "flip_only"]
#         class, L, tiles
CASES2 = ([(cls, L, 2) for cls in CLASSES for L in (13, 11)] + [(cls, 10, 2) for cls in ALSO_L10] +
          [(cls, L, 1) for cls in ONE_TILE for L in (13, 10)])
assert len(CASES2) == 22 + 3 + 6 and len(set(CASES2)) == len(CASES2)
SEED2 = {c: 6001 + i for i, c in enumerate(CASES2)}


def class_problem(cls, L, tiles):
    """The register of a section-2 case and its reference key."""
    n, seed = L + tiles - 1, SEED2[cls, L, tiles]
    TB = L - REG_BITS
    top = L if tiles == 2 else L - 1   # 1-tile: register bit 3 stands in for the top bit
    if cls in ("residue", "above_residue"):
        assert tiles == 2
        p = _imag_problem(n, seed)
        flip = p.flip.copy()
        eps = 6e-17 if cls == "residue" else 1e-14
        flip[:, 0] = flip[:, 2] = eps * np.abs(flip[:, 1])
        return dataclasses.replace(p, flip=flip), (cls, n, seed)
    p = _random_problem(n, seed, rare_bit=n - 1)
    pair, flip = p.pair.copy(), p.flip.copy()

    def keep_crossing(rows):
        for i in range(L):
            if i not in rows:
                pair[i, L] = 0.0

    if cls == "flip_only":
        pair[:top, top] = 0.0
    elif cls == "decoupled":
        pair[:, L] = 0.0
        flip[L] = 0.0
    elif cls == "pairs_no_drive":
        flip[L] = 0.0
    elif cls == "cross_reg012":
        keep_crossing([TB, TB + 1, TB + 2])
    elif cls == "cross_reg3":
        keep_crossing([TB + 3])
    elif cls == "cross_lanes":
        keep_crossing(range(min(TB, 6)))
    elif cls == "cross_waves":
        assert TB > 6
        keep_crossing(range(6, TB))
    elif cls == "sparse":
        for b in range(n):
            if b not in (0, 3, TB + 2, top):
                flip[b] = 0.0
        pair[1, :TB] = 0.0
        pair[:TB, 1] = 0.0
        keep = pair[TB, TB + 3]
        pair[TB:L, TB:L] = 0.0
        pair[TB, TB + 3] = keep
    elif cls == "no_drives":
        flip[:] = 0.0
    else:
        raise ValueError(cls)
    assert cls in ONE_TILE or tiles == 2
    return dataclasses.replace(p, pair=pair, flip=flip), (cls, n, seed)


def class_table(cls, L, tiles):
    """interval_table of the class, by construction."""
    n, TB = L + tiles - 1, L - REG_BITS
    T = full_table(n, L, cls in ("no_drives", "residue"))
    if cls == "flip_only" and tiles == 2:
        T.update(n_pairs_hi=0, xg=[], xq=[], xgen=False, xraw=True)
    elif cls == "flip_only":   # register bit 3 keeps its drive and loses its pairs
        T.update(sweep_pairs=3 * TB, rr_g=[(0, 1), (0, 2), (1, 2)])
    elif cls == "decoupled":
        T.update(n_pairs_hi=0, n_flips_hi=0, xg=[], xq=[], xgen=False, xraw=True)
    elif cls == "pairs_no_drive":
        T.update(n_flips_hi=0)
    elif cls == "cross_reg012":
        T.update(n_pairs_hi=3, xg=[0, 1, 2], xq=[])
    elif cls == "cross_reg3":
        T.update(n_pairs_hi=1, xg=[3], xq=[])
    elif cls == "cross_lanes":
        T.update(n_pairs_hi=min(TB, 6), xg=[], xq=list(range(min(TB, 6))))
    elif cls == "cross_waves":
        T.update(n_pairs_hi=TB - 6, xg=[], xq=list(range(6, TB)))
    elif cls == "sparse":
        tt = TB * (TB - 1) // 2 - (TB - 1)
        T.update(n_pairs_tt=tt, it_padding=4 * TB - tt, thread_drives=[0, 3], rr_g=[(0, 3)],
                 rflip_mask=(1 << 2) | ((1 << 3) if tiles == 1 else 0))
    elif cls == "no_drives":
        T.update(thread_drives=[], rflip_mask=0, n_flips_hi=0)
    return T


# ------------------------------------------------------------------------------ Chebyshev degrees
def series_degree(z, tol=1e-14):
    """The degree cheb_series gives e^{-i H tau} at z = alpha tau."""
    kmax = int(math.ceil(z + 12.0 * np.cbrt(z + 1.0) + 60.0))
    return int(bessel_native(z, kmax, tol)[1])


def half_width(p):
    lo, hi = spectral_bounds_native(p)
    return max(0.5 * (hi - lo), 1e-300)


def chosen_m(probs, t, m):
    """M of an evolve of probs on k_interval with option outputs_per_launch = m (choose_outputs_per_launch):
    1 on a coarse grid (alpha dt >= 400 for some register and interval)."""
    z = max(half_width(p) * float(np.max(np.diff(t))) for p in probs)
    return max(1, min(m, len(t) - 1)) if z < 400.0 else 1


def predicted_degrees(p, t, M, tol=1e-14):
    """(per launch group of M outputs the tuple of d_j, K): d_j the degree of the series of offset
    t[m0 + j + 1] - t[m0], K their maximum, which every launch of the evolve runs (P.degree)."""
    alpha = half_width(p)
    groups = []
    for m0 in range(0, len(t) - 1, M):
        n_out = min(M, len(t) - 1 - m0)
        groups.append(tuple(series_degree(alpha * (t[m0 + j + 1] - t[m0]), tol) for j in range(n_out)))
    return groups, max(max(g) for g in groups)


def predicted_max_degree(probs, t, M, tol=1e-14):
    """stats max_degree of an evolve of probs: the largest K."""
    return max(predicted_degrees(p, t, M, tol)[1] for p in probs)


# uneven grids: T6 five intervals (at M = 2 launches of 2, 2, 1 outputs), T8 seven (2, 2, 2, 1), its
# spacings chosen on the CPU so that both section-3 registers meet series_edges below
T6 = np.array([0.0, 1e-4, 1.5e-4, 3e-4, 3.2e-4, 5e-4])
T8 = np.array([0.0, 1.07e-4, 1.69e-4, 1.97e-4, 3.10e-4, 3.92e-4, 4.24e-4, 4.55e-4])
SECTION3 = [(13, 2, "complex"), (11, 2, "imag")]


def series_edges(p, t):
    """The conditions section 3 needs of (register, grid) at M = 2; raises AssertionError otherwise."""
    groups, K = predicted_degrees(p, t, 2)
    assert len(t) == 8 and [len(g) for g in groups] == [2, 2, 2, 1]   # a lone trailing output
    for j, n_g in ((0, 4), (1, 3)):   # the last update of output j carries 3, 1 and 2 terms somewhere
        d = [g[j] for g in groups if len(g) > j]
        assert len(d) == n_g and {(x - 1) % 3 for x in d} == {0, 1, 2}, (j, d)
    assert any(max(g) < K for g in groups), (groups, K)   # a launch whose outputs both end before K
    groups1, K1 = predicted_degrees(p, t, 1)
    assert {(g[0] - 1) % 3 for g in groups1} == {0, 1, 2} and any(g[0] < K1 for g in groups1)
    return groups, K


def coarse_problem():
    """Section 3's coarse case: a complex 2-tile register at L = 10 and 3 outputs with alpha dt >= 400."""
    p = _random_problem(11, 5511, rare_bit=10)
    dt = 420.0 / half_width(p)
    return p, ("coarse", 11, 5511), np.array([0.0, dt, 2.1 * dt])


# ------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("L,tiles,form,seed", CASES1)
def test_section1_tables_are_full(L, tiles, form, seed):
    p, _ = problem1(L, tiles, form)
    TB = L - REG_BITS
    T = interval_table(p, L)
    assert T == full_table(p.n_qubits, L, form == "imag")
    assert T["n_pairs_tt"] == TB * (TB - 1) // 2
    assert (T["it_padding"] == 0) == (L == 13)   # at L = 13 the list fills S.it exactly: 36 = 4 * 9


@pytest.mark.parametrize("cls,L,tiles", CASES2)
def test_class_tables(cls, L, tiles):
    p, _ = class_problem(cls, L, tiles)
    T = interval_table(p, L)
    assert T == class_table(cls, L, tiles), T
    # the path of each class (ISSUE table): raw hand-off with and without a top drive, pre-pass with
    # n_flips_hi 0 and 1, the pre-pass's pair families one at a time
    if tiles == 2:
        assert T["xraw"] == (cls in ("flip_only", "decoupled")) and T["xgen"] != T["xraw"]
        assert T["n_flips_hi"] == (0 if cls in ("decoupled", "pairs_no_drive", "no_drives") else 1)
    else:
        assert not T["xgen"] and not T["xraw"] and T["n_pairs_hi"] == 0
    if cls == "cross_waves":
        assert T["xq"] and min(T["xq"]) >= 6
    if cls == "cross_lanes":
        assert T["xq"] and max(T["xq"]) < 6 and not T["xg"]
    if cls == "sparse":
        assert T["it_padding"] > 0 and len(T["rr_g"]) == 1 and 0 < T["rflip_mask"] < 15
    # Hermitian tables: the two rows of a drive are conjugates
    assert np.array_equal(p.flip[:, 0], p.flip[:, 2]) and np.array_equal(p.flip[:, 1], -p.flip[:, 3])


def test_residue_rule():
    """6e-17 |im| is dropped (IMAG build), 1e-14 |im| is kept (general build); the given tables differ
    from the kept ones by the residue alone."""
    for L in (13, 11):
        lo, _ = class_problem("residue", L, 2)
        hi, _ = class_problem("above_residue", L, 2)
        assert np.all(lo.flip[:, 0] > 0.0) and np.all(hi.flip[:, 0] > 0.0)
        assert np.all(kernel_flip(lo)[:, (0, 2)] == 0.0) and np.array_equal(kernel_flip(lo)[:, (1, 3)], lo.flip[:, (1, 3)])
        assert np.array_equal(kernel_flip(hi), hi.flip)
        assert interval_table(lo, L)["imag"] and not interval_table(hi, L)["imag"]


def test_it_list_bound():
    for L in TILES:
        TB = L - REG_BITS
        assert TB * (TB - 1) // 2 <= 4 * TB


@pytest.mark.parametrize("L,tiles,form", SECTION3)
def test_section3_grid_has_the_series_edges(L, tiles, form):
    p, _ = problem1(L, tiles, form)
    assert np.ptp(np.diff(T8)) > 0.0
    groups, K = series_edges(p, T8)
    assert chosen_m([p], T8, 2) == 2 and chosen_m([p], T8, 1) == 1
    assert K == predicted_max_degree([p], T8, 2)


def test_coarse_grid():
    p, _, t = coarse_problem()
    alpha = half_width(p)
    assert p.n_qubits == 11 and len(t) == 3 and not interval_table(p, 10)["imag"]
    assert np.all(alpha * np.diff(t) >= 400.0)
    assert chosen_m([p], t, 2) == 1
    groups, K = predicted_degrees(p, t, 1)
    assert [len(g) for g in groups] == [1, 1] and K > 400
    assert 0.01 < t[-1] < 0.2   # seconds of expm_multiply at dimension 2048, not minutes


def test_series_degree_rule():
    """d grows with z, is at least 1, and J_d is the last coefficient above tol."""
    assert series_degree(0.0) == 1
    ds = [series_degree(z) for z in (0.5, 3.0, 20.0, 150.0, 450.0)]
    assert ds == sorted(ds) and ds[-1] > 450
    z = 20.0
    J, d = bessel_native(z, 200, 1e-14)
    assert d == series_degree(z) and abs(J[d]) > 1e-14 and np.all(np.abs(J[d + 1:]) <= 1e-14)
