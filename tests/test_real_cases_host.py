"""Host side of tests/test_gpu_real_cases.py: the registers of its cases, a Python restatement of what
dse_runtime.hip build_real_table sorts a raw-table pb.Problem of 13 or 14 qubits into for k_real
(dse_real.hip), and the CPU tests that every case's register has the table its class
names, that the restated table applied the way the kernel applies it is D H D^dagger of
problem_to_csr, and that the section-3 grids have the series edges they are chosen for.  No device is
touched (the degree prediction is tests/test_interval_cases_host.py's).

Layout of a k_real register (dse_real.hip): TB = 9 thread bits b < 9, RB = n - 9 register bits 9 <= b
< n, the top register bit n - 1 (register index TOP = RB - 1) splitting a thread's rows into halves.
"""
import dataclasses

import numpy as np
import pytest
import scipy.sparse as sp

from quantumsimulations_amd.dipolar_ensemble_with_rare import problem_to_csr
from test_gpu_parity import _rand, _random_problem
from test_gpu_site_obs import _imag_problem
from test_interval_cases_host import T6, chosen_m, half_width, predicted_degrees, predicted_max_degree

TB = 9
MAX_RB = 5                      # kRealRB: register bits at n = 14
N_RR = MAX_RB * (MAX_RB - 1) // 2
FROM_BUFFER = (1 << 64) - 1     # kRealFromBuffer: a custom psi(t0)
SIZES = (14, 13)


# ------------------------------------------------------------------------------ the tables k_real reads
def real_rr_index(a, b):
    """dse_internal.h real_rr_index: slot of the register pair a < b < 5."""
    assert 0 <= a < b < MAX_RB
    return a * (2 * MAX_RB - a - 1) // 2 + (b - a - 1)


def real_table(p, custom_init=False):
    """build_real_table's RealTab of p (n = 13 or 14) in the rotated frame D|x> = i^|x| |x>:
    it[j] = (drive of thread bit j by output value 0, 1; pairs (j, register bit 0 .. 5); the four
    thread pairs of iteration j), rr_g, rflip by output value, rflip_mask, x0, x0pop.  Raises
    ValueError for a drive with a real part above the 1e-15 residue."""
    n = p.n_qubits
    RB = n - TB
    if not 4 <= RB <= MAX_RB:
        raise ValueError(f"k_real holds 13 or 14 qubits, not {n}")
    it = np.zeros((TB, 12))
    rr_g = np.zeros(N_RR)
    rflip = np.zeros((MAX_RB, 2))
    mask = 0
    pair = np.asarray(p.pair, dtype=float)
    for i in range(n):
        for j in range(i + 1, n):
            g = -pair[i, j]                     # i^{+-2}
            if g == 0.0:
                continue
            if j < TB:                          # canonical slot, four thread pairs per iteration
                s = i * TB - i * (i + 1) // 2 + (j - i - 1)
                it[s // 4, 8 + s % 4] = g
            elif i < TB:
                it[i, 2 + (j - TB)] = g
            else:
                rr_g[real_rr_index(i - TB, j - TB)] = g
    for b in range(n):
        f = np.array(p.flip[b], dtype=float)
        for c in (0, 2):                        # the residue of cos(pi / 2) is dropped
            if abs(f[c]) <= 1e-15 * np.hypot(f[c], f[c + 1]):
                f[c] = 0.0
        if f[0] != 0.0 or f[2] != 0.0:
            raise ValueError(f"drive of bit {b} is not imaginary")
        if f[1] == 0.0 and f[3] == 0.0:
            continue
        if b < TB:                              # output value 0: i^-1 (i im0); 1: i (i im1)
            it[b, 0], it[b, 1] = f[1], -f[3]
        else:
            rflip[b - TB] = f[1], -f[3]
            mask |= 1 << (b - TB)
    x0 = FROM_BUFFER if custom_init else int(p.psi0_index)
    return {"it": it, "rr_g": rr_g, "rflip": rflip, "rflip_mask": mask, "x0": x0,
            "x0pop": 0 if custom_init else bin(x0).count("1")}


THREAD_PAIRS = [(a, b) for a in range(TB) for b in range(a + 1, TB)]   # real_pair_mask's order
assert len(THREAD_PAIRS) == 4 * TB


def pattern(T):
    """The zero / non-zero pattern of a real_table: which slots hold a coefficient."""
    it = T["it"]
    return {"thread_drives": [j for j in range(TB) if it[j, 0] != 0.0 or it[j, 1] != 0.0],
            "thread_reg": [(j, i) for j in range(TB) for i in range(6) if it[j, 2 + i] != 0.0],
            "thread_pairs": [(j, q) for j in range(TB) for q in range(4) if it[j, 8 + q] != 0.0],
            "rr_g": [s for s in range(N_RR) if T["rr_g"][s] != 0.0],
            "rflip": [i for i in range(MAX_RB) if T["rflip"][i, 0] != 0.0 or T["rflip"][i, 1] != 0.0],
            "rflip_mask": T["rflip_mask"]}


def table_pattern(n, thread_pairs, thread_reg, reg_pairs, drives):
    """pattern() of a register holding the given pairs of bits and drives, from the kernel's side:
    the slot of a thread pair is its place in real_pair_mask's lexicographic list."""
    RB = n - TB
    assert all(a < b < TB for a, b in thread_pairs) and all(j < TB <= b < n for j, b in thread_reg)
    assert all(TB <= a < b < n for a, b in reg_pairs)
    slots = sorted(divmod(THREAD_PAIRS.index(ab), 4) for ab in thread_pairs)
    rr = []
    for a, b in reg_pairs:   # slots of the 5-bit triangle, row by row
        a, b = a - TB, b - TB
        rr.append(sum(MAX_RB - 1 - k for k in range(a)) + (b - a - 1))
    reg_drives = sorted(b - TB for b in drives if b >= TB)
    assert all(i < RB for i in reg_drives)
    return {"thread_drives": sorted(b for b in drives if b < TB),
            "thread_reg": sorted((j, b - TB) for j, b in thread_reg), "thread_pairs": slots, "rr_g": sorted(rr),
            "rflip": reg_drives, "rflip_mask": sum(1 << i for i in reg_drives)}


def rotated_apply(T, n, w):
    """(H' - diagonal) w with the coefficients of a real_table, term by term as k_real applies them:
    a drive by the output row's bit value, a pair on the rows whose two bits are equal."""
    x = np.arange(1 << n)
    bit = lambda b: (x >> b) & 1
    out = np.zeros_like(w)
    for j in range(TB):
        row = T["it"][j]
        out += np.where(bit(j) == 0, row[0], row[1]) * w[x ^ (1 << j)]
        for i in range(n - TB):
            out += np.where(bit(j) == bit(TB + i), row[2 + i], 0.0) * w[x ^ (1 << j) ^ (1 << (TB + i))]
        for q in range(4):
            a, b = THREAD_PAIRS[4 * j + q]
            out += np.where(bit(a) == bit(b), row[8 + q], 0.0) * w[x ^ (1 << a) ^ (1 << b)]
    for i in range(n - TB):
        if (T["rflip_mask"] >> i) & 1:
            out += np.where(bit(TB + i) == 0, T["rflip"][i, 0], T["rflip"][i, 1]) * w[x ^ (1 << (TB + i))]
        for k in range(i + 1, n - TB):
            g = T["rr_g"][real_rr_index(i, k)]
            out += np.where(bit(TB + i) == bit(TB + k), g, 0.0) * w[x ^ (1 << (TB + i)) ^ (1 << (TB + k))]
    return out


def rotated_offdiagonal(p):
    """D H D^dagger - its diagonal from problem_to_csr, D = diag(i^popcount); real for imaginary drives."""
    n = p.n_qubits
    H = problem_to_csr(p).tocoo()
    pop = np.array([bin(v).count("1") for v in range(1 << n)])
    vals = H.data * np.array([1.0, 1j, -1.0, -1j])[(pop[H.row] - pop[H.col]) % 4]
    off = H.row != H.col
    return sp.csr_matrix((vals[off], (H.row[off], H.col[off])), shape=H.shape)


# ------------------------------------------------------------------------------ section 1 registers
SEED1 = {14: 7114, 13: 7113}
#        n, x0: popcount = 0, 1, 2, 3 (mod 4) at either size, |0> and |1..1> among them
CASES1 = [(14, 0), (14, (1 << 0) | (1 << 4) | (1 << 8) | (1 << 9) | (1 << 13)), (14, (1 << 14) - 1),
          (14, (1 << 2) | (1 << 10) | (1 << 12)),
          (13, 0), (13, (1 << 13) - 1), (13, (1 << 3) | (1 << 12)), (13, (1 << 1) | (1 << 8) | (1 << 11))]
assert len(CASES1) == 8


def problem1(n, x0=None):
    """The full imaginary-drive register of size n (every coupling and drive non-zero, rare_bit = n - 1)
    from the basis state x0 (None: the random one of the tables), and its reference key."""
    p = _imag_problem(n, SEED1[n])
    if x0 is not None:
        p = dataclasses.replace(p, psi0_index=int(x0))
    return p, ("full", n, SEED1[n], int(p.psi0_index))


# ------------------------------------------------------------------------------ section 2 registers
CLASSES = ["thread_pairs_only", "thread_reg_low_only", "thread_top_only", "reg_low_only", "reg_top_only",
           "drive_top_only", "drive_reg_partial", "drive_threads_sparse", "no_drives", "diagonal", "residue"]
CASES2 = [(cls, n) for cls in CLASSES for n in SIZES]
assert len(CASES2) == 22
SEED2 = {c: 8001 + i for i, c in enumerate(CASES2 + [("above_residue", 14), ("above_residue", 13)])}
# the pair classes keep every drive (the state reaches every row) and one kind of pair; the drive classes
# keep every pair and the drives they name
PAIR_CLASSES = CLASSES[:5]


def _kinds(n):
    """The five kinds of pairs (a, b), a < b, of a k_real register."""
    top = n - 1
    return {"thread_pairs_only": list(THREAD_PAIRS),
            "thread_reg_low_only": [(j, b) for j in range(TB) for b in range(TB, top)],
            "thread_top_only": [(j, top) for j in range(TB)],
            "reg_low_only": [(a, b) for a in range(TB, top) for b in range(a + 1, top)],
            "reg_top_only": [(a, top) for a in range(TB, top)]}


def _class_content(cls, n):
    """(pairs by kind, driven bits) of the class, by construction."""
    kinds = _kinds(n)
    drives = list(range(n))
    if cls in PAIR_CLASSES:
        kinds = {k: (v if k == cls else []) for k, v in kinds.items()}
    elif cls == "drive_top_only":
        drives = [n - 1]
    elif cls == "drive_reg_partial":
        drives = [TB, TB + 2]
    elif cls == "drive_threads_sparse":
        drives = [0, 3, 8]
        kinds["thread_pairs_only"] = [ab for ab in THREAD_PAIRS if 1 not in ab]
    elif cls == "no_drives":
        drives = []
    elif cls == "diagonal":
        kinds, drives = {k: [] for k in kinds}, []
    else:
        assert cls in ("residue", "above_residue"), cls
    return kinds, drives


def class_problem(cls, n):
    """The register of a section-2 case, from the full imaginary-drive random problem by zeroing entries,
    and its reference key."""
    seed = SEED2[cls, n]
    p = _imag_problem(n, seed)
    kinds, drives = _class_content(cls, n)
    keep = np.zeros((n, n), dtype=bool)
    for pairs in kinds.values():
        for a, b in pairs:
            keep[a, b] = True
    pair = np.where(keep, p.pair, 0.0)
    flip = p.flip.copy()
    for b in range(n):
        if b not in drives:
            flip[b] = 0.0
    if cls in ("residue", "above_residue"):
        flip[:, 0] = flip[:, 2] = (6e-17 if cls == "residue" else 1e-14) * np.abs(flip[:, 1])
    return dataclasses.replace(p, pair=pair, flip=flip), (cls, n, seed)


def class_table(cls, n):
    """pattern(real_table(.)) of the class, by construction."""
    kinds, drives = _class_content(cls, n)
    return table_pattern(n, kinds["thread_pairs_only"], kinds["thread_reg_low_only"] + kinds["thread_top_only"],
                         kinds["reg_low_only"] + kinds["reg_top_only"], drives)


def has_thread_pairs(cls):
    return cls not in ("thread_reg_low_only", "thread_top_only", "reg_low_only", "reg_top_only", "diagonal")


def general_state(n, seed):
    """A normalised, fully complex psi0."""
    return _rand(n, seed)


def product_amps(n, seed):
    """(n, 2) complex single-spin amplitudes, each spin normalised."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
    return a / np.linalg.norm(a, axis=1)[:, None]


# ------------------------------------------------------------------------------ section 3 grids
# seven uneven intervals (at M = 2 launches of 2, 2, 2, 1 outputs), chosen on the CPU from predicted_degrees
# alone so that both section-1 registers meet series_edges below
T8R = np.array([0.0, 5.7e-5, 1.30e-4, 1.69e-4, 2.36e-4, 2.82e-4, 3.35e-4, 4.39e-4])


def series_edges(p, t):
    """The conditions section 3 needs of (register, grid); raises AssertionError otherwise."""
    groups, K = predicted_degrees(p, t, 2)
    assert len(t) == 8 and [len(g) for g in groups] == [2, 2, 2, 1]   # a final one-output launch: phase5<1>
    for j, n_g in ((0, 4), (1, 3)):   # the last update of output j carries 3, 1 and 2 terms somewhere
        d = [g[j] for g in groups if len(g) > j]
        assert len(d) == n_g and {(x - 1) % 3 for x in d} == {0, 1, 2}, (j, d)
    # output 0 ends before the launch's K while output 1 still updates: its sums pass through phase5<2>
    assert any(len(g) == 2 and g[0] < g[1] <= K for g in groups), (groups, K)
    groups1, K1 = predicted_degrees(p, t, 1)
    assert {(g[0] - 1) % 3 for g in groups1} == {0, 1, 2} and any(g[0] < K1 for g in groups1)
    return groups, K


def coarse_problem():
    """Section 3's coarse case: the n = 13 register and 3 outputs with alpha dt >= 400."""
    p, key = problem1(13)
    dt = 420.0 / half_width(p)
    return p, key, np.array([0.0, dt, 2.1 * dt])


# ------------------------------------------------------------------------------ section 5 registers
MIXED = [(14, 7514, 1.0), (13, 7513, 1.5), (14, 7524, 0.55), (13, 7523, 0.8), (14, 7534, 1.5)]


def scaled(p, f):
    return dataclasses.replace(p, field=p.field * f, zz=p.zz * f, pair=p.pair * f, flip=p.flip * f, shift=p.shift * f)


def mixed_problems():
    """Five imaginary-drive registers, n = 13 and 14 mixed, their tables scaled to unequal degrees."""
    probs = [scaled(_imag_problem(n, seed), f) for n, seed, f in MIXED]
    return probs, [("mixed", n, seed, f) for n, seed, f in MIXED]


def fallback_problems(kind):
    """The registers of a choose_real fall-back: two k_real-eligible ones and the one that is not."""
    (a, ka), (b, kb) = problem1(14), problem1(13)
    if kind == "complex":
        c, kc = _random_problem(13, 7613, rare_bit=12), ("complex", 13, 7613)
    elif kind == "n12":
        c, kc = _imag_problem(12, 7612), ("imag", 12, 7612)
    elif kind == "above_residue":
        c, kc = class_problem("above_residue", 14)
    else:
        raise ValueError(kind)
    return [a, c, b], [ka, kc, kb]


# ------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("n", SIZES)
def test_full_table(n):
    """Every slot of RealTab the size uses is non-zero and the coefficients are pairwise distinct, so a
    permuted slot changes H."""
    p, _ = problem1(n)
    assert p.rare_bit == n - 1
    T = real_table(p)
    RB = n - TB
    P = pattern(T)
    kinds = _kinds(n)
    assert P == table_pattern(n, kinds["thread_pairs_only"], kinds["thread_reg_low_only"] + kinds["thread_top_only"],
                              kinds["reg_low_only"] + kinds["reg_top_only"], list(range(n)))
    assert len(P["thread_pairs"]) == 36 and len(P["thread_reg"]) == TB * RB and len(P["rr_g"]) == RB * (RB - 1) // 2
    assert P["rflip_mask"] == (1 << RB) - 1 and P["thread_drives"] == list(range(TB))
    g = np.abs(np.triu(p.pair, 1)[np.triu_indices(n, 1)])
    d = np.abs(p.flip[:, 1])
    assert np.all(g > 0.0) and np.all(d > 0.0)
    assert len(np.unique(g)) == len(g) and len(np.unique(d)) == n
    # Hermitian tables: the two rotated rows of a drive are equal (i^-1 (i a) = i (-i a)), so
    # rflip[i][0] == rflip[i][1] and no Hermitian problem tells the kernel's two drive rows apart
    assert np.array_equal(T["rflip"][:RB, 0], T["rflip"][:RB, 1]) and np.array_equal(T["it"][:, 0], T["it"][:, 1])


@pytest.mark.parametrize("n,x0", CASES1)
def test_section1_start_states(n, x0):
    p, _ = problem1(n, x0)
    T = real_table(p)
    assert T["x0"] == x0 and T["x0pop"] == bin(x0).count("1")
    per_size = [bin(x).count("1") % 4 for m, x in CASES1 if m == n]
    assert sorted(per_size) == [0, 1, 2, 3]
    assert {x for m, x in CASES1 if m == n} >= {0, (1 << n) - 1}
    assert chosen_m([p], T6, 2) == 2 and [len(g) for g in predicted_degrees(p, T6, 2)[0]] == [2, 2, 1]


@pytest.mark.parametrize("cls,n", CASES2)
def test_class_tables(cls, n):
    p, _ = class_problem(cls, n)
    T = real_table(p)
    P = pattern(T)
    assert P == class_table(cls, n), P
    RB, top = n - TB, n - TB - 1
    full = pattern(real_table(problem1(n)[0]))
    if cls in PAIR_CLASSES:   # one non-empty kind of pair, every drive
        assert P["thread_drives"] == full["thread_drives"] and P["rflip_mask"] == full["rflip_mask"]
        sizes = {"thread_pairs": len(P["thread_pairs"]), "thread_reg_low": sum(1 for _, i in P["thread_reg"] if i < top),
                 "thread_top": sum(1 for _, i in P["thread_reg"] if i == top),
                 "reg_low": sum(1 for s in P["rr_g"] if s not in [real_rr_index(a, top) for a in range(top)]),
                 "reg_top": sum(1 for s in P["rr_g"] if s in [real_rr_index(a, top) for a in range(top)])}
        want = {"thread_pairs_only": ("thread_pairs", 36), "thread_reg_low_only": ("thread_reg_low", TB * (RB - 1)),
                "thread_top_only": ("thread_top", TB), "reg_low_only": ("reg_low", (RB - 1) * (RB - 2) // 2),
                "reg_top_only": ("reg_top", RB - 1)}[cls]
        assert sizes == {k: (want[1] if k == want[0] else 0) for k in sizes}, sizes
    elif cls == "drive_top_only":
        assert P["rflip_mask"] == 1 << top and not P["thread_drives"]
    elif cls == "drive_reg_partial":
        assert P["rflip_mask"] == 0b101 and not P["thread_drives"]
    elif cls == "drive_threads_sparse":
        assert P["thread_drives"] == [0, 3, 8] and P["rflip_mask"] == 0
        assert len(P["thread_pairs"]) == 36 - 8 and all(1 not in THREAD_PAIRS[4 * j + q] for j, q in P["thread_pairs"])
    elif cls == "no_drives":
        assert P["rflip_mask"] == 0 and not P["thread_drives"] and not np.any(p.flip)
    elif cls == "diagonal":
        assert not any(P[k] for k in P) and np.all(p.field != 0.0)
        assert np.count_nonzero(np.triu(p.zz, 1)) == n * (n - 1) // 2
    if cls not in PAIR_CLASSES + ["diagonal"]:
        assert P["thread_reg"] == full["thread_reg"] and P["rr_g"] == full["rr_g"]
    assert has_thread_pairs(cls) == bool(P["thread_pairs"])
    # Hermitian tables
    assert np.array_equal(p.flip[:, 0], p.flip[:, 2]) and np.array_equal(p.flip[:, 1], -p.flip[:, 3])


@pytest.mark.parametrize("cls,n", [("full", 14), ("full", 13), ("drive_threads_sparse", 14), ("reg_top_only", 13),
                                   ("residue", 14)])
def test_restated_table_is_the_rotated_hamiltonian(cls, n):
    """real_table's coefficients, applied row by row as k_real applies them, give D H D^dagger of
    problem_to_csr off the diagonal: within rounding of the sums (2^-50 of the largest row 1-norm times
    max |w|); for the residue class the dropped real parts add at most 6e-17 of the same."""
    p = problem1(n)[0] if cls == "full" else class_problem(cls, n)[0]
    Hr = rotated_offdiagonal(p)
    rng = np.random.default_rng(n)
    w = rng.standard_normal(1 << n)
    got = rotated_apply(real_table(p), n, w)
    want = Hr @ w
    scale = float(abs(Hr).sum(axis=1).max() * np.max(np.abs(w)))
    bound = (2.0 ** -50 + (6e-17 if cls == "residue" else 0.0)) * scale
    if cls != "residue":
        assert np.all(Hr.data.imag == 0.0)
    err = float(np.max(np.abs(got - want)))
    print(f"{cls} n = {n}: max |table apply - D H D^dagger w| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_residue_rule_and_refusal():
    """6e-17 |im| is dropped and the register stays on k_real's tables; 1e-14 |im|, and a complex drive
    on any one bit, are refused."""
    for n in SIZES:
        lo, _ = class_problem("residue", n)
        hi, _ = class_problem("above_residue", n)
        assert np.all(lo.flip[:, 0] > 0.0) and np.all(hi.flip[:, 0] > 0.0)
        full = dataclasses.replace(lo, flip=np.stack([0 * lo.flip[:, 1], lo.flip[:, 1], 0 * lo.flip[:, 1], lo.flip[:, 3]], 1))
        a, b = real_table(lo), real_table(full)
        assert all(np.array_equal(a[k], b[k]) for k in ("it", "rr_g", "rflip")) and a["rflip_mask"] == b["rflip_mask"]
        with pytest.raises(ValueError):
            real_table(hi)
        for b_bad in (0, TB, n - 1):
            q, _ = problem1(n)
            flip = q.flip.copy()
            flip[b_bad, 0] = flip[b_bad, 2] = 1.0
            with pytest.raises(ValueError):
                real_table(dataclasses.replace(q, flip=flip))
    for n in (12, 15):
        with pytest.raises(ValueError):
            real_table(_imag_problem(n, 5))


def test_slots():
    """The closed-form slot of build_real_table is the place in real_pair_mask's list; real_rr_index
    fills the 5-bit triangle row by row; a custom psi(t0) has x0pop = 0."""
    for s, (a, b) in enumerate(THREAD_PAIRS):
        assert a * TB - a * (a + 1) // 2 + (b - a - 1) == s
    assert [real_rr_index(a, b) for a in range(MAX_RB) for b in range(a + 1, MAX_RB)] == list(range(N_RR))
    p, _ = problem1(14, (1 << 14) - 1)
    assert real_table(p)["x0pop"] == 14
    T = real_table(p, custom_init=True)
    assert T["x0"] == FROM_BUFFER and T["x0pop"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_section3_grid_has_the_series_edges(n):
    p, _ = problem1(n)
    assert np.ptp(np.diff(T8R)) > 0.0
    groups, K = series_edges(p, T8R)
    assert chosen_m([p], T8R, 2) == 2 and chosen_m([p], T8R, 1) == 1
    assert K == predicted_max_degree([p], T8R, 2)


def test_coarse_grid():
    p, _, t = coarse_problem()
    alpha = half_width(p)
    assert p.n_qubits == 13 and len(t) == 3
    assert np.all(alpha * np.diff(t) >= 400.0)
    assert chosen_m([p], t, 2) == 1
    groups, K = predicted_degrees(p, t, 1)
    assert [len(g) for g in groups] == [1, 1] and K > 400 and min(g[0] for g in groups) > 400


def test_mixed_and_fallback_contexts():
    probs, keys = mixed_problems()
    assert [p.n_qubits for p in probs] == [14, 13, 14, 13, 14] and len(set(keys)) == 5
    K = [predicted_degrees(p, T6, 2)[1] for p in probs]
    assert len(set(K)) == 5, K   # unequal degrees
    for p in probs:
        real_table(p)            # every one eligible
    for kind, n_bad in (("complex", 13), ("n12", 12), ("above_residue", 14)):
        fb, _ = fallback_problems(kind)
        assert [p.n_qubits for p in fb] == [14, n_bad, 13]
        real_table(fb[0]), real_table(fb[2])
        with pytest.raises(ValueError):
            real_table(fb[1])
