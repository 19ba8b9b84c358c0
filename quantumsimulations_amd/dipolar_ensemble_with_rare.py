"""Drop-in replacement for the reference's ``dipolar_ensemble_with_rare`` module.

Same public names and call contracts as TimHarrelson/QuantumSimulations'
``dipolar_ensemble_with_rare.py``; ``sweep_sea_detuning.py`` imports exactly
``DipolarRareParams, get_derived_frequencies, simulate_rare,
shell_positions_with_rare_center, dipolar_couplings_from_positions``
(sweep_sea_detuning.py:103-109), all provided here, with no QuTiP import.

``simulate_rare`` (reference :611-680) keeps its signature and return contract:
``(t, {"Ix_sea", "Iy_sea", "Iz_sea", "Iz_R", "Ix_R", "Iy_R", "state_norm"})``,
float64 arrays of length ``steps``, keys in that order.  The evolution runs on
an MI355X through libdse (exact Chebyshev propagation of the time-independent
rotating-frame H); the reference's ZVODE knobs (``solver_*``) do not apply to
an exact propagator and are accepted and ignored.  The truncation tolerance of
the Chebyshev series is ``DSE_TOL`` (default 1e-14).

Functions that return QuTiP objects in the reference return numpy / scipy.sparse
equivalents here (``build_hamiltonian_rare``, ``initial_state_rare``), in the
reference's basis order (site 0 = most significant bit).
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence, Tuple

import numpy as np
import scipy.sparse as sp

from .model import (  # noqa: F401  (re-exported API)
    DipolarRareParams,
    _platonic_vertices,
    dipolar_couplings_from_positions,
    get_derived_frequencies,
    shell_positions_with_rare_center,
)
from .problem import OBS_NAMES, Problem, build_problem, pair_traces_from_bits, site_traces_from_bits, time_grid

__all__ = [
    "DipolarRareParams", "get_derived_frequencies", "shell_positions_with_rare_center",
    "dipolar_couplings_from_positions", "simulate_rare", "simulate_rare_batch", "simulate_rare_sites",
    "simulate_rare_pairs",
    "build_hamiltonian_rare", "initial_state_rare", "dims_with_rare",
    "simulate_rare_from", "simulate_rare_sequence", "simulate_rare_overlaps", "rotation_matrices",
    "simulate_rare_strings", "op_strings_by_bit", "rdm_strings", "rdm_from_string_values",
    "simulate_rare_sectors", "sector_masks_by_bit", "mqc_intensities", "sector_moments",
]

_ENGINES: Dict[int, object] = {}


def _default_device() -> int:
    for key in ("DSE_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(key)
        if v is not None and v.strip() != "":
            return int(v)
    return 0


def _engine(device: int):
    from .engine import Engine  # loads libdse.so; raises if it is missing
    eng = _ENGINES.get(device)
    if eng is None:
        eng = Engine(device)
        _ENGINES[device] = eng
    return eng


def _tol() -> float:
    return float(os.environ.get("DSE_TOL", "1e-14"))


def dims_with_rare(n_sea: int, is_spin_three_half: bool = False) -> List[int]:
    """Local dimensions, dipolar_ensemble_with_rare.py:28-34."""
    return [2] * n_sea + ([4] if is_spin_three_half else [2])


SITE_NAMES: Tuple[str, ...] = ("Ix", "Iy", "Iz")


def simulate_rare_batch(params_list: Sequence[DipolarRareParams], device: int | None = None,
                        site_resolved: bool = False, pair_resolved: bool = False) -> List[Tuple]:
    """Many evolutions at once on one device (same results as calling simulate_rare on each).

    ``site_resolved=True``: every result is ``(t, obs, sites)`` with ``sites = {"Ix", "Iy", "Iz"}``,
    each ``(n_sites, steps)`` by reference site index (see simulate_rare_sites); ``t`` and ``obs``
    are what the default call returns.  ``pair_resolved=True``: every result is
    ``(t, obs, sites, pairs)`` with ``pairs = {"zz", "zq", "dq"}``, each ``(n_sites, n_sites, steps)``
    (see simulate_rare_pairs; it needs, and so includes, the site traces)."""
    site_resolved = site_resolved or pair_resolved
    device = _default_device() if device is None else device
    grids = [time_grid(p) for p in params_list]       # raises ValueError like :620-621
    probs = [build_problem(p, order="engine", reduce=True) for p in params_list]
    eng = _engine(device)
    results: List = [None] * len(params_list)
    # one engine call per distinct time grid and engine class (engine.evolve_groups)
    from .engine import batches_for_memory, evolve_groups
    by_grid = evolve_groups([(float(p.t_final), int(p.steps)) for p in params_list], probs)
    for key, idxs in by_grid.items():
        eng.clear()  # free the previous group's buffers before sizing this group's batches
        for batch in batches_for_memory([probs[i] for i in idxs], device):
            members = [idxs[b] for b in batch]
            eng.clear()
            for i in members:
                eng.add(probs[i])
            t = grids[members[0]]
            if site_resolved:
                # only for this call: the cached engine is shared with the default path
                eng.set_option("site_obs", 1)
            if pair_resolved:
                eng.set_option("pair_obs", 1)
            try:
                obs, _ = eng.evolve(t, tol=_tol())
                traces = [eng.site_traces(slot) for slot in range(len(members))] if site_resolved else None
                ptraces = [eng.pair_traces(slot) for slot in range(len(members))] if pair_resolved else None
            finally:
                if site_resolved:
                    eng.set_option("site_obs", 0)
                if pair_resolved:
                    eng.set_option("pair_obs", 0)
            for slot, i in enumerate(members):
                results[i] = (t.copy(), {name: obs[slot, j].copy() for j, name in enumerate(OBS_NAMES)})
                if site_resolved:
                    p = probs[i]
                    by_site = site_traces_from_bits(traces[slot], p.site_of_bit, p.n_sites, p.reduced,
                                                    p.rare_z_const)
                    results[i] += ({name: by_site[c].copy() for c, name in enumerate(SITE_NAMES)},)
                if pair_resolved:
                    p = probs[i]
                    results[i] += (pair_traces_from_bits(ptraces[slot], traces[slot], p.site_of_bit, p.n_sites,
                                                         p.reduced, p.rare_z_const),)
    eng.clear()
    return results


def simulate_rare(params: DipolarRareParams) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
    """Time grid and the six expectation traces + state norm (reference :611-680).

    ``state_norm`` always has length ``steps`` here (||psi(t)|| of the exactly propagated state).
    The reference computes it from ``res.states`` (:669); when no ``solver_*`` override is set it
    passes ``options=None`` and QuTiP 5, by its ``store_states`` default with ``e_ops`` given,
    likely stores no states, so its ``state_norm`` would be empty.  That default cannot be
    checked offline (QuTiP is absent: parity unpinned); the sweep always sets the overrides
    (sweep_sea_detuning.py:1247-1250), where both return one norm per output time."""
    return simulate_rare_batch([params])[0]


def simulate_rare_sites(params: DipolarRareParams
                        ) -> Tuple[np.ndarray, Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """simulate_rare plus the site-resolved traces: ``(t, obs, sites)``.

    ``sites = {"Ix": (n_sites, steps), "Iy": ..., "Iz": ...}``: <Ix_k>, <Iy_k>, <Iz_k> of the
    normalised state for every site k in the reference's site order (sea sites 0 .. n_sea - 1, the
    rare site last).  When the rare spin is frozen (center geometry, not driven: the register holds
    only the sea spins) its row is the constant Iz = -init_x_sign / 2, Ix = Iy = 0, as ``obs["Iz_R"]``.
    No reference counterpart: the reference returns only the seven aggregates."""
    return simulate_rare_batch([params], site_resolved=True)[0]


def simulate_rare_pairs(params: DipolarRareParams) -> Tuple[np.ndarray, Dict[str, np.ndarray],
                                                            Dict[str, np.ndarray], Dict[str, np.ndarray]]:
    """simulate_rare_sites plus the two-spin correlators: ``(t, obs, sites, pairs)``.

    ``pairs = {"zz", "zq", "dq"}``, each ``(n_sites, n_sites, steps)`` in the reference's site order:
    zz[k, l] = <Iz_k Iz_l> (real, symmetric), zq[k, l] = <I+_k I-_l> (Hermitian), dq[k, l] =
    <I+_k I+_l> (symmetric) of the normalised state, so <Ix_k Ix_l> = Re(zq + dq) / 2 and
    <Iy_k Iy_l> = Re(zq - dq) / 2.  Diagonals: zz = 1/4, zq = 1/2 + <Iz_k>, dq = 0.  When the rare
    spin is frozen its row and column are zz = Iz_R <Iz_k>, zq = dq = 0.
    No reference counterpart."""
    return simulate_rare_batch([params], pair_resolved=True)[0]


def problem_to_csr(prob: Problem) -> sp.csr_matrix:
    """Dense-free CSR of the H described by ``prob`` (host helper; small registers only)."""
    n = prob.n_qubits
    if n > 20:
        raise ValueError("CSR construction is limited to 20 qubits")
    dim = 1 << n
    x = np.arange(dim, dtype=np.int64)
    s = [0.5 - ((x >> b) & 1) for b in range(n)]
    diag = np.full(dim, prob.shift)
    for b in range(n):
        diag = diag + prob.field[b] * s[b]
    for i in range(n):
        for j in range(i + 1, n):
            if prob.zz[i, j] != 0.0:
                diag = diag + prob.zz[i, j] * (s[i] * s[j])
    rows, cols, vals = [x], [x], [diag.astype(complex)]
    for b in range(n):
        f = prob.flip[b]
        if np.any(f != 0.0):
            bit = (x >> b) & 1
            rows.append(x)
            cols.append(x ^ (1 << b))
            vals.append(np.where(bit == 0, f[0] + 1j * f[1], f[2] + 1j * f[3]))
    for i in range(n):
        for j in range(i + 1, n):
            g = prob.pair[i, j]
            if g != 0.0:
                eq = ((x >> i) & 1) == ((x >> j) & 1)
                rows.append(x[eq])
                cols.append(x[eq] ^ ((1 << i) | (1 << j)))
                vals.append(np.full(int(eq.sum()), g, dtype=complex))
    m = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(dim, dim))
    m.sum_duplicates()
    return m


def build_hamiltonian_rare(params: DipolarRareParams) -> Tuple[sp.csr_matrix, Dict[str, sp.csr_matrix]]:
    """H and the six observables as scipy.sparse matrices in the reference's basis order
    (site 0 = most significant bit), as the QuTiP objects of :453-588 would be."""
    prob = build_problem(params, order="reference", reduce=False)
    H = problem_to_csr(prob)
    n = prob.n_qubits
    dim = 1 << n
    x = np.arange(dim, dtype=np.int64)

    def z_of(bits):
        d = np.zeros(dim)
        for b in bits:
            d += 0.5 - ((x >> b) & 1)
        return sp.diags(d.astype(complex), format="csr")

    def xy_of(bits, comp):
        m = sp.csr_matrix((dim, dim), dtype=complex)
        for b in bits:
            bit = (x >> b) & 1
            if comp == "x":
                v = np.full(dim, 0.5, dtype=complex)
            else:  # <x^e_b| Iy |x>: +i/2 when the output bit is 1 (input bit 0), -i/2 otherwise
                v = np.where(bit == 0, 0.5j, -0.5j)
            m = m + sp.csr_matrix((v, (x ^ (1 << b), x)), shape=(dim, dim))
        return m

    sea_bits = [b for b in range(n) if (prob.sea_mask >> b) & 1]
    rare = [prob.rare_bit]
    obs = {"Ix_sea": xy_of(sea_bits, "x"), "Iy_sea": xy_of(sea_bits, "y"), "Iz_sea": z_of(sea_bits),
           "Iz_R": z_of(rare), "Ix_R": xy_of(rare, "x"), "Iy_R": xy_of(rare, "y")}
    return H, obs


def initial_state_rare(params: DipolarRareParams) -> np.ndarray:
    """Product initial state as a dense ket in the reference's basis order (:591-606)."""
    prob = build_problem(params, order="reference", reduce=False)
    v = np.zeros(1 << prob.n_qubits, dtype=complex)
    v[prob.psi0_index] = 1.0
    return v


# ---- evolutions from general initial states (no reference counterpart) -------------------------
# The reference always starts from the basis ket of initial_state_rare.  The helpers below start
# from any state of the n_sea + 1 spins: a dense ket in the reference's basis order, or a product
# state given spin by spin.  They build the unreduced register (``reduce=False``): the frozen-rare
# reduction of simulate_rare assumes the rare spin sits in a basis state.

def reference_to_engine_state(psi_ref: np.ndarray, site_of_bit: np.ndarray) -> np.ndarray:
    """A ket in the reference's basis order (site 0 = most significant bit) as the register state
    whose bit b holds site ``site_of_bit[b]``.  Pure numpy."""
    sob = np.asarray(site_of_bit, dtype=np.int64)
    n = sob.shape[0]
    v = np.asarray(psi_ref, dtype=np.complex128)
    if v.shape != (1 << n,) or sorted(sob.tolist()) != list(range(n)):
        raise ValueError(f"state must have shape ({1 << n},) and site_of_bit be a permutation of the sites")
    # tensor axis s of the reference ket = site s; axis k of the register state = bit n - 1 - k
    return np.ascontiguousarray(v.reshape((2,) * n).transpose([int(sob[n - 1 - k]) for k in range(n)])).reshape(-1)


def engine_to_reference_state(psi_eng: np.ndarray, site_of_bit: np.ndarray) -> np.ndarray:
    """Inverse of reference_to_engine_state."""
    sob = np.asarray(site_of_bit, dtype=np.int64)
    n = sob.shape[0]
    v = np.asarray(psi_eng, dtype=np.complex128)
    if v.shape != (1 << n,) or sorted(sob.tolist()) != list(range(n)):
        raise ValueError(f"state must have shape ({1 << n},) and site_of_bit be a permutation of the sites")
    axes = [int(sob[n - 1 - k]) for k in range(n)]  # register axis k holds site axes[k]
    return np.ascontiguousarray(v.reshape((2,) * n).transpose(np.argsort(axes))).reshape(-1)


def spin_amplitudes(spins, n_sites: int) -> np.ndarray:
    """(n_sites, 2) complex amplitudes on (up, down) per site from ``spins``: either that array
    itself, or (n_sites, 3) Bloch vectors (x, y, z) of any non-zero length, the spin pointing along
    them: (cos(theta / 2), e^{i phi} sin(theta / 2)), so +z is up, +x is (1, 1) / sqrt(2) and +y is
    (1, i) / sqrt(2) (<Ix>, <Iy>, <Iz> = the unit vector / 2)."""
    a = np.asarray(spins)
    if a.ndim != 2 or a.shape[0] != n_sites or a.shape[1] not in (2, 3):
        raise ValueError(f"spins must have shape ({n_sites}, 2) (amplitudes) or ({n_sites}, 3) (Bloch vectors)")
    if a.shape[1] == 2:
        out = np.array(a, dtype=np.complex128)
    else:
        if np.iscomplexobj(a):
            raise ValueError("Bloch vectors must be real")
        r = np.array(a, dtype=np.float64)
        if not np.all(np.isfinite(r)) or np.any(np.linalg.norm(r, axis=1) == 0.0):
            raise ValueError("Bloch vectors must be finite and non-zero")
        theta = np.arctan2(np.hypot(r[:, 0], r[:, 1]), r[:, 2])
        phi = np.arctan2(r[:, 1], r[:, 0])
        out = np.stack([np.cos(0.5 * theta).astype(np.complex128), np.exp(1j * phi) * np.sin(0.5 * theta)], axis=1)
    if not np.all(np.isfinite(out)) or np.any(np.abs(out).max(axis=1) == 0.0):
        raise ValueError("every spin needs a finite, non-zero amplitude pair")
    return out


def product_state_reference(amps: np.ndarray) -> np.ndarray:
    """The product ket of per-site amplitudes (n_sites, 2) in the reference's basis order (the
    Kronecker product over sites 0, 1, ...: site 0 = most significant bit)."""
    v = np.ones(1, dtype=np.complex128)
    for a in np.asarray(amps, dtype=np.complex128):
        v = np.kron(v, a)
    return v


_SAME_SPINS = ("n_sea", "is_center_rare", "is_spin_three_half", "gamma_sea", "gamma_rare", "dipolar_scale",
               "shell_scale")


def _check_segments(segments) -> list:
    segs = list(segments)
    if not segs:
        raise ValueError("segments must hold at least one DipolarRareParams")
    for k, p in enumerate(segs[1:], start=1):
        for name in _SAME_SPINS:
            if getattr(p, name) != getattr(segs[0], name):
                raise ValueError(f"segment {k} does not describe the same spins as segment 0: {name} differs")
    return segs


def _check_start(psi0, spins) -> None:
    if (psi0 is None) == (spins is None):
        raise ValueError("pass exactly one of psi0 and spins")


def _evolve_from(eng, params: DipolarRareParams, psi_eng, amps_by_site, refs_eng=None, ops_eng=None,
                 secs_eng=None):
    """One evolve of the unreduced register of ``params`` from an engine-order ket or a product
    state; returns (t, obs dict, final state in engine order, the Problem).  ``refs_eng``: reference
    states of the register in engine order, (K, 2^n), or "initial" (the state the evolve starts
    from, as the engine holds it); the overlap traces (K, n_t) are then returned as a fifth item.
    ``ops_eng``: operator strings of the register by bit, (K, n) codes; their traces (K, n_t) are then
    returned as the next item.  ``secs_eng``: sector sets of the register by bit, (K, 3) masks; their
    traces, a list of (B_k, n_t) arrays, are then returned as the last item.  The engine is left
    cleared, so without references, strings and sets."""
    t = time_grid(params)
    prob = build_problem(params, order="engine", reduce=False)
    eng.clear()
    try:
        pid = eng.add(prob)
        if psi_eng is not None:
            eng.set_initial_state(pid, psi_eng)
        else:
            eng.set_initial_product(pid, amps_by_site[prob.site_of_bit])
        if refs_eng is not None:
            eng.set_overlap_refs(pid, eng.initial_state(pid)[None, :] if isinstance(refs_eng, str) else refs_eng)
        if ops_eng is not None:
            eng.set_op_strings(pid, ops_eng)
        if secs_eng is not None:
            eng.set_sectors(pid, secs_eng)
        obs, _ = eng.evolve(t, tol=_tol())
        final = eng.state(pid)
        ovl = eng.overlap_traces(pid) if refs_eng is not None else None
        strs = eng.op_string_traces(pid) if ops_eng is not None else None
        secs = eng.sector_traces(pid) if secs_eng is not None else None
    finally:
        eng.clear()
    out = (t, {name: obs[0, j].copy() for j, name in enumerate(OBS_NAMES)}, final, prob)
    if refs_eng is not None:
        out = out + (ovl,)
    if ops_eng is not None:
        out = out + (strs,)
    return out if secs_eng is None else out + (secs,)


def simulate_rare_from(params: DipolarRareParams, psi0=None, spins=None, return_state: bool = False,
                       device: int | None = None):
    """simulate_rare from a general initial state: ``(t, obs)`` as simulate_rare returns them.

    Pass exactly one of ``psi0``, a dense ket of dimension 2^(n_sea + 1) in the reference's basis
    order (what initial_state_rare and build_hamiltonian_rare use: site 0 = most significant bit),
    and ``spins``, per-site amplitudes (n_sites, 2) on (up, down) or Bloch vectors (n_sites, 3)
    (spin_amplitudes); a product state is built on the device.  The state need not be normalised:
    ``obs["state_norm"]`` reports its norm, the expectations are of the normalised state.  The
    register is built unreduced (the frozen-rare reduction assumes the basis state).
    ``return_state=True``: ``(t, obs, psi_final)`` with the final state in the reference's order."""
    _check_start(psi0, spins)
    n_sites = params.n_sea + 1
    amps = spin_amplitudes(spins, n_sites) if spins is not None else None
    prob = build_problem(params, order="engine", reduce=False)
    psi_eng = reference_to_engine_state(psi0, prob.site_of_bit) if psi0 is not None else None
    eng = _engine(_default_device() if device is None else device)
    t, obs, final, prob = _evolve_from(eng, params, psi_eng, amps)
    if return_state:
        return t, obs, engine_to_reference_state(final, prob.site_of_bit)
    return t, obs


def simulate_rare_overlaps(params: DipolarRareParams, refs, psi0=None, spins=None, device: int | None = None):
    """simulate_rare_from that also returns the overlaps with reference states:
    ``(t, obs, overlaps)``, ``overlaps[k, j] = <refs[k]|psi(t_j)> / ||psi(t_j)||`` (complex128, with
    the phase of psi(t) = exp(-i H (t - t_0)) psi(t_0)).

    ``refs``: a ``(K, 2^(n_sea + 1))`` array of kets in the reference's basis order (used as given,
    not normalised; K <= 16), or the string ``"initial"``: K = 1, the initial state itself, i.e. the
    return amplitude <psi(t_0)|psi(t)> whose Fourier transform is the spectrum of the prepared
    state.  ``psi0`` / ``spins`` as in simulate_rare_from (at most one); with neither the evolution
    starts from ``initial_state_rare(params)``.  ``obs`` is what simulate_rare_from returns for the
    same start."""
    if psi0 is not None and spins is not None:
        raise ValueError("pass at most one of psi0 and spins")
    if psi0 is None and spins is None:
        psi0 = initial_state_rare(params)
    n_sites = params.n_sea + 1
    amps = spin_amplitudes(spins, n_sites) if spins is not None else None
    prob = build_problem(params, order="engine", reduce=False)
    psi_eng = reference_to_engine_state(psi0, prob.site_of_bit) if psi0 is not None else None
    if isinstance(refs, str):
        if refs != "initial":
            raise ValueError('refs must be an array of kets or the string "initial"')
        refs_eng = refs
    else:
        r = np.asarray(refs, dtype=np.complex128)
        if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] != 1 << n_sites:
            raise ValueError(f"refs must have shape (K, {1 << n_sites}) with K >= 1")
        refs_eng = np.stack([reference_to_engine_state(v, prob.site_of_bit) for v in r])
    eng = _engine(_default_device() if device is None else device)
    t, obs, _, _, ovl = _evolve_from(eng, params, psi_eng, amps, refs_eng)
    return t, obs, ovl


# The alphabet of an operator string, one letter per site: the codes of enum dse_site_op
# (include/dse.h): 1, Ix, Iy, Iz, I+, I-, Ea = |up><up|, Eb = |down><down|
OP_STRING_ALPHABET = "1xyz+-ab"
MAX_OP_STRINGS = 64  # DSE_MAX_OP_STRINGS


def op_strings_by_bit(strings, site_of_bit: np.ndarray) -> np.ndarray:
    """Operator strings over the alphabet ``"1xyz+-ab"``, one letter per site in the reference's site
    order (each of length n_sites = len(site_of_bit)), as the ``(K, n)`` uint8 code array by register
    bit that Engine.set_op_strings takes: ``out[s, b] = code(strings[s][site_of_bit[b]])``."""
    site_of_bit = np.asarray(site_of_bit, dtype=np.int64)
    n = site_of_bit.size
    if isinstance(strings, str):
        strings = [strings]
    strings = list(strings)
    if sorted(site_of_bit.tolist()) != list(range(n)):
        raise ValueError("site_of_bit must be a permutation of the sites")
    out = np.zeros((len(strings), n), dtype=np.uint8)
    for k, w in enumerate(strings):
        if not isinstance(w, str) or len(w) != n:
            raise ValueError(f"string {k} must be a str of {n} letters, one per site")
        codes = [OP_STRING_ALPHABET.find(ch) for ch in w]
        if min(codes) < 0:
            raise ValueError(f"string {k} holds a letter outside {OP_STRING_ALPHABET!r}")
        out[k] = np.asarray(codes, dtype=np.uint8)[site_of_bit]
    return out


def simulate_rare_strings(params: DipolarRareParams, strings, psi0=None, spins=None, device: int | None = None):
    """simulate_rare_from that also returns expectation values of operator strings:
    ``(t, obs, values)``, ``values[k, j] = <psi(t_j)| prod_s O_s |psi(t_j)> / <psi|psi>`` (complex128)
    for ``strings[k]``, a str of n_sea + 1 letters over ``"1xyz+-ab"`` in the reference's site order
    (1, Ix, Iy, Iz, I+, I-, |up><up|, |down><down|); K <= 64.  ``psi0`` / ``spins`` as in
    simulate_rare_from (at most one); with neither the evolution starts from
    ``initial_state_rare(params)``.  See rdm_strings / rdm_from_string_values for reduced density
    matrices."""
    if psi0 is not None and spins is not None:
        raise ValueError("pass at most one of psi0 and spins")
    n_sites = params.n_sea + 1
    if isinstance(strings, str):
        strings = [strings]
    strings = list(strings)
    if not 1 <= len(strings) <= MAX_OP_STRINGS:
        raise ValueError(f"pass 1..{MAX_OP_STRINGS} strings")
    prob = build_problem(params, order="engine", reduce=False)
    if len(prob.site_of_bit) != n_sites:
        raise ValueError("the unreduced register must hold every site")
    ops = op_strings_by_bit(strings, prob.site_of_bit)
    if psi0 is None and spins is None:
        psi0 = initial_state_rare(params)
    amps = spin_amplitudes(spins, n_sites) if spins is not None else None
    psi_eng = reference_to_engine_state(psi0, prob.site_of_bit) if psi0 is not None else None
    eng = _engine(_default_device() if device is None else device)
    t, obs, _, _, vals = _evolve_from(eng, params, psi_eng, amps, ops_eng=ops)
    return t, obs, vals


def rdm_strings(sites, n_sites: int) -> List[str]:
    """The 4^m - 1 strings over {1, x, y, z} on the m <= 3 distinct ``sites`` (identity elsewhere, the
    all-identity string left out) whose values determine the reduced density matrix of those sites.
    String c - 1, c = 1 .. 4^m - 1, carries the letter ``"1xyz"[d_i]`` on ``sites[i]``, d the base-4
    digits of c with ``sites[0]`` the most significant."""
    sites = [int(x) for x in sites]
    m = len(sites)
    if not 1 <= m <= 3 or len(set(sites)) != m or min(sites) < 0 or max(sites) >= n_sites:
        raise ValueError("sites: 1 to 3 distinct sites in 0..n_sites - 1")
    out = []
    for c in range(1, 4 ** m):
        w = ["1"] * n_sites
        for i, site in enumerate(sites):
            w[site] = "1xyz"[(c >> (2 * (m - 1 - i))) & 3]
        out.append("".join(w))
    return out


def rdm_from_string_values(values) -> np.ndarray:
    """``(n_t, 2^m, 2^m)`` reduced density matrices from the values ``(4^m - 1, n_t)`` (or
    ``(4^m - 1,)``: one time) of rdm_strings, rho = 2^-m sum_c <sigma_c> sigma_c with sigma = 2 I and
    <sigma_0> = 1.  Basis: ``sites[0]`` the most significant bit, 0 = up.  The values of Hermitian
    strings are real; their real parts are used, so rho is Hermitian with trace 1."""
    v = np.asarray(values)
    if v.ndim == 1:
        v = v[:, None]
    m = {3: 1, 15: 2, 63: 3}.get(v.shape[0]) if v.ndim == 2 else None
    if m is None:
        raise ValueError("values must have 4^m - 1 rows, m = 1, 2 or 3")
    sig = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]], dtype=np.complex128)
    dim = 1 << m
    rho = np.zeros((v.shape[1], dim, dim), dtype=np.complex128)
    rho += np.eye(dim) / dim
    for c in range(1, 4 ** m):
        digits = [(c >> (2 * (m - 1 - i))) & 3 for i in range(m)]
        mat = np.ones((1, 1), dtype=np.complex128)
        for d in digits:
            mat = np.kron(mat, sig[d])
        weight = sum(1 for d in digits if d)
        rho += (v[c - 1].real * (2.0 ** weight / dim))[:, None, None] * mat[None]
    return rho


# The alphabet of a sector set, one letter per site: w counted, . ignored, a / b selected up / down
SECTOR_ALPHABET = "w.ab"
MAX_SECTOR_SETS = 16  # DSE_MAX_SECTOR_SETS


def sector_masks_by_bit(sets, site_of_bit: np.ndarray) -> np.ndarray:
    """Sector sets over the alphabet ``"w.ab"``, one letter per site in the reference's site order
    (each of length n_sites = len(site_of_bit)): ``w`` a counted spin, ``.`` an ignored one, ``a`` /
    ``b`` a spin selected up / down.  Returns the ``(K, 3)`` uint64 masks by register bit (m, cm, cv)
    that Engine.set_sectors takes: bit b of a mask is set by the letter of site ``site_of_bit[b]``.
    1..16 sets."""
    site_of_bit = np.asarray(site_of_bit, dtype=np.int64)
    n = site_of_bit.size
    if isinstance(sets, str):
        sets = [sets]
    sets = list(sets)
    if sorted(site_of_bit.tolist()) != list(range(n)):
        raise ValueError("site_of_bit must be a permutation of the sites")
    if not 1 <= len(sets) <= MAX_SECTOR_SETS:
        raise ValueError(f"pass 1..{MAX_SECTOR_SETS} sets")
    out = np.zeros((len(sets), 3), dtype=np.uint64)
    for k, w in enumerate(sets):
        if not isinstance(w, str) or len(w) != n:
            raise ValueError(f"set {k} must be a str of {n} letters, one per site")
        if any(ch not in SECTOR_ALPHABET for ch in w):
            raise ValueError(f"set {k} holds a letter outside {SECTOR_ALPHABET!r}")
        m = cm = cv = 0
        for b in range(n):
            ch = w[site_of_bit[b]]
            m |= (ch == "w") << b
            cm |= (ch in "ab") << b
            cv |= (ch == "b") << b
        out[k] = (m, cm, cv)
    return out


def simulate_rare_sectors(params: DipolarRareParams, sets, psi0=None, spins=None, device: int | None = None):
    """simulate_rare_from that also returns magnetisation-sector populations: ``(t, obs,
    populations)``, ``populations[k]`` the ``(B_k, n_t)`` array of set ``sets[k]``, a str of n_sea + 1
    letters over ``"w.ab"`` in the reference's site order (counted, ignored, selected up, selected
    down); row j is the weight of the states with j counted spins down among those that meet the
    selection, over <psi|psi>; 1..16 sets.  ``psi0`` / ``spins`` as in simulate_rare_from (at most
    one); with neither the evolution starts from ``initial_state_rare(params)``.  The unreduced
    register is used and the cached engine is left without sets.  See mqc_intensities and
    sector_moments."""
    if psi0 is not None and spins is not None:
        raise ValueError("pass at most one of psi0 and spins")
    n_sites = params.n_sea + 1
    if isinstance(sets, str):
        sets = [sets]
    sets = list(sets)
    if not 1 <= len(sets) <= MAX_SECTOR_SETS:
        raise ValueError(f"pass 1..{MAX_SECTOR_SETS} sets")
    prob = build_problem(params, order="engine", reduce=False)
    if len(prob.site_of_bit) != n_sites:
        raise ValueError("the unreduced register must hold every site")
    masks = sector_masks_by_bit(sets, prob.site_of_bit)
    if psi0 is None and spins is None:
        psi0 = initial_state_rare(params)
    amps = spin_amplitudes(spins, n_sites) if spins is not None else None
    psi_eng = reference_to_engine_state(psi0, prob.site_of_bit) if psi0 is not None else None
    eng = _engine(_default_device() if device is None else device)
    out = _evolve_from(eng, params, psi_eng, amps, secs_eng=masks)
    return out[0], out[1], out[-1]


def mqc_intensities(P) -> np.ndarray:
    """Multiple-quantum-coherence intensities of a pure state from its sector populations: ``P`` of
    shape ``(n_t, B)`` (or ``(B,)``: one time), P[:, M] the population of the sector of M spins down,
    to ``(n_t, 2 B - 1)``: column q + B - 1 holds I_q = sum_M P_M P_{M - q} for q = -(B - 1) .. B - 1,
    the sum of |rho_xy|^2 over the pairs whose weights differ by q.  I_q = I_{-q}; for populations that
    sum to 1 so do the intensities."""
    p = np.asarray(P, dtype=np.float64)
    if p.ndim == 1:
        p = p[None, :]
    if p.ndim != 2 or p.shape[1] < 1:
        raise ValueError("P must have shape (n_t, B)")
    return np.stack([np.correlate(row, row, mode="full") for row in p])


def sector_moments(P, order: int) -> np.ndarray:
    """``(n_t, order + 1)`` moments of the number M of spins down under the populations ``P`` of shape
    ``(n_t, B)`` (or ``(B,)``): column 0 the total weight sum_M P_M, column 1 the mean of M, column
    r >= 2 the central moment <(M - <M>)^r>, means taken with P / sum_M P_M.  The polarisation of the
    counted spins is (B - 1) / 2 - <M>."""
    p = np.asarray(P, dtype=np.float64)
    if p.ndim == 1:
        p = p[None, :]
    order = int(order)
    if p.ndim != 2 or p.shape[1] < 1 or order < 1:
        raise ValueError("P must have shape (n_t, B) and order must be at least 1")
    M = np.arange(p.shape[1], dtype=np.float64)
    w = p.sum(axis=1)
    q = p / np.where(w > 0.0, w, 1.0)[:, None]
    mean = q @ M
    out = np.empty((p.shape[0], order + 1))
    out[:, 0], out[:, 1] = w, mean
    for r in range(2, order + 1):
        out[:, r] = np.sum(q * (M[None, :] - mean[:, None]) ** r, axis=1)
    return out


def rotation_matrices(vecs) -> np.ndarray:
    """(n_sites, 2, 2) matrices exp(-i theta n.sigma / 2) of the rotation vectors ``vecs``
    (n_sites, 3), row s = theta n of site s (the rotation of a hard pulse of flip angle theta about
    the axis n); a zero row is the identity.  Row / column 0 = spin up.  A rotation about z comes
    out exactly diagonal."""
    v = np.asarray(vecs)
    if v.ndim != 2 or v.shape[1] != 3 or np.iscomplexobj(v):
        raise ValueError("rotation vectors must be a real array of shape (n_sites, 3)")
    v = np.array(v, dtype=np.float64)
    if not np.all(np.isfinite(v)):
        raise ValueError("rotation vectors must be finite")
    theta = np.linalg.norm(v, axis=1)
    c = np.cos(0.5 * theta)
    # sin(theta / 2) n = (sin(theta / 2) / theta) v, 1/2 v at theta = 0
    s = v * np.where(theta > 0.0, np.sin(0.5 * theta) / np.where(theta > 0.0, theta, 1.0), 0.5)[:, None]
    u = np.empty((v.shape[0], 2, 2), dtype=np.complex128)
    u[:, 0, 0] = c - 1j * s[:, 2]
    u[:, 0, 1] = -s[:, 1] - 1j * s[:, 0]
    u[:, 1, 0] = s[:, 1] - 1j * s[:, 0]
    u[:, 1, 1] = c + 1j * s[:, 2]
    return u


def pulse_matrices_by_bit(mats_by_site: np.ndarray, site_of_bit: np.ndarray) -> np.ndarray:
    """Per-site pulse matrices (n_sites, 2, 2), sites in the reference's order, as the (n, 2, 2) array
    Engine.apply_pulse takes: row b = the matrix of the site register bit b holds."""
    sob = np.asarray(site_of_bit, dtype=np.int64)
    m = np.asarray(mats_by_site, dtype=np.complex128)
    if m.ndim != 3 or m.shape[1:] != (2, 2) or sorted(sob.tolist()) != list(range(m.shape[0])):
        raise ValueError("matrices must have shape (n_sites, 2, 2) and site_of_bit be a permutation of the sites")
    return np.ascontiguousarray(m[sob])


def _check_pulses(pulses, n_segments: int, n_sites: int) -> list:
    """One entry per segment: None or the (n_sites, 2, 2) matrices of the pulse before it."""
    if pulses is None:
        return [None] * n_segments
    entries = list(pulses)
    if len(entries) != n_segments:
        raise ValueError(f"pulses must have one entry per segment ({n_segments}), got {len(entries)}")
    out = []
    for k, e in enumerate(entries):
        if e is None:
            out.append(None)
            continue
        a = np.asarray(e)
        if a.shape == (n_sites, 3):
            out.append(rotation_matrices(a))
        elif a.shape == (n_sites, 2, 2):
            m = np.array(a, dtype=np.complex128)
            if not np.all(np.isfinite(m)):
                raise ValueError(f"pulse {k}: non-finite matrix entry")
            out.append(m)
        else:
            raise ValueError(f"pulse {k} must be None, rotation vectors ({n_sites}, 3) or matrices ({n_sites}, 2, 2)")
    return out


def simulate_rare_sequence(segments, psi0=None, spins=None, device: int | None = None, pulses=None):
    """A pulse sequence: piecewise-constant Hamiltonians, segment k starting from segment k - 1's
    final state, with an optional hard pulse before each segment.

    ``segments``: DipolarRareParams of the same spins (n_sea, geometry flags, gyromagnetic ratios
    and couplings equal, ValueError otherwise) that differ in drives, phases, detunings and their
    own (t_final, steps).  The start is ``psi0`` or ``spins`` as in simulate_rare_from.
    ``pulses``: None, or one entry per segment, applied to the state before that segment starts:
    None, rotation vectors (n_sites, 3) (rotation_matrices: theta n per site, a zero row leaves the
    spin alone) or matrices (n_sites, 2, 2) used as given; sites in the reference's order.  A wrong
    length or shape is a ValueError before a device is touched.  Returns
    ``([(t_0, obs_0), (t_1, obs_1), ...], psi_final)``: the times of segment k are offset by the
    preceding segments' t_final (a junction time appears in both neighbours), psi_final is in the
    reference's basis order.  The state stays on the device: the register is added once, and per
    segment its tables are replaced (Engine.set_hamiltonian), the pulse applied (Engine.apply_pulse),
    the segment evolved and its final state made the next start (Engine.continue_from_final).
    Every segment is in its own rotating frame (its omega_rf); the caller keeps them consistent."""
    segs = _check_segments(segments)
    _check_start(psi0, spins)
    n_sites = segs[0].n_sea + 1
    mats = _check_pulses(pulses, len(segs), n_sites)
    amps = spin_amplitudes(spins, n_sites) if spins is not None else None
    probs = [build_problem(p, order="engine", reduce=False) for p in segs]
    psi_eng = reference_to_engine_state(psi0, probs[0].site_of_bit) if psi0 is not None else None
    eng = _engine(_default_device() if device is None else device)
    out, t_off = [], 0.0
    eng.clear()
    try:
        pid = eng.add(probs[0])
        if psi_eng is not None:
            eng.set_initial_state(pid, psi_eng)
        else:
            eng.set_initial_product(pid, amps[probs[0].site_of_bit])
        for k, (p, prob) in enumerate(zip(segs, probs)):
            if k:
                eng.continue_from_final(pid)
                eng.set_hamiltonian(pid, prob)
            if mats[k] is not None:
                eng.apply_pulse(pid, pulse_matrices_by_bit(mats[k], prob.site_of_bit))
            t = time_grid(p)
            obs, _ = eng.evolve(t, tol=_tol())
            out.append((t + t_off, {name: obs[0, j].copy() for j, name in enumerate(OBS_NAMES)}))
            t_off += float(p.t_final)
        final = eng.state(pid)
    finally:
        eng.clear()
    return out, engine_to_reference_state(final, probs[-1].site_of_bit)
