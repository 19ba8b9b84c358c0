"""Python handle on one device's engine context (libdse.so).

``Engine`` owns a ``dse_ctx``: problems (coefficient tables from ``problem.py``)
are added, then evolved together on one MI355X with the exact Chebyshev
propagator.  Errors from the library surface as ``ValueError`` (bad arguments,
as the reference raises for a bad grid, dipolar_ensemble_with_rare.py:620-621)
or ``RuntimeError`` (HIP / allocation / degree-cap failures).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np

from . import _lib
from .problem import Problem

DEFAULT_TOL = 1e-14


def device_count() -> int:
    return int(_lib.lib().dse_device_count())


def device_memory(device: int) -> Tuple[float, float]:
    """(free, total) bytes of a device's memory (hipMemGetInfo)."""
    out = np.empty(2)
    rc = _lib.lib().dse_device_memory(int(device), _lib.ptr(out))
    if rc != 0:
        raise RuntimeError(f"dse_device_memory({device}) failed ({rc})")
    return float(out[0]), float(out[1])


def problem_bytes(prob: Problem, stored_initial_state: bool = False, overlap_refs: int = 0) -> float:
    """Upper estimate of one problem's device footprint in a context: 3 state buffers, one
    intermediate output of a two-output launch, the Walsh-Hadamard engine's 2 extra vectors or the
    2-tile hand-off ring (the larger: 2 vectors), plus tables and coefficients.
    ``stored_initial_state``: the problem will carry a stored initial state (Engine.set_initial_state
    or continue_from_final): one more state-sized buffer (a product state costs none).
    ``overlap_refs``: the reference states it will carry (Engine.set_overlap_refs): one state-sized
    buffer each."""
    return 16.0 * (3 + 1 + 2 + (1 if stored_initial_state else 0) + int(overlap_refs)) * (1 << prob.n_qubits) + (4 << 20)


# A libdse evolve runs its persistent interval kernel only when every register that is not on the
# small-register engine fits one or two 2^13-amplitude tiles (dse_runtime.hip, dse_evolve's mode
# choice); one larger register in the call drops all of them to the streaming kernels.
PERSISTENT_MAX_QUBITS = 14


def engine_class(prob: Problem) -> int:
    """0: a register the persistent kernel (or the small-register engine) takes, 1: a larger one."""
    return 0 if prob.n_qubits <= PERSISTENT_MAX_QUBITS else 1


def evolve_groups(grid_keys, probs) -> Dict[Tuple, list]:
    """Indices of problems that share one evolve call: the same time grid and the same engine
    class, so a mixed batch keeps its tile-sized registers on the persistent kernel."""
    groups: Dict[Tuple, list] = {}
    for i, (key, p) in enumerate(zip(grid_keys, probs)):
        groups.setdefault((*key, engine_class(p)), []).append(i)
    return groups


# Device memory a context holds besides its problems: observable partials (up to 256 MiB), the
# intermediate outputs and hand-off slots of the interval kernel beyond the per-problem estimate,
# flags, coefficient arenas.
CONTEXT_BYTES = 512 << 20


def batches_for_memory(probs, device: int, headroom: float = 0.8, stored_initial_state=None):
    """Index batches of ``probs`` whose summed footprint fits ``headroom`` of the free memory of
    ``device`` less one context's fixed arenas (at least one problem per batch; a problem too large
    alone still gets its own).  Call it with the context cleared, so its last batch's buffers are
    not counted as used.  ``stored_initial_state``: per problem, whether it will carry a stored
    initial state (problem_bytes); None: none does."""
    free, _ = device_memory(device)
    budget = headroom * free - CONTEXT_BYTES
    out, cur, used = [], [], 0.0
    for i, p in enumerate(probs):
        b = problem_bytes(p, bool(stored_initial_state[i]) if stored_initial_state is not None else False)
        if cur and used + b > budget:
            out.append(cur)
            cur, used = [], 0.0
        cur.append(i)
        used += b
    if cur:
        out.append(cur)
    return out


class Engine:
    def __init__(self, device: int = 0, tile_bits: int | None = None, time_kernels: bool = True):
        self._L = _lib.lib()
        h = self._L.dse_create(int(device))
        if not h:
            raise RuntimeError("dse_create failed: " + self._L.dse_create_error().decode())
        self._h = C.c_void_p(h)
        self.device = device
        self.problems: list[Problem] = []
        self._dims: list[int] = []       # state size the hooks of each problem id take
        self._sector_off: dict[int, np.ndarray] = {}  # problem id -> first unit of each sector set, then U
        if tile_bits is not None:
            self.set_option("tile_bits", tile_bits)
        self.set_option("time_kernels", 1.0 if time_kernels else 0.0)

    # -- plumbing --
    def _check(self, rc: int) -> int:
        if rc >= 0:
            return rc
        msg = self._L.dse_last_error(self._h).decode()
        if rc == _lib.DSE_ERR_ARG:
            raise ValueError(msg)
        raise RuntimeError(f"libdse error {rc}: {msg}")

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.dse_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, key: str, value: float) -> None:
        self._check(self._L.dse_set_option(self._h, key.encode(), float(value)))

    # -- problems --
    @staticmethod
    def _tables(prob: Problem):
        n = prob.n_qubits
        return (np.ascontiguousarray(prob.field, dtype=np.float64),
                np.ascontiguousarray(prob.zz, dtype=np.float64).reshape(n * n),
                np.ascontiguousarray(prob.pair, dtype=np.float64).reshape(n * n),
                np.ascontiguousarray(prob.flip, dtype=np.float64).reshape(4 * n))

    def add(self, prob: Problem) -> int:
        tabs = self._tables(prob)
        pid = self._check(self._L.dse_add_problem(
            self._h, prob.n_qubits, *[_lib.ptr(a) for a in tabs],
            float(prob.shift), int(prob.psi0_index), int(prob.sea_mask), int(prob.rare_bit),
            float(prob.rare_z_const)))
        self.problems.append(prob)
        self._dims.append(1 << prob.n_qubits)
        return pid

    def add_sharded(self, prob: Problem, shard_bits: int, rank: int = -1) -> int:
        """A register partitioned by its top ``shard_bits`` qubits (include/dse.h): all shards
        on this device (rank -1, returns shard 0's id; its hooks take whole-register states) or
        this process's shard ``rank`` of a register spread over processes (after dist_init)."""
        tabs = self._tables(prob)
        pid = self._check(self._L.dse_add_problem_sharded(
            self._h, prob.n_qubits, *[_lib.ptr(a) for a in tabs],
            float(prob.shift), int(prob.psi0_index), int(prob.sea_mask), int(prob.rare_bit),
            float(prob.rare_z_const), int(shard_bits), int(rank)))
        n_members = 1 if rank >= 0 else (1 << shard_bits)
        for i in range(n_members):
            self.problems.append(prob)
            self._dims.append((1 << prob.n_qubits) if (rank < 0 and i == 0)
                              else int(self._L.dse_problem_dim(self._h, pid + i)))
        return pid

    @staticmethod
    def dist_unique_id() -> bytes:
        buf = C.create_string_buffer(_lib.DSE_DIST_ID_BYTES)
        if _lib.lib().dse_dist_unique_id(buf) != 0:
            raise RuntimeError("dse_dist_unique_id (ncclGetUniqueId) failed")
        return buf.raw

    def dist_init(self, rank: int, world: int, uid: bytes) -> None:
        """Join the RCCL communicator of a register partitioned over ``world`` processes."""
        if len(uid) != _lib.DSE_DIST_ID_BYTES:
            raise ValueError("unique id must have DSE_DIST_ID_BYTES bytes")
        self._check(self._L.dse_dist_init(self._h, int(rank), int(world), uid))

    def dist_init_exchange(self, rank: int, world: int, dist) -> None:
        """Join a partitioned register's ranks over ``dist`` (an initialised torch.distributed,
        e.g. gloo) instead of RCCL: libdse hands every exchange to this host callback
        (include/dse.h dse_dist_init_exchange)."""
        import torch

        def view(addr, nbytes, dtype):
            buf = (C.c_uint8 * nbytes).from_address(addr)
            return torch.from_numpy(np.frombuffer(buf, dtype=dtype))

        def fn(_user, op, send, recv, nbytes, peer):
            try:
                if op == _lib.DSE_XCHG_ALLTOALL:
                    dist.all_to_all_single(view(recv, nbytes * world, np.uint8),
                                           view(send, nbytes * world, np.uint8))
                elif op == _lib.DSE_XCHG_SENDRECV:
                    reqs = [dist.isend(view(send, nbytes, np.uint8), peer),
                            dist.irecv(view(recv, nbytes, np.uint8), peer)]
                    for r in reqs:
                        r.wait()
                elif op == _lib.DSE_XCHG_ALLREDUCE_F64:
                    dist.all_reduce(view(send, nbytes, np.float64))
                else:
                    return 1
                return 0
            except Exception:  # reported to the library as a failed exchange
                return 1

        self._xfn = _lib.EXCHANGE_FN(fn)   # kept alive with the engine
        self._check(self._L.dse_dist_init_exchange(self._h, int(rank), int(world), self._xfn, None))

    def clear(self) -> None:
        self._check(self._L.dse_clear(self._h))
        self.problems = []
        self._dims = []
        self._sector_off = {}

    # -- hot path --
    def apply_h(self, pid: int, psi: np.ndarray) -> np.ndarray:
        dim = self._dims[pid]
        x = np.ascontiguousarray(psi, dtype=np.complex128)
        if x.shape != (dim,):
            raise ValueError(f"state must have shape ({dim},)")
        out = np.empty_like(x)
        self._check(self._L.dse_apply_h(self._h, pid, _lib.ptr(x), _lib.ptr(out)))
        return out

    def observables(self, pid: int, psi: np.ndarray) -> np.ndarray:
        dim = self._dims[pid]
        x = np.ascontiguousarray(psi, dtype=np.complex128)
        if x.shape != (dim,):
            raise ValueError(f"state must have shape ({dim},)")
        out = np.empty(7)
        self._check(self._L.dse_observables(self._h, pid, _lib.ptr(x), _lib.ptr(out)))
        return out

    def evolve(self, t: np.ndarray, tol: float = DEFAULT_TOL) -> Tuple[np.ndarray, Dict[str, float]]:
        """obs[problem, 7, n_t] for all problems, and the call's counters."""
        tt = np.ascontiguousarray(t, dtype=np.float64)
        out = np.empty((len(self.problems), _lib.DSE_N_OBS, len(tt)))
        st = _lib.DseStats()
        self._check(self._L.dse_evolve(self._h, _lib.ptr(tt), len(tt), float(tol), _lib.ptr(out),
                                       C.byref(st)))
        stats = st.as_dict()
        # (a counter added after dse_stats was closed: a getter, include/dse.h at DSE_ABI_MINOR)
        stats["leap_problems"] = int(self._L.dse_leap_problems(self._h))
        return out, stats

    def site_observables(self, pid: int, psi: np.ndarray) -> np.ndarray:
        """(3, n): <Ix_b>, <Iy_b>, <Iz_b> of every register bit b of the normalised state ``psi``
        (dse_site_observables: the kernel of the option "site_obs", whatever its value)."""
        dim = self._dims[pid]
        x = np.ascontiguousarray(psi, dtype=np.complex128)
        if x.shape != (dim,):
            raise ValueError(f"state must have shape ({dim},)")
        out = np.empty((3, self.problems[pid].n_qubits))
        self._check(self._L.dse_site_observables(self._h, pid, _lib.ptr(x), _lib.ptr(out)))
        return out

    def site_traces(self, pid: int) -> np.ndarray:
        """(3, n, n_t): the site-resolved traces of register ``pid`` from the last evolve, which
        must have run with the option "site_obs" = 1 (RuntimeError otherwise)."""
        if not 0 <= pid < len(self.problems):
            raise ValueError("bad problem id")
        # sized from what the library holds (0: none; the call below then raises and writes nothing)
        n_t = max(int(self._L.dse_site_obs_outputs(self._h)), 0)
        out = np.empty((3, self.problems[pid].n_qubits, max(n_t, 1)))
        self._check(self._L.dse_get_site_obs(self._h, pid, _lib.ptr(out)))
        return out

    def pair_observables(self, pid: int, psi: np.ndarray) -> np.ndarray:
        """(5, NP): ZZ, Re ZQ, Im ZQ, Re DQ, Im DQ of every pair of register bits i < j (at
        ``problem.pair_index(i, j)``) of the normalised state ``psi`` (dse_pair_observables: the
        kernel of the option "pair_obs", whatever its value)."""
        dim = self._dims[pid]
        x = np.ascontiguousarray(psi, dtype=np.complex128)
        if x.shape != (dim,):
            raise ValueError(f"state must have shape ({dim},)")
        n = self.problems[pid].n_qubits
        out = np.empty((5, n * (n - 1) // 2))
        self._check(self._L.dse_pair_observables(self._h, pid, _lib.ptr(x), _lib.ptr(out)))
        return out

    def pair_traces(self, pid: int) -> np.ndarray:
        """(5, NP, n_t): the two-spin correlators of register ``pid`` from the last evolve, which
        must have run with the option "pair_obs" = 1 (RuntimeError otherwise)."""
        if not 0 <= pid < len(self.problems):
            raise ValueError("bad problem id")
        n_t = max(int(self._L.dse_pair_obs_outputs(self._h)), 0)
        n = self.problems[pid].n_qubits
        out = np.empty((5, n * (n - 1) // 2, max(n_t, 1)))
        self._check(self._L.dse_get_pair_obs(self._h, pid, _lib.ptr(out)))
        return out

    def pair_obs_problems(self) -> int:
        """Registers whose pair sums the last successful evolve produced."""
        return int(self._L.dse_pair_obs_problems(self._h))

    # -- overlaps with stored reference states (include/dse.h, feature "overlap_obs") --
    def set_overlap_refs(self, pid: int, refs) -> None:
        """Register ``pid`` carries the reference states ``refs`` ((K, 2^n) complex, K <=
        DSE_MAX_OVERLAP_REFS, used as given; a loopback partitioned register: shard 0's id and whole
        states): every later evolve keeps <refs[k]|psi(t_j)> / ||psi(t_j)|| of every output.  The set
        replaces the previous one; ``None`` or an empty array clears it."""
        pid = self._pid(pid)
        if refs is None or len(refs) == 0:
            self._check(self._L.dse_set_overlap_refs(self._h, pid, 0, None))
            return
        dim = self._dims[pid]
        x = np.ascontiguousarray(refs, dtype=np.complex128)
        if x.ndim == 1:
            x = x[None, :]
        if x.ndim != 2 or x.shape[1] != dim:
            raise ValueError(f"references must have shape (K, {dim})")
        self._check(self._L.dse_set_overlap_refs(self._h, pid, x.shape[0], _lib.ptr(x)))

    def overlap_refs(self, pid: int) -> int:
        """K of register ``pid`` (0: none)."""
        return self._check(self._L.dse_overlap_refs(self._h, self._pid(pid)))

    def overlaps(self, pid: int, psi: np.ndarray) -> np.ndarray:
        """(K,) complex: <refs[k]|psi> / ||psi|| of the given state (dse_overlaps: the tile kernel of
        the evolve).  RuntimeError for a register without references."""
        pid = self._pid(pid)
        dim = self._dims[pid]
        x = np.ascontiguousarray(psi, dtype=np.complex128)
        if x.shape != (dim,):
            raise ValueError(f"state must have shape ({dim},)")
        out = np.empty((2, max(self.overlap_refs(pid), 1)))
        self._check(self._L.dse_overlaps(self._h, pid, _lib.ptr(x), _lib.ptr(out)))
        return out[0] + 1j * out[1]

    def overlap_traces(self, pid: int) -> np.ndarray:
        """(K, n_t) complex128: <refs[k]|psi(t_j)> / ||psi(t_j)|| of register ``pid`` from the last
        evolve (RuntimeError before one, after a failed one and for a register without references)."""
        pid = self._pid(pid)
        n_t = max(int(self._L.dse_overlap_outputs(self._h)), 0)
        out = np.empty((2, max(self.overlap_refs(pid), 1), max(n_t, 1)))
        self._check(self._L.dse_get_overlaps(self._h, pid, _lib.ptr(out)))
        return out[0] + 1j * out[1]

    def overlap_problems(self) -> int:
        """Registers whose overlaps the last successful evolve produced."""
        return int(self._L.dse_overlap_problems(self._h))

    # -- expectation values of operator strings (include/dse.h, feature "op_strings") --
    def set_op_strings(self, pid: int, ops) -> None:
        """Register ``pid`` carries the operator strings ``ops``: a ``(K, n)`` uint8 array,
        ``ops[s, b]`` the code of register bit b in string s (0..7: 1, Ix, Iy, Iz, I+, I-, Ea, Eb;
        K <= DSE_MAX_OP_STRINGS; a loopback partitioned register: shard 0's id and all n bits).  Every
        later evolve keeps <psi(t_j)| prod_b O_b |psi(t_j)> / <psi|psi> of every output.  The set
        replaces the previous one; ``None`` or an empty array clears it."""
        pid = self._pid(pid)
        if ops is None or len(ops) == 0:
            self._check(self._L.dse_set_op_strings(self._h, pid, 0, None))
            return
        n = self.problems[pid].n_qubits
        x = np.asarray(ops)
        if x.ndim == 1:
            x = x[None, :]
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"operator strings must have shape (K, {n})")
        if not np.issubdtype(x.dtype, np.integer) or x.min() < 0 or x.max() > 255:
            raise ValueError("operator codes must be integers in 0..7")
        x = np.ascontiguousarray(x, dtype=np.uint8)
        self._check(self._L.dse_set_op_strings(self._h, pid, x.shape[0], _lib.u8ptr(x)))

    def op_strings(self, pid: int) -> int:
        """K of register ``pid`` (0: none)."""
        return self._check(self._L.dse_op_strings(self._h, self._pid(pid)))

    def op_string_values(self, pid: int, psi: np.ndarray) -> np.ndarray:
        """(K,) complex: the values of the register's strings on the given state
        (dse_op_string_values: the tile kernel of the evolve).  RuntimeError for a register without
        strings."""
        pid = self._pid(pid)
        dim = self._dims[pid]
        x = np.ascontiguousarray(psi, dtype=np.complex128)
        if x.shape != (dim,):
            raise ValueError(f"state must have shape ({dim},)")
        out = np.empty((2, max(self.op_strings(pid), 1)))
        self._check(self._L.dse_op_string_values(self._h, pid, _lib.ptr(x), _lib.ptr(out)))
        return out[0] + 1j * out[1]

    def op_string_traces(self, pid: int) -> np.ndarray:
        """(K, n_t) complex128: the values of the register's strings at every output of the last
        evolve (RuntimeError before one, after a failed one and for a register without strings)."""
        pid = self._pid(pid)
        n_t = max(int(self._L.dse_op_string_outputs(self._h)), 0)
        out = np.empty((2, max(self.op_strings(pid), 1), max(n_t, 1)))
        self._check(self._L.dse_get_op_strings(self._h, pid, _lib.ptr(out)))
        return out[0] + 1j * out[1]

    def op_string_problems(self) -> int:
        """Registers whose string values the last successful evolve produced."""
        return int(self._L.dse_op_string_problems(self._h))

    # -- magnetisation-sector populations (include/dse.h, feature "sector_obs") --
    def set_sectors(self, pid: int, masks) -> None:
        """Register ``pid`` carries the sector sets ``masks``: a ``(K, 3)`` array of register-bit masks,
        row k = (m, cm, cv): the counted bits, the selecting bits and their values (K <=
        DSE_MAX_SECTOR_SETS; m & cm == 0, cv within cm; a loopback partitioned register: shard 0's id
        and masks over all n bits).  Every later evolve keeps, for every output, the populations
        P_j = sum |psi_x|^2 / <psi|psi> over the x with (x & cm) == cv and popcount(x & m) == j,
        j = 0 .. popcount(m).  The sets replace the previous ones; ``None`` or an empty array clears
        them."""
        pid = self._pid(pid)
        if masks is None or len(masks) == 0:
            self._check(self._L.dse_set_sectors(self._h, pid, 0, None))
            self._sector_off.pop(pid, None)
            return
        x = _lib.sector_masks(masks)
        self._check(self._L.dse_set_sectors(self._h, pid, x.shape[0], _lib.u64ptr(x)))
        self._sector_off[pid] = _lib.sector_layout(self.problems[pid].n_qubits, x)[1]

    def sectors(self, pid: int) -> int:
        """K of register ``pid`` (0: none)."""
        return self._check(self._L.dse_sectors(self._h, self._pid(pid)))

    def sector_units(self, pid: int) -> int:
        """U = sum_k (popcount(m_k) + 1) of register ``pid`` (0: none)."""
        return self._check(self._L.dse_sector_units(self._h, self._pid(pid)))

    def _split_sectors(self, pid: int, flat: np.ndarray):
        off = self._sector_off[pid]
        return [flat[off[k]:off[k + 1]].copy() for k in range(len(off) - 1)]

    def sector_values(self, pid: int, psi: np.ndarray):
        """A list of K arrays, entry k the ``(B_k,)`` populations of set k on the given state
        (dse_sector_values: the tile kernel of the evolve).  RuntimeError for a register without
        sets."""
        pid = self._pid(pid)
        dim = self._dims[pid]
        x = np.ascontiguousarray(psi, dtype=np.complex128)
        if x.shape != (dim,):
            raise ValueError(f"state must have shape ({dim},)")
        out = np.empty(max(self.sector_units(pid), 1))
        self._check(self._L.dse_sector_values(self._h, pid, _lib.ptr(x), _lib.ptr(out)))
        return self._split_sectors(pid, out)

    def sector_traces(self, pid: int):
        """A list of K arrays, entry k the ``(B_k, n_t)`` populations of set k at every output of the
        last evolve, row j the sector of j counted spins down (RuntimeError before an evolve, after a
        failed one and for a register without sets)."""
        pid = self._pid(pid)
        n_t = max(int(self._L.dse_sector_outputs(self._h)), 0)
        out = np.empty((max(self.sector_units(pid), 1), max(n_t, 1)))
        self._check(self._L.dse_get_sectors(self._h, pid, _lib.ptr(out)))
        return self._split_sectors(pid, out)

    def sector_problems(self) -> int:
        """Registers whose sector populations the last successful evolve produced."""
        return int(self._L.dse_sector_problems(self._h))

    def state(self, pid: int) -> np.ndarray:
        out = np.empty(self._dims[pid], dtype=np.complex128)
        self._check(self._L.dse_get_state(self._h, pid, _lib.ptr(out)))
        return out

    # -- initial states other than the basis state (include/dse.h, ABI 14.1) --
    def _pid(self, pid: int) -> int:
        if not 0 <= int(pid) < len(self.problems):
            raise ValueError("bad problem id")
        return int(pid)

    def set_initial_state(self, pid: int, psi) -> None:
        """Later evolves of register ``pid`` start from ``psi`` (2^n complex, any non-zero norm;
        a loopback partitioned register: shard 0's id and the whole state) at t[0].  ``None``: back
        to the basis state ``psi0_index``."""
        pid = self._pid(pid)
        if psi is None:
            self._check(self._L.dse_set_initial_state(self._h, pid, None))
            return
        dim = self._dims[pid]
        x = np.ascontiguousarray(psi, dtype=np.complex128)
        if x.shape != (dim,):
            raise ValueError(f"state must have shape ({dim},)")
        self._check(self._L.dse_set_initial_state(self._h, pid, _lib.ptr(x)))

    def set_initial_product(self, pid: int, amps) -> None:
        """Later evolves of register ``pid`` start from the product state psi(x) = prod_b
        amps[b, bit_b(x)] (``amps``: (n, 2) complex, column 0 = bit value 0 = spin up), built on the
        device."""
        pid = self._pid(pid)
        n = self.problems[pid].n_qubits
        a = np.ascontiguousarray(amps, dtype=np.complex128)
        if a.shape != (n, 2):
            raise ValueError(f"amplitudes must have shape ({n}, 2)")
        self._check(self._L.dse_set_initial_product(self._h, pid, _lib.ptr(a)))

    def continue_from_final(self, pid: int) -> None:
        """The final state of the last evolve becomes register ``pid``'s initial state (on the
        device).  RuntimeError without a successful evolve before."""
        self._check(self._L.dse_continue_from_final(self._h, self._pid(pid)))

    def initial_state(self, pid: int) -> np.ndarray:
        """The state the next evolve of register ``pid`` would start from."""
        pid = self._pid(pid)
        out = np.empty(self._dims[pid], dtype=np.complex128)
        self._check(self._L.dse_get_initial_state(self._h, pid, _lib.ptr(out)))
        return out

    # -- hard pulses and a new H for a problem (include/dse.h, features "pulse", "set_hamiltonian") --
    def apply_pulse(self, pid: int, mats) -> None:
        """The state the next evolve of register ``pid`` starts from becomes U psi, U the tensor
        product of ``mats[b]`` over the register bits b (``mats``: (n, 2, 2) complex, row / column
        index = bit value, 0 = spin up; used as given, unitary or not).  A stored state is
        transformed in place on the device, a product state stays one, the basis state becomes a
        product state (dse_apply_pulse).  ``rotation_matrices`` makes ``mats`` from rotation vectors."""
        pid = self._pid(pid)
        n = self.problems[pid].n_qubits
        u = np.ascontiguousarray(mats, dtype=np.complex128)
        if u.shape != (n, 2, 2):
            raise ValueError(f"matrices must have shape ({n}, 2, 2)")
        self._check(self._L.dse_apply_pulse(self._h, pid, _lib.ptr(u)))

    def pulse_stats(self) -> Dict[str, float]:
        """Passes (kernel launches), their HIP-event time in ms and the bytes they moved, of the last
        apply_pulse (zeros when it ran on the host: product and basis starts, the identity)."""
        out = np.zeros(3)
        self._check(self._L.dse_pulse_stats(self._h, _lib.ptr(out)))
        return {"passes": int(out[0]), "ms": float(out[1]), "bytes": float(out[2])}

    def set_hamiltonian(self, pid: int, prob: Problem) -> None:
        """Register ``pid`` gets the tables of ``prob`` (the same number of qubits); it keeps its
        initial state, overlap references, operator strings, sector sets, masks and shard layout.  The final state of the last evolve
        is dropped: call continue_from_final first (dse_set_hamiltonian)."""
        pid = self._pid(pid)
        if prob.n_qubits != self.problems[pid].n_qubits:
            raise ValueError("the new tables must describe a register of the same size")
        tabs = self._tables(prob)
        self._check(self._L.dse_set_hamiltonian(self._h, pid, *[_lib.ptr(a) for a in tabs], float(prob.shift)))
        old, i = self.problems[pid], pid
        while i < len(self.problems) and self.problems[i] is old:  # the shards of a loopback register follow
            self.problems[i] = prob
            i += 1

    def energy(self, pid: int) -> Tuple[float, float]:
        """(<psi|H|psi> / <psi|psi>, <psi|psi>) of the final state after evolve, on the device."""
        out = np.empty(2)
        self._check(self._L.dse_energy(self._h, pid, _lib.ptr(out)))
        return float(out[0]), float(out[1])

    def time_step_kernel(self, reps: int = 20) -> Tuple[float, float]:
        ms = C.c_double()
        by = C.c_double()
        self._check(self._L.dse_time_step_kernel(self._h, int(reps), C.byref(ms), C.byref(by)))
        return ms.value, by.value


def spectral_bounds_native(prob: Problem) -> Tuple[float, float]:
    """dse_spectral_bounds (host-only library function)."""
    L = _lib.lib()
    n = prob.n_qubits
    arrs = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (prob.field, prob.zz, prob.pair, prob.flip)]
    lo, hi = C.c_double(), C.c_double()
    rc = L.dse_spectral_bounds(n, *[_lib.ptr(a) for a in arrs], float(prob.shift), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise ValueError("dse_spectral_bounds failed")
    return lo.value, hi.value


def bessel_native(z: float, kmax: int, tol: float = 1e-14) -> Tuple[np.ndarray, int]:
    """dse_bessel_j (host-only library function): J_0..J_kmax(z) and the truncation degree."""
    L = _lib.lib()
    out = np.empty(kmax + 1)
    deg = C.c_int()
    rc = L.dse_bessel_j(float(z), int(kmax), _lib.ptr(out), float(tol), C.byref(deg))
    if rc != 0:
        raise ValueError("dse_bessel_j failed")
    return out, deg.value
