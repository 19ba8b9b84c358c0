"""dse_set_option (csrc/dse_runtime.hip: the option table kOptions and the few keys spelled out beside
it): every key's accepted boundary and interior values, and for every checked key the nearest
rejected values -- below and above a range, a non-member of a set, a fraction where whole numbers
are required, NaN -- with the exact message.  The messages and ranges are written out here
literally, so the table cannot drift from them unnoticed.

The module opens a context of its own (no later test sees its options), evolves nothing, launches
no kernel, and closes the context at the end.  No option can be read back without an evolve
(dse_stats is the only way out), so tile_bits and streams are set and not read back.
"""
import pytest

pytestmark = pytest.mark.gpu

NAN = float("nan")
TWO30 = float(1 << 30)

# keys stored as value != 0.0: any value is accepted, NaN too (true)
BOOLEAN = ["persistent", "swap_overlap", "wht", "small", "dense_refine", "symv_fused", "handoff_fences",
           "xcd_pairs", "span_partial", "mixed_launch", "obs_overlap"]

# keys stored as (int)value (probe_items: (int64_t)value) without a check
UNCHECKED = {"wht_persist": [0, 2, 2.7, -1], "dbg": [7, 1.5, 0], "probe_items": [100, 2.5, 0]}

# key: (accepted values, rejected values, message).  A key whose range is not one of whole numbers only
# also takes a fraction inside it (stored as (int)value), and that is pinned here with one such
# value first in its accepted list; the keys without one (sets, wht_mid_inpage, wht_half) refuse 0.5
# or 2.5 in their rejected list.
CHECKED = {
    "tile_bits": ([1.5, 1, 7, 13], [0, 14, NAN], "tile_bits must be in 1..13"),
    "streams": ([1.5, 1, 8, 16, 4], [0, 17, NAN], "streams must be in 1..16"),
    "site_obs": ([1, 0], [-1, 2, 0.5, NAN], "site_obs must be 0 or 1"),
    "pair_obs": ([1, 0], [-1, 2, 0.5, NAN], "pair_obs must be 0 or 1"),
    "wht_contiguous": ([1, 0], [-1, 2, 0.5, NAN], "wht_contiguous must be 0 or 1"),
    "wht_fuse": ([0, 1], [-1, 2, 0.5, NAN], "wht_fuse must be 0 or 1"),
    "wht_mid_inpage": ([8, 4, 0], [-1, 9, 2.5, NAN], "wht_mid_inpage must be 0..8"),
    "wht_half": ([0, 3, 7], [-1, 8, 2.5, NAN], "wht_half must be 0..7"),
    "wht_tile_bits": ([12, 13, 0], [-1, 1, 11, 12.5, 14, NAN], "wht_tile_bits must be 0, 12 or 13"),
    "wht_group_bits": ([2.5, 2, 6, 11, 0], [-1, 1, 12, NAN], "wht_group_bits must be 0 or in 2..11"),
    "outputs_per_launch": ([1.5, 1, 2], [0, 3, NAN], "outputs_per_launch must be in 1..2"),
    "span_outputs": ([1.5, 1, 2, 4], [0, 5, NAN], "span_outputs must be in 1..4"),
    "coresident": ([2.5, 2, 100, 4096, 0], [-1, 1, 4097, NAN], "coresident must be 0 or in 2..4096"),
    "matrix": ([0, 2, 1], [-1, 3, 0.5, NAN], "matrix must be 0, 1 or 2"),
    "eig_streams": ([1.5, 1, 8, 3], [0, 9, NAN], "eig_streams must be in 1..8"),
    "eig_impl": ([0.5, 0, 2, 3, 1], [-1, 4, NAN], "eig_impl must be 0, 1, 2 or 3"),
    "eig_spin_limit": ([0.5, -1, 1000, TWO30, 1 << 16], [-2, TWO30 + 1, NAN], "eig_spin_limit must be in -1..2^30"),
    "dense_nufft": ([0, 2, 1], [-1, 3, 0.5, NAN], "dense_nufft must be 0, 1 or 2"),
    "dense": ([0, 2, 1], [-1, 3, 0.5, NAN], "dense must be 0, 1 or 2"),
    "small_chunk": ([1.5, 1, 1e6, 64], [0, 1e6 + 1, NAN], "small_chunk must be in 1..1e6"),
    "spin_limit": ([0.5, -1, 1000, TWO30, 1 << 22], [-2, TWO30 + 1, NAN], "spin_limit must be in -1..2^30"),
    "span": ([0.5, 2, 4, 0], [-1, 5, NAN], "span must be in 0..4"),
    "real": ([1, 2, 0], [-1, 3, 0.5, NAN], "real must be 0, 1 or 2"),
    "span_tile": ([10.5, 0, 10, 12, 13, -1], [-2, 1, 9, 14, NAN], "span_tile must be -1, 0 or in 10..13"),
    "span_rb": ([0.5, 2, 3, 0], [-1, 4, NAN], "span_rb must be in 0..3"),
    "span_chunks": ([0, 1, 2], [-1, 3, 0.5, NAN], "span_chunks must be 0, 1 or 2"),
    "span_partial_tile": ([10, 11], [9, 12, 10.5, NAN], "span_partial_tile must be 10 or 11"),
    "time_kernels": ([0.5, 0, 5, 1], [-1, NAN], "time_kernels must be >= 0"),
    "max_degree": ([1.5, 1, 1e9, 2e6], [0, NAN], "max_degree must be >= 1"),
}


@pytest.fixture(scope="module")
def own_engine():
    from quantumsimulations_amd.engine import Engine
    eng = Engine(0)
    yield eng
    eng.close()


def test_every_option_accepts_its_boundary_and_interior_values(own_engine):
    for key in BOOLEAN:
        for v in (0, 1, -3.5, NAN, 1):
            own_engine.set_option(key, v)
    for key, values in UNCHECKED.items():
        for v in values:
            own_engine.set_option(key, v)
    for key, (accepted, _, _) in CHECKED.items():
        for v in accepted:
            own_engine.set_option(key, v)


def test_every_checked_option_rejects_the_nearest_values_with_its_message(own_engine):
    wrong = []
    for key, (accepted, rejected, message) in CHECKED.items():
        for v in rejected:
            try:
                own_engine.set_option(key, v)
                wrong.append((key, v, "accepted"))
            except ValueError as e:
                if str(e) != message:
                    wrong.append((key, v, str(e)))
        own_engine.set_option(key, accepted[-1])  # after a refusal the key still takes a good value
    assert not wrong, wrong


def test_unknown_option(own_engine):
    with pytest.raises(ValueError) as e:
        own_engine.set_option("nope", 1.0)
    assert str(e.value) == "unknown option nope"


@pytest.mark.parametrize("key", ["ablate", "real_ablate", "span_ablate"])
def test_ablation_masks_need_a_diagnostics_build(own_engine, key):
    try:
        own_engine.set_option(key, 0)  # a diagnostics build takes the empty mask
    except ValueError as e:
        assert str(e) == f"option {key} needs a diagnostics build of libdse (-DDSE_DIAG)"

