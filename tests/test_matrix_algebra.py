"""The thread-pair slot arithmetic of the propagator-matrix column build (csrc/dse_matrix.hip, k_ucols),
enumerated on the CPU.

k_ucols<L> has TB = L - 4 thread bits and a list of ntt pairs of two thread bits (build_tables drops the
zero couplings, so ntt is anything in 0 .. C(TB, 2)).  Its fused loop visits thread bit j = 0 .. TB - 1
and takes, with NPI = ceil(C(TB, 2) / TB) and

    ja = min(TB, max(0, ntt - TB (NPI - 1))),

NPI pairs for j < ja and NPI - 1 pairs for the others, out of a table of TB * NPI slots in LDS:
slot (j, q) holds list index j NPI - max(0, j - ja) + q when q is below the iteration's count and the
index is below ntt, and a zero pair otherwise.  Pinned here, for TB = 6 .. 9 (L = 10 .. 13) and every
ntt: each list index sits in exactly one executed slot, no executed slot holds an index >= ntt, and
from ntt = TB (NPI - 1) up no executed slot is a padded one.  tests/test_gpu_matrix_cases.py chooses
its ntt values (ja = 0, 1, TB and the mixed ones) by these helpers.
"""
import pytest

TBS = (6, 7, 8, 9)


def n_pairs(tb):
    return tb * (tb - 1) // 2


def npi_of(tb):
    """thread pairs per fused iteration (UcGeo<L>::NPI)"""
    return (n_pairs(tb) + tb - 1) // tb


def ja_of(tb, ntt):
    return min(tb, max(0, ntt - tb * (npi_of(tb) - 1)))


def slot_table(tb, ntt, back=lambda j, ja: max(0, j - ja)):
    """S.tt as k_ucols fills it: {(j, q): list index or None (a zero pair)} for all TB * NPI slots."""
    npi, ja = npi_of(tb), ja_of(tb, ntt)
    tt = {}
    for p in range(tb * npi):
        j, q = divmod(p, npi)
        nj = npi if j < ja else npi - 1
        idx = j * npi - back(j, ja) + q
        tt[j, q] = idx if (q < nj and idx < ntt) else None
    return tt


def executed(tb, ntt):
    """the slots the fused loop reads: NPI of iteration j < ja, NPI - 1 of the others"""
    npi, ja = npi_of(tb), ja_of(tb, ntt)
    return [(j, q) for j in range(tb) for q in range(npi if j < ja else npi - 1)]


def test_geometry_of_the_four_instances():
    assert [npi_of(tb) for tb in TBS] == [3, 3, 4, 4]
    assert [n_pairs(tb) for tb in TBS] == [15, 21, 28, 36]
    # the values the GPU cases rely on
    assert ja_of(6, 15) == 3 and ja_of(8, 28) == 4          # full lists at L = 10, 12: what ran before
    assert ja_of(7, 21) == 7 and ja_of(9, 36) == 9          # full lists at L = 11, 13: every iteration NPI
    assert ja_of(7, 20) == 6 and ja_of(9, 34) == 7          # the wave bits split
    for tb in TBS:
        assert ja_of(tb, 0) == 0 and ja_of(tb, tb * (npi_of(tb) - 1)) == 0
        assert ja_of(tb, tb * (npi_of(tb) - 1) + 1) == 1


@pytest.mark.parametrize("tb", TBS)
def test_every_pair_in_exactly_one_executed_slot(tb):
    npi = npi_of(tb)
    for ntt in range(n_pairs(tb) + 1):
        tt = slot_table(tb, ntt)
        ex = executed(tb, ntt)
        held = [tt[s] for s in ex if tt[s] is not None]
        assert sorted(held) == list(range(ntt)), (tb, ntt)
        assert all(v is None or 0 <= v < ntt for v in tt.values()), (tb, ntt)
        if ntt >= tb * (npi - 1):  # no padded pair is executed
            assert len(ex) == ntt, (tb, ntt)
        else:
            assert len(ex) == tb * (npi - 1), (tb, ntt)


@pytest.mark.parametrize("tb", TBS)
def test_enumeration_sees_a_slot_off_by_one(tb):
    """The check above is not vacuous: with max(0, j - ja - 1) in the slot index, lists that make
    ja < TB - 1 lose or repeat a pair."""
    bad = 0
    for ntt in range(n_pairs(tb) + 1):
        tt = slot_table(tb, ntt, back=lambda j, ja: max(0, j - ja - 1))
        held = [tt[s] for s in executed(tb, ntt) if tt[s] is not None]
        if sorted(held) != list(range(ntt)):
            bad += 1
            assert ja_of(tb, ntt) < tb - 1
    assert bad > 0
