"""The grouped cell-acquisition model (tests/_lmac_groups.py oracle_groups) on the CPU: what
tests/test_gpu_lmac_groups.py holds tetra_lmac_etsi_acquire_groups to means what is assumed there.
With G = 1 it is Receiver.lower_mac_acquire; the hand-built groups have the answers written here.
Integer and bit-exact: no tolerance anywhere.
"""
import numpy as np

import etsi as E
import _lmac_rows as R
import _lmac_groups as GR


def _same(a, b):
    """Two lists of lower_mac row results are equal (type-1 bits included)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        fx, fy = R.flatten(x), R.flatten(y)
        assert fx[:2] == fy[:2]
        assert all(np.array_equal(p, q) for p, q in zip(fx[2], fy[2]))


def test_one_row_groups_are_lower_mac_acquire():
    """G = 1 over Viterbi-batch rows (adversarial soft bits) and over random rows with synchronisation
    bursts: rows, cell_init after and ngood from oracle_groups equal lower_mac_acquire's rows and
    init, and ngood the CRC-good BSCH blocks of the row."""
    rx = E.Receiver()
    b = R.viterbi_batch(7, 6, 1)
    rows, inits = GR.random_groups(3, 12, 1)
    h2, s2, n2 = GR.pack(rows)
    for hard, soft, nsym, init in ((b["hard"], b["soft"], b["nsym"], [3] * 6), (h2, s2, n2, inits)):
        got, after, ngood = GR.oracle_groups(hard, soft, nsym, 1, init)
        want, state, good = [], [], []
        for ch in range(len(nsym)):
            nd = max(int(nsym[ch]) - 1, 0)
            w, i = rx.lower_mac_acquire(soft[ch, :2 * nd], hard[ch, :nd], int(init[ch]))
            want.append(w)
            state.append(i)
            good.append(sum(1 for _, _, dec in w for k, _, ok in dec if k == 2 and ok))
        _same(got, want)
        assert after == state and ngood == good
    assert sum(ngood) > 0 and any(a != i for a, i in zip(after, inits))   # the second batch acquired cells


def test_sync_burst_only_in_the_last_row():
    """Three rows of cell A, the synchronisation burst in row 2: rows 0 and 1 decode with A too; the
    same rows as groups of one leave rows 0 and 1 on the unknown cell, their blocks failing."""
    rng = np.random.default_rng(21)
    rows, init, A = GR.case_sync_in_row(rng, 2)
    hard, soft, nsym = GR.pack(rows)
    want, after, ngood = GR.oracle_groups(hard, soft, nsym, 3, init)
    assert after == [A] and ngood == [1]
    assert [len(w) for w in want] == [3, 3, 3]
    assert all(all(GR.crc_flags(w)) for w in want)
    alone, after1, ngood1 = GR.oracle_groups(hard, soft, nsym, 1, [3, 3, 3])
    assert after1 == [3, 3, A] and ngood1 == [0, 0, 1]
    assert not any(GR.crc_flags(alone[0])) and not any(GR.crc_flags(alone[1])) and all(GR.crc_flags(alone[2]))


def test_sync_burst_only_in_the_first_row():
    rng = np.random.default_rng(22)
    rows, init, A = GR.case_sync_in_row(rng, 0)
    hard, soft, nsym = GR.pack(rows)
    want, after, ngood = GR.oracle_groups(hard, soft, nsym, 3, init)
    assert after == [A] and ngood == [1] and all(all(GR.crc_flags(w)) for w in want)


def test_two_cells_in_one_group_the_later_wins():
    """A in row 0, B in row 2: the state is B, both BSCH blocks pass (colour code 0), every block
    scrambled with B passes -- row 0's included -- and the one scrambled with A fails."""
    rng = np.random.default_rng(23)
    rows, init, A, B = GR.case_two_cells(rng)
    hard, soft, nsym = GR.pack(rows)
    want, after, ngood = GR.oracle_groups(hard, soft, nsym, 3, init)
    assert A != B and after == [B] and ngood == [2]
    # row 0: BSCH, SB block 2 (A), SCH/F (B); row 1: SCH/F (A), 2 x SCH/HD (B); row 2: all of B
    assert GR.crc_flags(want[0]) == [True, False, True]
    assert GR.crc_flags(want[1]) == [False, True, True]
    assert GR.crc_flags(want[2]) == [True, True, True, True, True]


def test_broken_bsch_after_a_good_one_keeps_the_cell():
    rng = np.random.default_rng(24)
    rows, init, A = GR.case_broken_after_good(rng)
    hard, soft, nsym = GR.pack(rows)
    want, after, ngood = GR.oracle_groups(hard, soft, nsym, 2, init)
    assert after == [A] and ngood == [1]
    assert GR.crc_flags(want[0]) == [True, True, True]
    assert GR.crc_flags(want[1]) == [True, True, False, True, True]   # the noise BSCH alone fails


def test_no_sync_burst_keeps_the_init_and_zero_cell_counts():
    """No synchronisation burst: the incoming init stays (3, or a real cell) with ngood 0.  The
    all-zero cell leaves init 3 too, told apart by ngood."""
    rng = np.random.default_rng(25)
    A, _ = R.cell_fields(rng)
    rows = [GR.row(rng, [(0, R.NDB_N, A, None), (3, R.NDB_P, A, None)]) for _ in range(4)]
    hard, soft, nsym = GR.pack(rows)
    want, after, ngood = GR.oracle_groups(hard, soft, nsym, 2, [3, A])
    assert after == [3, A] and ngood == [0, 0]
    assert not any(GR.crc_flags(want[0]) + GR.crc_flags(want[1]))
    assert all(GR.crc_flags(want[2]) + GR.crc_flags(want[3]))
    rows, init, Z = GR.case_zero_cell(rng)
    hard, soft, nsym = GR.pack(rows)
    want, after, ngood = GR.oracle_groups(hard, soft, nsym, 2, init)
    assert after == [3] and ngood == [1] and all(GR.crc_flags(want[0]) + GR.crc_flags(want[1]))


def test_random_groups_cover_the_sweep():
    """The sweep's generator: rows fit the widest row the library takes, and over a few seeds it
    holds groups that acquire, groups that keep their init, failed BSCH blocks and empty rows."""
    seen = dict(acquired=0, kept=0, bad_bsch=0, empty=0)
    for seed, G in ((1, 1), (2, 2), (3, 3), (4, 4)):
        rows, inits = GR.random_groups(seed, 6, G)
        assert len(rows) == 6 * G and max(len(b) for b, _ in rows) <= 2 * 2048
        hard, soft, nsym = GR.pack(rows)
        want, after, ngood = GR.oracle_groups(hard, soft, nsym, G, inits)
        seen["acquired"] += sum(g > 0 for g in ngood)
        seen["kept"] += sum(g == 0 for g in ngood)
        assert all(a == i for a, i, g in zip(after, inits, ngood) if g == 0)
        seen["bad_bsch"] += sum(1 for w in want for _, _, dec in w for k, _, ok in dec if k == 2 and not ok)
        seen["empty"] += sum(len(w) == 0 for w in want)
    assert min(seen.values()) > 0, seen
