"""tetra_lmac_etsi_acquire_groups (k_cell_acquire_groups between a BSCH pass and the SCH pass of the
production trellis) on rows built on the CPU: every case against tests/_lmac_groups.py
oracle_groups -- nburst, every burst, nblock, every block and its type-1 bits (assert_rows_equal),
cell_init and ngood.  Integer and bit-exact: no tolerance anywhere.  tests/test_lmac_groups_model.py
proves on the CPU that the model and the hand-built cases mean what is assumed here.
"""
import os

import numpy as np
import pytest

import _lmac_rows as R
import _lmac_groups as GR

pytestmark = pytest.mark.gpu

N, P, SB = R.NDB_N, R.NDB_P, R.SB
SCALE = max(1, int(os.environ.get("TETRA_FUZZ_SCALE", "1")))


def test_one_row_groups_equal_lmac_etsi_acquire():
    """G = 1 over viterbi_batch rows (every block kind, adversarial soft bits, synchronisation bursts
    in every row): every output and cell_init equal tetra_lmac_etsi_acquire's bit for bit."""
    b = R.viterbi_batch(300, 37, 2)
    C = len(b["nsym"])
    init = np.where(np.arange(C) % 3 == 0, b["cells"], 3).astype(np.uint32)
    out, want, after, good = GR.check_groups(b["hard"], b["soft"], b["nsym"], 1, init, "G = 1")
    ref_state = init.copy()
    ref = R.run_lmac(b["hard"], b["soft"], b["nsym"], cell_init=ref_state)
    assert ref_state.tolist() == after
    assert np.array_equal(out["nburst"], ref["nburst"]) and np.array_equal(out["nblock"], ref["nblock"])
    assert R.live_outputs(out) == R.live_outputs(ref)   # entries past the counts are not written: unspecified
    assert sum(good) > 0


@pytest.mark.parametrize("where", [2, 0])
def test_sync_burst_in_one_row_serves_the_group(where):
    """G = 3, the synchronisation burst only in row 2 (rows 0 and 1, before it, are decoded with its
    cell) or only in row 0; a second group beside it hears nothing and keeps its init."""
    rng = np.random.default_rng(31 + where)
    rows, init, A = GR.case_sync_in_row(rng, where)
    B, _ = R.cell_fields(rng)
    rows += [GR.row(rng, [(r, N, B, None), (0, P, B, None)]) for r in range(3)]
    hard, soft, nsym = GR.pack(rows)
    out, want, after, good = GR.check_groups(hard, soft, nsym, 3, init + [B], "sync in row %d" % where)
    assert after == [A, B] and good == [1, 0]
    assert all(all(GR.crc_flags(w)) for w in want)


def test_no_sync_burst_keeps_the_init():
    """No synchronisation burst: init 3 stays 3 (blocks fail), a real cell stays (blocks pass), ngood 0."""
    rng = np.random.default_rng(33)
    A, _ = R.cell_fields(rng)
    rows = [GR.row(rng, [(r, N, A, None), (3, P, A, None)]) for r in range(4)]
    hard, soft, nsym = GR.pack(rows)
    out, want, after, good = GR.check_groups(hard, soft, nsym, 2, [3, A], "no sync")
    assert after == [3, A] and good == [0, 0]
    assert not any(GR.crc_flags(want[0]) + GR.crc_flags(want[1])) and all(GR.crc_flags(want[2]) + GR.crc_flags(want[3]))


def test_hand_built_groups():
    """Two cells in one group (the later wins), a BSCH with a broken CRC after a good one (the good
    one stays), the all-zero cell (init 3 with ngood > 0): the model's answers, known from
    tests/test_lmac_groups_model.py."""
    rng = np.random.default_rng(34)
    rows, init, A, B = GR.case_two_cells(rng)
    hard, soft, nsym = GR.pack(rows)
    _, _, after, good = GR.check_groups(hard, soft, nsym, 3, init, "two cells")
    assert after == [B] and good == [2]
    rows, init, A = GR.case_broken_after_good(rng)
    hard, soft, nsym = GR.pack(rows)
    _, _, after, good = GR.check_groups(hard, soft, nsym, 2, init, "broken after good")
    assert after == [A] and good == [1]
    rows, init, Z = GR.case_zero_cell(rng)
    hard, soft, nsym = GR.pack(rows)
    _, want, after, good = GR.check_groups(hard, soft, nsym, 2, init, "zero cell")
    assert after == [3] and good == [1] and all(GR.crc_flags(want[0]) + GR.crc_flags(want[1]))


@pytest.mark.parametrize("NG", [1, 5, 67])
def test_group_counts_off_the_workgroup_width(NG):
    """1, 5 and 67 groups of 3 rows (no multiple of the group kernel's waves per workgroup, nor of
    the sync kernel's): the synchronisation burst in row g mod 3, every fifth group without one."""
    rng = np.random.default_rng(40 + NG)
    rows, inits, cells = [], [], []
    for g in range(NG):
        A, fA = R.cell_fields(rng)
        heard = g % 5 != 4
        for r in range(3):
            if heard and r == g % 3:
                rows.append(GR.row(rng, [(g % 7, SB, A, R.sync_payloads(rng, fA)), (0, N, A, None)]))
            else:
                rows.append(GR.row(rng, [(r, P, A, None), (1, N, A, None)]))
        inits.append(3)
        cells.append(A if heard else 3)
    hard, soft, nsym = GR.pack(rows)
    _, _, after, good = GR.check_groups(hard, soft, nsym, 3, inits, "%d groups" % NG)
    assert after == cells and good == [int(c != 3) for c in cells]


def test_short_rows_and_a_full_burst_table():
    """Rows with nsym 0 and 1 inside a group (one before, one after the synchronisation burst's row),
    and a row of 8 bursts (ETSI_MAXB, 16 blocks) whose last burst is the group's only
    synchronisation burst."""
    rng = np.random.default_rng(50)
    A, fA = R.cell_fields(rng)
    full = [(0, (P, N)[i & 1], A, None) for i in range(7)] + [(0, SB, A, R.sync_payloads(rng, fA))]
    rows = [GR.empty_row(rng), GR.row(rng, [(2, SB, A, R.sync_payloads(rng, fA)), (0, P, A, None)]),
            GR.empty_row(rng), GR.row(rng, [(4, N, A, None)]),
            GR.row(rng, [(0, N, A, None)]), GR.row(rng, full), GR.empty_row(rng, 100), GR.row(rng, [(1, P, A, None)])]
    hard, soft, nsym = GR.pack(rows, 2050)
    nsym[0], nsym[2] = 0, 1
    out, want, after, good = GR.check_groups(hard, soft, nsym, 4, [3, 3], "short rows, full table")
    assert after == [A, A] and good == [1, 1]
    assert int(out["nburst"][5]) == 8 and int(out["nblock"][5]) == 13
    assert out["nburst"][[0, 2, 6]].tolist() == [0, 0, 0]
    assert all(all(GR.crc_flags(w)) for w in want)


def test_rows_that_are_not_whole_groups_are_refused():
    """C % G != 0 (and G = 0): TETRA_E_INVALID, and nothing is written -- outputs, cell_init, ngood."""
    rng = np.random.default_rng(51)
    rows, _, A = GR.case_sync_in_row(rng, 1)
    rows = rows + rows[:2]
    hard, soft, nsym = GR.pack(rows)
    for G in (2, 3, 4, 6, 0):
        out, state, ngood, rc = GR.run_groups(hard, soft, nsym, G, [3, 7])
        assert rc == -1, G
        assert state.tolist() == [3, 7] and ngood.tolist() == [-1, -1]
        assert not any(v.any() for v in out.values()), G
    out, state, ngood, rc = GR.run_groups(hard, soft, nsym, 5, [3])
    assert rc == 0 and state.tolist() == [A] and ngood.tolist() == [2]


def test_table_follows_the_state_after_configured_cells():
    """One context: a grouped call acquires A; tetra_etsi_set_cells + tetra_lmac_etsi with other
    cells rewrite the scrambler table; a grouped call without a synchronisation burst on the old
    state must decode with A again, not with the table the configured call left."""
    rng = np.random.default_rng(52)
    rows, init, A = GR.case_sync_in_row(rng, 1)
    hard, soft, nsym = GR.pack(rows)
    _, _, after, _ = GR.check_groups(hard, soft, nsym, 3, init, "first grouped call")
    assert after == [A]
    B, _ = R.cell_fields(rng)
    rows_b = [GR.row(rng, [(r, N, B, None), (0, P, B, None)]) for r in range(3)]
    hb, sb, nb = GR.pack(rows_b, hard.shape[1])
    cells = np.full(3, B, np.uint32)
    out = R.run_lmac(hb, sb, nb, cells)
    R.assert_rows_equal(out, R.oracle_rows(hb, sb, nb, cells), "configured cells")
    rows_a = [GR.row(rng, [(2 * r, P, A, None), (1, N, A, None)]) for r in range(3)]
    ha, sa, na = GR.pack(rows_a, hard.shape[1])
    _, want, after, good = GR.check_groups(ha, sa, na, 3, after, "second grouped call")
    assert after == [A] and good == [0] and all(all(GR.crc_flags(w)) for w in want)


def test_device_pointers_give_the_host_pointers_outputs():
    rows, inits = GR.random_groups(60, 9, 3)
    hard, soft, nsym = GR.pack(rows)
    host = GR.check_groups(hard, soft, nsym, 3, inits, "host pointers")
    dev = GR.check_groups(hard, soft, nsym, 3, inits, "device pointers", device=True)
    assert R.live_outputs(host[0]) == R.live_outputs(dev[0])
    assert host[2:] == dev[2:]


@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_random_sweep(G):
    """Seeded random groups (tests/_lmac_groups.py random_groups: kinds, gaps and soft classes of
    _lmac_rows, cells announced, changed and broken, incoming inits unknown / right / wrong), fresh
    seeds per TETRA_FUZZ_SCALE step; the state is carried into a second call on other rows."""
    for rep in range(SCALE):
        seed = 1000 * G + rep
        NG = 11 + 2 * G
        rows, inits = GR.random_groups(seed, NG, G)
        hard, soft, nsym = GR.pack(rows)
        _, _, after, _ = GR.check_groups(hard, soft, nsym, G, inits, "sweep %d" % seed)
        rows2, _ = GR.random_groups(seed + 500, NG, G)
        h2, s2, n2 = GR.pack(rows2)
        GR.check_groups(h2, s2, n2, G, after, "sweep %d, second call" % seed)
