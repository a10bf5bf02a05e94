"""tests/_etsi_tdma_vote.py (the CPU model of tetra_etsi_mac_vote_groups) checked on the CPU: the hand cases,
whose expected rows, keeps, scores and tvote are written out by hand from the rule in include/tetra_hip.h;
the equivalence with tetra_etsi_mac_groups' model where no cluster holds two own-SYNC bursts and no SYNC
contradicts its prediction; keep exactly once per cluster.  tests/test_gpu_etsi_tdma_vote.py holds the
kernel to the model."""
import numpy as np

import _etsi_mac_model as M
import _etsi_mac_groups as MG
import _etsi_tdma_vote as TV


def run_case(case, rng):
    """A hand case through the model: every call's expected values."""
    td, ts = [MG.GroupTdma(*case["state"])], [case["score"]]
    for k, call in enumerate(case["calls"]):
        assert len(call["rows"]) == case["G"]
        arrays = TV.arrays_of(rng, call["rows"])
        want = TV.run(case["G"], case["row_bits"], case["tol"], call["advance"], case["cap"], *arrays, td, ts)
        what = (case["name"], k)
        assert want[2] == call["slots"], (what, want[2])
        assert want[3] == call["keep"], (what, want[3])
        assert want[4][0].tolist() == call["tvote"], (what, want[4])
        assert td[0].state() == call["state"], (what, td[0].state())
        assert ts[0] == call["score"], (what, ts[0])


def test_hand_cases():
    rng = np.random.default_rng(1)
    cases = TV.hand_cases()
    assert len({c["name"] for c in cases}) == len(cases) >= 24
    for case in cases:
        run_case(case, rng)


def _case(name):
    return next(c for c in TV.hand_cases() if c["name"] == name)


def test_the_sequence_of_a_b_and_c():
    """The hand case spelled out once more, score by score (a second statement of the same sequence)."""
    case = _case("a b c in sequence")
    row = case["calls"][0]["rows"][0]
    arrays = TV.arrays_of(np.random.default_rng(3), [row])
    scores = []
    for n in range(1, len(row) + 1):   # the first n bursts
        a = list(arrays)
        a[0] = np.array([n], np.int32)
        td, ts = [MG.GroupTdma()], [0]
        TV.run(1, 0, 32, 0, case["cap"], *a, td, ts)
        scores.append(ts[0])
    #          a     b     c <   c ==  c wins  -  b     c wins
    assert scores == [5000, 8000, 5000, 0, 1, 1, 7001, 1999]


def test_mac_groups_on_the_foreign_sync_re_anchors():
    """What the vote is for: tetra_etsi_mac_groups' model on the same arrays gives up the grid."""
    rng = np.random.default_rng(4)
    call = _case("a foreign SYNC off the grid")["calls"][0]
    arrays = TV.arrays_of(rng, call["rows"])
    old = MG.run(1, 0, 32, 98, *arrays[:5], [MG.GroupTdma()])
    assert old[2][(0, 3)] == [1, 15, 28, 3]   # slot 2000, FLAGS 3
    assert [old[2][(0, b)] for b in range(4, 8)] == [[0, 0, 0, 0]] * 4
    assert [call["slots"][(0, b)][:3] for b in range(4, 8)] == [[2, 4, 1], [3, 4, 1], [4, 4, 1], [1, 5, 1]]


def test_mac_groups_keeps_the_worse_copy():
    rng = np.random.default_rng(5)
    call = _case("keep by quality")["calls"][0]
    arrays = TV.arrays_of(rng, call["rows"])
    old = MG.run(2, 0, 32, 0, *arrays[:5], [MG.GroupTdma()])
    assert old[3][(0, 0)] == 1 and old[3][(1, 0)] == 0          # row 0's copy: both blocks CRC-bad
    assert arrays[3][0, :2, 1].tolist() == [0, 0] and arrays[3][1, :2, 1].tolist() == [1, 1]
    assert call["keep"][(0, 0)] == 0 and call["keep"][(1, 0)] == 1


def _own_sync(arrays):
    """{(c, b)} of the bursts with an own SYNC, read off tetra_etsi_mac_groups' model: FLAGS bit 0 from an
    unlocked walk of each row alone."""
    nburst, bursts, nblock, blocks, type1 = arrays[:5]
    C = len(nburst)
    rows = MG.run(1, 0, 0, 0, nburst, bursts, nblock, blocks, type1, [MG.GroupTdma() for _ in range(C)])[2]
    return {cb for cb, r in rows.items() if r[3] & 1}


def _equivalent_input(G, row_bits, tol, arrays, state):
    """The stated condition: no cluster holds two own-SYNC bursts, and tetra_etsi_mac_groups sets FLAGS
    bit 1 nowhere (no SYNC contradicts its prediction)."""
    NG = len(arrays[0]) // G
    own = _own_sync(arrays)
    for g in range(NG):
        for cl in TV.clusters(MG.merged_order(arrays[0], arrays[1], g * G, G, row_bits), tol):
            if sum((g * G + i, b) in own for _, i, b in cl) > 1:
                return False
    rows = MG.run(G, row_bits, tol, 0, *arrays[:5], [MG.GroupTdma(*s) for s in state])[2]
    return not any(r[3] & 2 for r in rows.values())


def test_equivalence_with_mac_groups():
    """On inputs of the stated condition, from score 0 and from cap (and a score in between): slots, FLAGS,
    tdma, npdu and the records are tetra_etsi_mac_groups' model's, over two calls; keep is its keep wherever
    the copies of a cluster have equal Q.  One group an input, so that one contradiction discards one
    group only; an input whose first call fails the condition is dropped, one whose second does is cut."""
    used = ballots = 0
    by_g = {}
    for seed in range(240):
        rng = np.random.default_rng(900 + seed)
        G = int(rng.choice((1, 2, 3, 5, 9)))
        row_bits, tol = 1966, int(rng.choice((32, 32, 3)))
        state = [(int(rng.integers(0, 1 << 45)), 0, 0, 0)]
        calls = [MG.random_groups(rng, 1, G, row_bits) for _ in range(2)]
        quality = [TV.random_quality(rng, a) for a in calls]
        for score in (0, TV.CAP_DEFAULT, 4000):
            old_td, new_td, ts = [MG.GroupTdma(*state[0])], [MG.GroupTdma(*state[0])], [score]
            for k, (a, (bq, kq)) in enumerate(zip(calls, quality)):
                if not _equivalent_input(G, row_bits, tol, a, [old_td[0].state()]):
                    break
                old = MG.run(G, row_bits, tol, G * row_bits - 1080, *a, old_td)
                new = TV.run(G, row_bits, tol, G * row_bits - 1080, TV.CAP_DEFAULT, *a, bq, kq, new_td, ts)
                assert np.array_equal(old[0], new[0]) and old[1] == new[1] and old[2] == new[2], (seed, score, k)
                assert old_td[0].state() == new_td[0].state(), (seed, score, k)
                for cl in TV.clusters(MG.merged_order(a[0], a[1], 0, G, row_bits), tol):
                    keys = {TV.quality_key(i, b, a[2], a[3], bq) for _, i, b in cl}
                    if len(keys) == 1:
                        assert all(old[3][(i, b)] == new[3][(i, b)] for _, i, b in cl), (seed, score, k)
                used += 1
                by_g[G] = by_g.get(G, 0) + 1
                ballots += int(new[4][0, TV.BALLOTS])
                assert new[4][0, TV.OUTVOTED] == new[4][0, TV.WON] == 0
    # (nine rows of random_groups hardly ever pass the filter: an SB in one of eight overlaps is enough)
    assert used >= 200 and ballots >= 200 and all(by_g.get(G, 0) >= 12 for G in (1, 2, 3, 5)), (used, ballots, by_g)


def test_keep_is_exactly_one_per_cluster():
    shared = 0   # clusters of more than one burst
    for seed in range(6):
        rng = np.random.default_rng(40 + seed)
        G, NG = int(rng.choice((2, 9, 64))), 2
        arrays = MG.random_groups(rng, NG, G, 1966, full=True)
        bq, kq = TV.random_quality(rng, arrays)
        want = TV.run(G, 1966, 32, 0, TV.CAP_DEFAULT, *arrays, bq, kq, [MG.GroupTdma() for _ in range(NG)], [0] * NG)
        for g in range(NG):
            for cl in TV.clusters(MG.merged_order(arrays[0], arrays[1], g * G, G, 1966), 32):
                kept = [(g * G + i, b) for _, i, b in cl if want[3][(g * G + i, b)]]
                assert len(kept) == 1, (seed, g, cl)
                best = max(TV.quality_key(g * G + i, b, arrays[2], arrays[3], bq) for _, i, b in cl)
                assert TV.quality_key(*kept[0], arrays[2], arrays[3], bq) == best
                shared += len(cl) > 1
        assert set(want[3]) == set(want[2]) == {(c, b) for c in range(NG * G)
                                                for b in range(min(max(int(arrays[0][c]), 0), M.MAXB))}
    assert shared >= 100, shared


def test_random_inputs_hold_what_they_are_meant_to():
    """The sweep inputs of the GPU test exercise every branch: a, b, both kinds of c, FLAGS 6, an own SYNC
    that is not the ballot, -1 records, keeps that differ from tetra_etsi_mac_groups'."""
    seen, flags, differ = np.zeros(4, np.int64), set(), 0
    for seed in range(8):
        rng = np.random.default_rng(7000 + seed)
        G, NG = int(rng.choice((2, 3, 9))), 7
        arrays = MG.random_groups(rng, NG, G, 1966)
        bq, kq = TV.random_quality(rng, arrays)
        assert (bq[..., 0] == -1).any() and (kq[..., 0] == -1).any()
        td, ts = [MG.GroupTdma() for _ in range(NG)], [0] * NG
        want = TV.run(G, 1966, 32, 0, 3000, *arrays, bq, kq, td, ts)
        old = MG.run(G, 1966, 32, 0, *arrays, [MG.GroupTdma() for _ in range(NG)])
        seen += want[4].sum(axis=0)
        flags |= {r[3] for r in want[2].values()}
        differ += sum(old[3][k] != want[3][k] for k in old[3])
        assert all(0 <= s <= 3000 for s in ts)
    assert (seen > 0).all() and flags == {0, 1, 3, 6} and differ > 0, (seen, flags, differ)
