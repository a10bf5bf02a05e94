"""tests/_etsi_mac_groups.py (the CPU model of tetra_etsi_mac_groups) checked on the CPU: its keep
against merge_chunks, G = 1 against _etsi_mac_model.run, and the hand cases, whose expected rows are
written out by hand.  tests/test_gpu_etsi_mac_groups.py holds the kernel to the model."""
import numpy as np

import _etsi_mac_model as M
import _etsi_mac_groups as MG


def _keep_array(want, C):
    keep = np.zeros((C, M.MAXB), bool)
    for (c, b), v in want[3].items():
        keep[c, b] = bool(v)
    return keep


def test_keep_equals_merge_chunks():
    """Well-formed groups (with nburst 0, negative and above MAXB) and ill-formed arrays (any start
    bits, ties, any order): the model's keep is merge_chunks' on the same arrays, stride = 2 row_bits
    samples and tol = 2 tol_bits."""
    from tetraear.signal.wideband import merge_chunks
    for seed in range(30):
        rng = np.random.default_rng(seed)
        G = int(rng.choice((1, 2, 3, 9, 64)))
        NG = int(rng.integers(1, 5))
        row_bits, tol = int(rng.choice((1966, 0, 700))), int(rng.choice((32, 0, 2, 600)))
        if seed % 2:
            nburst, bursts, nblock, blocks, type1 = MG.random_groups(rng, NG, G, row_bits, full=seed % 4 == 1)
        else:
            C = NG * G
            nburst = rng.integers(-2, M.MAXB + 3, C).astype(np.int32)
            bursts = np.zeros((C, M.MAXB, 2), np.int32)
            bursts[..., 0] = rng.integers(-50, 50, (C, M.MAXB)) * int(rng.choice((1, 20, 510)))
            bursts[..., 1] = rng.integers(0, 3, (C, M.MAXB))
            nblock, blocks = np.zeros(C, np.int32), np.zeros((C, M.MAXJ, 4), np.int32)
            type1 = np.zeros((C, M.MAXJ, 268), np.uint8)
        C = len(nburst)
        want = MG.run(G, row_bits, tol, 0, nburst, bursts, nblock, blocks, type1, [MG.GroupTdma() for _ in range(NG)])
        keep, _ = merge_chunks(nburst, bursts, nblock, blocks, NG, G, 2 * row_bits, 2 * tol)
        assert np.array_equal(_keep_array(want, C), keep), seed
        assert set(want[3]) == {(c, b) for c in range(C) for b in range(min(max(int(nburst[c]), 0), M.MAXB))}


def test_one_row_groups_equal_the_row_model():
    """G = 1, row_bits = 0, rows of ascending bursts (a slot apart or more) and advance = 2 max(nsym -
    1, 0): rows, records and the carried state equal _etsi_mac_model.run's over three chunks."""
    rng = np.random.default_rng(5)
    C, nsym = 12, 1301
    a, b = [M.Tdma() for _ in range(C)], [MG.GroupTdma() for _ in range(C)]
    seen = set()
    for k in range(3):
        arrays = MG.random_groups(rng, C, 1, 1660)
        ns = np.full(C, nsym, np.int32)
        wa = M.run(ns, *arrays, a)
        wb = MG.run(1, 0, 32, 2 * (nsym - 1), *arrays, b)
        assert np.array_equal(wa[0], wb[0]) and wa[1] == wb[1] and wa[2] == wb[2], k
        assert [t.state() for t in a] == [t.state() for t in b], k
        seen |= {tuple(r) for r in wa[2].values()}
    assert any(r[3] == 1 for r in seen) and any(r[3] == 3 for r in seen) and (0, 0, 0, 0) in seen
    assert any(r[3] == 0 and r[0] for r in seen)


def test_hand_cases():
    rng = np.random.default_rng(1)
    cases = MG.hand_cases()
    assert len({c["name"] for c in cases}) == len(cases) >= 20
    for case in cases:
        td = [MG.GroupTdma(*case["state"])]
        for k, call in enumerate(case["calls"]):
            assert len(call["rows"]) == case["G"]
            arrays = MG.arrays_of(rng, call["rows"])
            want = MG.run(case["G"], case["row_bits"], case["tol"], call["advance"], *arrays, td)
            assert want[2] == call["slots"], (case["name"], k, want[2])
            assert want[3] == call["keep"], (case["name"], k, want[3])
            assert td[0].state() == call["state"], (case["name"], k, td[0].state())


def test_the_group_rule_differs_from_the_row_rule_only_behind_the_anchor():
    """The one deliberate difference: a burst behind the anchor drops the row model's lock, and is
    placed (anchor and lock kept) by the group model."""
    row, grp = M.Tdma(0, 1000, 10, 1), MG.GroupTdma(0, 1000, 10, 1)
    assert row.chunk(1, [(490, 0)], [None]) == [[0, 0, 0, 0]] and row.locked == 0
    assert grp.burst(490, None) == [2, 3, 1, 0] and grp.state() == (0, 1000, 10, 1)
