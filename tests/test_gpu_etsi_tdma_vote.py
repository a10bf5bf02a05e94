"""tetra_etsi_mac_vote_groups (k_mac_walk + k_tdma_vote_groups) on the GPU against tests/_etsi_tdma_vote.py:
keep, every live slot row, npdu, every live PDU record, tvote and the carried timebases and scores --
integers, compared exactly, on hand-made lower-MAC outputs and link-quality records poisoned past every
count.

  * the hand cases (expected values written by hand in the model module), each also against the model;
    the two that show the feature also against tetra_etsi_mac_groups on the same arrays;
  * sizes: groups of 1, 3 and 64 rows in 1, 5 and 67 groups, full burst tables, nburst / nblock 0,
    negative and above MAXB / MAXJ; refused shapes leave every output as it was;
  * host and device pointers; a seeded sweep with random records, two caps and a second call on the carried
    state; G = 1 against tetra_etsi_mac itself.
tests/test_etsi_tdma_vote_model.py checks the model on the CPU.
"""
import os

import numpy as np
import pytest

import _etsi_mac_model as M
import _etsi_mac_groups as MG
import _etsi_tdma_vote as TV

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("TETRA_FUZZ_SCALE", "1")))
U = MG.UNWRITTEN


def _outputs(C, NG):
    """keep, slots, npdu, pdus, tvote, every one UNWRITTEN."""
    return (np.full((C, M.MAXB), U, np.int32), np.full((C, M.MAXB, 4), U, np.int32), np.full((C, M.MAXJ), U, np.int32),
            np.full((C, M.MAXJ, M.MAXPDU, M.NF), U, np.int32), np.full((NG, 4), U, np.int32))


def _inputs(arrays):
    return [np.ascontiguousarray(v, np.int32) for v in arrays[:4]] + [np.ascontiguousarray(arrays[4], np.uint8)] + \
           [np.ascontiguousarray(v, np.int32) for v in arrays[5:7]]


def call_vote(G, row_bits, tol, advance, cap, arrays, tdma, tscore, rc_only=False, device=False):
    """tetra_etsi_mac_vote_groups on host arrays (or device copies of them); tdma (TDMA_DTYPE [C / G]) and
    tscore (int32 [C / G]) are updated in place.  Returns (npdu, pdus, slots, keep, tvote), every output
    started as UNWRITTEN."""
    from tetraear import _hip
    c = _hip.ctx()
    C = len(arrays[0])
    NG = len(tdma)
    a = _inputs(arrays)
    outs = list(_outputs(C, NG))
    nsym = np.zeros(C, np.int32)
    args = [nsym] + a + [tdma, tscore] + outs
    if device:
        import torch
        args = [torch.from_numpy(v.view(np.int64).reshape(NG, 3).copy() if v is tdma else v).cuda() for v in args]
        torch.cuda.synchronize()
    p = [_hip.ptr(v) for v in args]
    rc = c.lib.tetra_etsi_mac_vote_groups(c.handle, p[0], C, G, row_bits, tol, advance, cap, *p[1:])
    if device:
        c.synchronize()
        host = [v.cpu().numpy() for v in args]
        tdma[:] = host[8].view(M.TDMA_DTYPE).reshape(NG)
        tscore[:] = host[9]
        outs = host[10:]
    keep, slots, npdu, pdus, tvote = outs
    if rc_only:
        return rc, (npdu, pdus, slots, keep, tvote)
    c.check(rc, "tetra_etsi_mac_vote_groups")
    return npdu, pdus, slots, keep, tvote


def call_groups(G, row_bits, tol, advance, arrays, tdma):
    """tetra_etsi_mac_groups on the same arrays: (npdu, pdus, slots, keep)."""
    from tetraear import _hip
    c = _hip.ctx()
    C = len(arrays[0])
    keep, slots, npdu, pdus, _ = _outputs(C, 1)
    c.check(c.lib.tetra_etsi_mac_groups(c.handle, _hip.ptr(np.zeros(C, np.int32)), C, G, row_bits, tol, advance,
                                        *[_hip.ptr(v) for v in _inputs(arrays)[:5]], _hip.ptr(tdma), _hip.ptr(keep),
                                        _hip.ptr(slots), _hip.ptr(npdu), _hip.ptr(pdus)), "tetra_etsi_mac_groups")
    return npdu, pdus, slots, keep


def assert_untouched(out, want, nburst):
    npdu, pdus, slots, keep, tvote = out
    live = np.arange(M.MAXPDU)[None, None, :] < np.minimum(want[0], M.MAXPDU)[:, :, None]
    assert np.all(pdus[~live] == U)
    rows = np.arange(M.MAXB)[None, :] < np.clip(np.asarray(nburst), 0, M.MAXB)[:, None]
    assert np.all(slots[~rows] == U) and np.all(keep[~rows] == U)
    assert set(np.unique(keep[rows]).tolist()) <= {0, 1}


def check(G, row_bits, tol, advance, cap, arrays, tdma=None, tscore=None, what="", device=False):
    """One call against the model from the state (tdma, tscore): (out, want, tdma after, tscore after)."""
    NG = len(arrays[0]) // G
    models = [MG.GroupTdma(*s) for s in tdma.tolist()] if tdma is not None else [MG.GroupTdma() for _ in range(NG)]
    scores = [0] * NG if tscore is None else [int(v) for v in tscore]
    tdma, tscore = M.tdma_array(models), np.array(scores, np.int32)
    want = TV.run(G, row_bits, tol, advance, cap, *arrays, models, scores)
    out = call_vote(G, row_bits, tol, advance, cap, arrays, tdma, tscore, device=device)
    TV.assert_equal(out, want, what)
    assert_untouched(out, want, arrays[0])
    assert tdma.tolist() == M.tdma_array(models).tolist(), what
    assert tscore.tolist() == scores, (what, tscore.tolist(), scores)
    return out, want, tdma, tscore


CASES = TV.hand_cases()


def _case(name):
    return next(c for c in CASES if c["name"] == name)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"].replace(" ", "_"))
def test_hand_cases(case):
    rng = np.random.default_rng(2)
    tdma, tscore = M.tdma_array([MG.GroupTdma(*case["state"])]), np.array([case["score"]], np.int32)
    for k, call in enumerate(case["calls"]):
        arrays = TV.arrays_of(rng, call["rows"])
        out, want, tdma, tscore = check(case["G"], case["row_bits"], case["tol"], call["advance"], case["cap"], arrays,
                                        tdma, tscore, (case["name"], k))
        npdu, pdus, slots, keep, tvote = out
        for (i, b), row in call["slots"].items():
            assert slots[i, b].tolist() == row, (case["name"], k, i, b, slots[i, b].tolist())
        for (i, b), v in call["keep"].items():
            assert keep[i, b] == v, (case["name"], k, i, b)
        assert tvote[0].tolist() == call["tvote"], (case["name"], k, tvote)
        assert tuple(tdma[0].tolist()) == call["state"] and int(tscore[0]) == call["score"], (case["name"], k, tdma, tscore)


@pytest.mark.parametrize("name", ["a foreign SYNC off the grid", "a foreign SYNC on the grid bit"])
def test_a_foreign_sync_does_not_move_the_grid(name):
    """Three SBs of w = 15240 on the grid, a foreign SB (another slot, w = 5000), four bursts on the true
    grid.  tetra_etsi_mac_groups on the same arrays re-anchors -- off the grid bit the four read 0, 0, 0, 0,
    on it they carry the foreign slot numbers; the vote leaves the grid where it was."""
    rng = np.random.default_rng(11)
    call = _case(name)["calls"][0]
    arrays = TV.arrays_of(rng, call["rows"])
    assert [TV.weight(arrays[6][0, j]) for j in (0, 2, 4, 6)] == [15240, 15240, 15240, 5000]
    old = call_groups(1, 0, 32, 98, arrays, M.tdma_array([MG.GroupTdma()]))
    assert old[2][0, 3].tolist() == [1, 15, 28, 3]   # slot 2000 taken at its word
    if "off" in name:
        assert old[2][0, 4:8].tolist() == [[0, 0, 0, 0]] * 4
    else:
        assert old[2][0, 4:8].tolist() == [[2, 15, 28, 0], [3, 15, 28, 0], [4, 15, 28, 0], [1, 16, 28, 0]]
    tdma, tscore = M.tdma_array([MG.GroupTdma()]), np.zeros(1, np.int32)
    npdu, pdus, slots, keep, tvote = call_vote(1, 0, 32, 98, TV.CAP_DEFAULT, arrays, tdma, tscore)
    assert slots[0, 3].tolist() == ([0, 0, 0, 0] if "off" in name else [2, 4, 1, 6])
    want = [13, 14, 15, 16] if "off" in name else [14, 15, 16, 17]
    assert slots[0, 4:8].tolist() == [TV.slot_row(s, 0) for s in want]
    assert tvote[0].tolist() == [4, 2, 1, 0] and int(tscore[0]) == 3 * 15240 - 5000
    assert np.array_equal(npdu, old[0]) and np.array_equal(pdus, old[1])   # the unchanged walk_block


def test_the_better_copy_is_kept():
    """A burst in an overlap whose row-0 copy has both blocks CRC-bad and whose row-1 copy has both good:
    tetra_etsi_mac_groups keeps row 0's, the vote row 1's."""
    rng = np.random.default_rng(12)
    P = lambda start, crc: (start, 1, None, dict(crc=crc))
    arrays = TV.arrays_of(rng, [[P(440, (1, 1)), P(2000, (0, 0))], [P(36, (1, 1)), P(544, (1, 0))]])
    old = call_groups(2, 1966, 32, 3932, arrays, M.tdma_array([MG.GroupTdma()]))
    assert old[3][0, :2].tolist() == [1, 1] and old[3][1, :2].tolist() == [0, 1]
    out = call_vote(2, 1966, 32, 3932, TV.CAP_DEFAULT, arrays, M.tdma_array([MG.GroupTdma()]), np.zeros(1, np.int32))
    assert out[3][0, :2].tolist() == [1, 0] and out[3][1, :2].tolist() == [1, 1]
    assert out[4][0].tolist() == [0, 0, 0, 0]


def _odd_block_counts(rng, arrays):
    """nblock of some rows 0, negative or above MAXJ (nburst: random_groups does that)."""
    nblock = arrays[2]
    for c in range(len(nblock)):
        if rng.integers(0, 6) == 0:
            nblock[c] = int(rng.choice((0, -1, -1000, M.MAXJ + 1, 1000)))
    return arrays


def _random_input(rng, NG, G, row_bits, full=False):
    arrays = _odd_block_counts(rng, MG.random_groups(rng, NG, G, row_bits, full=full))
    return arrays + TV.random_quality(rng, arrays)


@pytest.mark.parametrize("NG", [1, 5, 67])
def test_full_tables_at_64_rows_a_group(NG):
    """512 entries a group: every LDS slot of the sort, the cluster walk and the ballot list in use."""
    rng = np.random.default_rng(NG)
    arrays = _random_input(rng, NG, 64, 1966, full=True)
    assert np.count_nonzero(np.clip(arrays[0], 0, M.MAXB) == M.MAXB) >= 55 * NG
    if NG == 1:
        arrays[0][:] = M.MAXB + 3   # every row full, counts above MAXB
    tdma = M.tdma_array([MG.GroupTdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(NG)])
    out, want, tdma, tscore = check(64, 1966, 32, 64 * 1966, TV.CAP_DEFAULT, arrays, tdma, None, "first")
    assert len(want[3]) >= 440 * NG and 0 < sum(want[3].values()) < len(want[3])
    assert want[4][:, TV.BALLOTS].sum() >= 10 * NG
    check(64, 1966, 32, 1, TV.CAP_DEFAULT, _random_input(rng, NG, 64, 1966, full=True), tdma, tscore, "second")


@pytest.mark.parametrize("NG,G", [(1, 1), (5, 1), (67, 1), (1, 3), (5, 3), (67, 3), (5, 9)])
def test_group_counts_and_odd_counts(NG, G):
    rng = np.random.default_rng(100 * NG + G)
    arrays = _random_input(rng, NG, G, 1966)
    if NG * G > 150:
        nb, nk = arrays[0], arrays[2]
        assert (nb == 0).any() and (nb < 0).any() and (nk <= 0).any() and (nk > M.MAXJ).any(), (np.unique(nb), np.unique(nk))
    out, want, tdma, tscore = check(G, 1966, 32, G * 1966 - 1080, 20000, arrays, None, None, "first")
    if NG * G > 60:   # the inputs hold what they are meant to
        flags = {r[3] for r in want[2].values()}
        assert {0, 1}.issubset(flags) and [0, 0, 0, 0] in want[2].values() and (tscore > 0).any()
    check(G, 1966, 32, G * 1966 - 1080, 20000, _random_input(rng, NG, G, 1966), tdma, tscore, "a carried tail")


def test_refused_shapes_write_nothing():
    rng = np.random.default_rng(4)
    arrays = _random_input(rng, 2, 3, 1966)
    bad = ((0, 1966, 32, 100), (65, 1966, 32, 100), (4, 1966, 32, 100), (5, 1966, 32, 100), (3, -1, 32, 100),
           (3, 1966, -1, 100), (3, 1966, 32, 0), (3, 1966, 32, -5))
    for G, row_bits, tol, cap in bad:
        tdma, tscore = M.tdma_array([MG.GroupTdma(7, 8, 9, 1) for _ in range(2)]), np.array([11, 12], np.int32)
        rc, out = call_vote(G, row_bits, tol, 100, cap, arrays, tdma, tscore, rc_only=True)
        assert rc == -1, (G, row_bits, tol, cap, rc)
        assert all(np.all(v == U) for v in out), (G, row_bits, tol, cap)
        assert tdma.tolist() == [(7, 8, 9, 1)] * 2 and tscore.tolist() == [11, 12]
    from tetraear import _hip
    c = _hip.ctx()
    a = _inputs(arrays)
    tdma, tscore = M.tdma_array([MG.GroupTdma(7, 8, 9, 1) for _ in range(2)]), np.array([11, 12], np.int32)
    outs = list(_outputs(6, 2))
    full = [np.zeros(6, np.int32)] + a + [tdma, tscore] + outs
    for skip in range(len(full)):   # every array NULL in turn
        p = [None if i == skip else _hip.ptr(v) for i, v in enumerate(full)]
        assert c.lib.tetra_etsi_mac_vote_groups(c.handle, p[0], 6, 3, 1966, 32, 100, 100, *p[1:]) == -1, skip
    assert c.lib.tetra_etsi_mac_vote_groups(c.handle, _hip.ptr(full[0]), 0, 3, 1966, 32, 100, 100,
                                            *[_hip.ptr(v) for v in full[1:]]) == -1
    assert all(np.all(v == U) for v in outs) and tdma.tolist() == [(7, 8, 9, 1)] * 2 and tscore.tolist() == [11, 12]
    rc, out = call_vote(3, 1966, 32, 100, 1, arrays, tdma, tscore, rc_only=True)
    assert rc == 0 and not np.all(out[2] == U) and not np.any(out[4] == U)


def test_device_pointers_equal_host_pointers():
    rng = np.random.default_rng(8)
    G, NG = 9, 40
    arrays = _random_input(rng, NG, G, 1966, full=True)
    state = M.tdma_array([MG.GroupTdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(NG)])
    score = rng.integers(-5, 3000, NG).astype(np.int32)
    host, want, th, sh = check(G, 1966, 32, 12345, 9000, arrays, state.copy(), score.copy(), "host")
    dev, _, td, sd = check(G, 1966, 32, 12345, 9000, arrays, state.copy(), score.copy(), "device", device=True)
    for name, x, y in zip(("npdu", "pdus", "slots", "keep", "tvote"), host, dev):
        assert np.array_equal(x, y), name
    assert th.tolist() == td.tolist() and sh.tolist() == sd.tolist()
    # a second call on the carried state
    check(G, 1966, 32, 0, 9000, _random_input(rng, NG, G, 1966), td, sd, "second", device=True)


def test_seeded_sweep():
    """A few hundred groups over seeds: group counts, G, row spacing, tolerance, two caps, random records
    (some -1), the carried state and score."""
    groups, seen, flags = 0, np.zeros(4, np.int64), set()
    for seed in range(24 * SCALE):
        rng = np.random.default_rng(7000 + seed)
        G = int(rng.choice((1, 2, 3, 8, 9, 10, 33, 64)))
        NG = int(rng.choice((1, 2, 7, 16, 31)))
        row_bits, tol = int(rng.choice((1966, 1966, 510, 0, 1 << 33))), int(rng.choice((32, 32, 0, 3, 511)))
        cap = (3000, TV.CAP_DEFAULT)[seed % 2]
        tdma = M.tdma_array([MG.GroupTdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(NG)])
        gen_bits = min(row_bits, 1966)
        _, w0, tdma, tscore = check(G, row_bits, tol, G * gen_bits - int(rng.integers(0, 1500)), cap,
                                    _random_input(rng, NG, G, gen_bits, full=bool(seed % 3 == 0)), tdma, None,
                                    "seed %d, call 0" % seed, device=bool(seed % 4 == 1))
        _, w1, _, tscore = check(G, row_bits, tol, 0, cap, _random_input(rng, NG, G, gen_bits), tdma, tscore,
                                 "seed %d, call 1" % seed)
        assert tscore.min() >= 0 and tscore.max() <= cap
        for w in (w0, w1):
            seen += w[4].sum(axis=0)
            flags |= {r[3] for r in w[2].values()}
        groups += NG
    assert groups >= 200 and (seen > 0).all() and flags == {0, 1, 3, 6}, (groups, seen, flags)


def test_one_row_groups_equal_tetra_etsi_mac():
    """G = 1, row_bits = 0 on rows of ascending bursts where no SYNC contradicts its prediction: slots, npdu,
    pdus and tdma are tetra_etsi_mac's over two chunks (the second on the carried timebases), whatever the
    records weigh."""
    import test_gpu_etsi_mac as T
    rng = np.random.default_rng(6)
    nsym = 1301
    ta = tb = None
    for k in range(2):
        arrays = MG.random_groups(rng, 90, 1, 1660)
        if ta is None:
            ta = M.tdma_array([M.Tdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(90)])
        C = len(ta)
        arrays = tuple(v[:C] for v in arrays)
        ns = np.full(C, nsym, np.int32)
        trial = ta.copy()
        a = T.call_mac(ns, *arrays, trial)
        live = np.arange(M.MAXB)[None, :] < np.clip(arrays[0], 0, M.MAXB)[:, None]
        ok = ~np.any(live & ((a[2][..., 3] & 2) != 0), axis=1)   # rows without a contradiction
        if k == 0:
            ta = ta[ok].copy()
            tb = ta.copy()
        else:
            ta, tb = ta[ok].copy(), tb[ok].copy()
        arrays = tuple(np.ascontiguousarray(v[ok]) for v in arrays)
        C = len(ta)
        assert C >= 20, C
        a = T.call_mac(np.full(C, nsym, np.int32), *arrays, ta)
        full = arrays + TV.random_quality(rng, arrays)
        out, want, tb, _ = check(1, 0, 32, 2 * (nsym - 1), TV.CAP_DEFAULT, full, tb, None, "chunk %d" % k)
        live = live[ok]
        assert np.array_equal(a[0], out[0]) and np.array_equal(a[1], out[1]), k
        assert np.array_equal(a[2][live], out[2][live]) and ta.tolist() == tb.tolist(), k
        assert np.all(out[3][live] == 1)
    assert any(r[3] == 1 for r in want[2].values())
