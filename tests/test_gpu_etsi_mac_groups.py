"""tetra_etsi_mac_groups (k_mac_walk + k_tdma_groups) on the GPU against tests/_etsi_mac_groups.py:
keep, every live slot row, npdu, every live PDU record and the carried timebases -- integers, compared
exactly, on hand-made lower-MAC outputs poisoned past every count and past a block's n1.

  * the hand cases (expected rows written by hand in the model module), each also against the model;
  * sizes: G = 64 with every burst table full (512 entries a group), 1 / 5 / 67 groups, rows whose
    nburst is 0, negative or above MAXB; refused shapes leave every output as it was;
  * G = 1 against tetra_etsi_mac itself; host and device pointers; a seeded sweep.
tests/test_etsi_mac_groups_model.py checks the model on the CPU.
"""
import os

import numpy as np
import pytest

import _etsi_mac_model as M
import _etsi_mac_groups as MG

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("TETRA_FUZZ_SCALE", "1")))
U = MG.UNWRITTEN


def _outputs(C):
    return (np.full((C, M.MAXB), U, np.int32), np.full((C, M.MAXB, 4), U, np.int32), np.full((C, M.MAXJ), U, np.int32),
            np.full((C, M.MAXJ, M.MAXPDU, M.NF), U, np.int32))


def call_groups(G, row_bits, tol, advance, arrays, tdma, rc_only=False):
    """tetra_etsi_mac_groups on host arrays; tdma (TDMA_DTYPE array [C / G]) is updated in place.
    Returns (npdu, pdus, slots, keep), every output started as UNWRITTEN."""
    from tetraear import _hip
    c = _hip.ctx()
    C = len(arrays[0])
    a = [np.ascontiguousarray(v, np.int32) for v in arrays[:4]] + [np.ascontiguousarray(arrays[4], np.uint8)]
    keep, slots, npdu, pdus = _outputs(C)
    nsym = np.zeros(C, np.int32)
    rc = c.lib.tetra_etsi_mac_groups(c.handle, _hip.ptr(nsym), C, G, row_bits, tol, advance, *[_hip.ptr(v) for v in a],
                                     _hip.ptr(tdma), _hip.ptr(keep), _hip.ptr(slots), _hip.ptr(npdu), _hip.ptr(pdus))
    if rc_only:
        return rc, (npdu, pdus, slots, keep)
    c.check(rc, "tetra_etsi_mac_groups")
    return npdu, pdus, slots, keep


def assert_untouched(out, want, nburst):
    npdu, pdus, slots, keep = out
    live = np.arange(M.MAXPDU)[None, None, :] < np.minimum(want[0], M.MAXPDU)[:, :, None]
    assert np.all(pdus[~live] == U)
    rows = np.arange(M.MAXB)[None, :] < np.clip(np.asarray(nburst), 0, M.MAXB)[:, None]
    assert np.all(slots[~rows] == U) and np.all(keep[~rows] == U)
    assert set(np.unique(keep[rows]).tolist()) <= {0, 1}


def check(G, row_bits, tol, advance, arrays, tdma=None, what=""):
    NG = len(arrays[0]) // G
    models = [MG.GroupTdma(*s) for s in tdma.tolist()] if tdma is not None else [MG.GroupTdma() for _ in range(NG)]
    tdma = M.tdma_array(models)
    want = MG.run(G, row_bits, tol, advance, *arrays, models)
    out = call_groups(G, row_bits, tol, advance, arrays, tdma)
    MG.assert_equal(out, want, what)
    assert_untouched(out, want, arrays[0])
    assert tdma.tolist() == M.tdma_array(models).tolist(), what
    return out, want, tdma


@pytest.mark.parametrize("case", MG.hand_cases(), ids=lambda c: c["name"].replace(" ", "_"))
def test_hand_cases(case):
    rng = np.random.default_rng(2)
    G = case["G"]
    tdma = M.tdma_array([MG.GroupTdma(*case["state"])])
    for k, call in enumerate(case["calls"]):
        arrays = MG.arrays_of(rng, call["rows"])
        out, want, tdma = check(G, case["row_bits"], case["tol"], call["advance"], arrays, tdma, (case["name"], k))
        npdu, pdus, slots, keep = out
        for (i, b), row in call["slots"].items():
            assert slots[i, b].tolist() == row, (case["name"], k, i, b, slots[i, b].tolist())
        for (i, b), v in call["keep"].items():
            assert keep[i, b] == v, (case["name"], k, i, b)
        assert tuple(tdma[0].tolist()) == call["state"], (case["name"], k, tdma[0])


@pytest.mark.parametrize("NG", [1, 5, 67])
def test_full_tables_at_64_rows_a_group(NG):
    """512 entries a group: every LDS slot of the rank sort in use."""
    rng = np.random.default_rng(NG)
    arrays = MG.random_groups(rng, NG, 64, 1966, full=True)
    assert np.count_nonzero(np.clip(arrays[0], 0, M.MAXB) == M.MAXB) >= 55 * NG
    assert NG == 1 or (arrays[0] > M.MAXB).any()
    if NG == 1:
        arrays[0][:] = M.MAXB + 3   # every row full, counts above MAXB
    tdma = M.tdma_array([MG.GroupTdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(NG)])
    out, want, tdma = check(64, 1966, 32, 64 * 1966, arrays, tdma, "first")
    assert len(want[3]) >= 440 * NG and 0 < sum(want[3].values()) < len(want[3])
    check(64, 1966, 32, 1, MG.random_groups(rng, NG, 64, 1966, full=True), tdma, "second")


@pytest.mark.parametrize("NG,G", [(1, 3), (5, 9), (67, 9), (67, 2)])
def test_group_counts_and_odd_burst_counts(NG, G):
    rng = np.random.default_rng(100 * NG + G)
    arrays = MG.random_groups(rng, NG, G, 1966)
    if NG > 1:
        nb = arrays[0]
        assert (nb == 0).any() and (nb < 0).any(), np.unique(nb)   # (counts above MAXB: the full tables' test)
    out, want, tdma = check(G, 1966, 32, G * 1966 - 1080, arrays, None, "first")
    rows = list(want[2].values())
    if NG > 1:   # the inputs hold what they are meant to
        assert any(r[3] == 1 for r in rows) and any(r[3] == 3 for r in rows) and [0, 0, 0, 0] in rows
        assert any(r[3] == 0 and r[0] for r in rows) and 0 in want[3].values()
    check(G, 1966, 32, G * 1966 - 1080, MG.random_groups(rng, NG, G, 1966), tdma, "a carried tail")


def test_refused_shapes_write_nothing():
    rng = np.random.default_rng(4)
    arrays = MG.random_groups(rng, 2, 3, 1966)
    for G, row_bits, tol in ((0, 1966, 32), (65, 1966, 32), (4, 1966, 32), (5, 1966, 32), (3, -1, 32), (3, 1966, -1)):
        tdma = M.tdma_array([MG.GroupTdma(7, 8, 9, 1) for _ in range(2)])
        rc, out = call_groups(G, row_bits, tol, 100, arrays, tdma, rc_only=True)
        assert rc == -1, (G, row_bits, tol, rc)
        assert all(np.all(v == U) for v in out), (G, row_bits, tol)
        assert tdma.tolist() == [(7, 8, 9, 1)] * 2
    rc, out = call_groups(3, 1966, 32, 100, arrays, M.tdma_array([MG.GroupTdma(), MG.GroupTdma()]), rc_only=True)
    assert rc == 0 and not np.all(out[2] == U)


def _lower_mac_case(rng, C):
    """C rows of hand-made lower-MAC outputs with every PDU kind in their blocks
    (test_gpu_etsi_mac.random_case), the bursts moved onto ascending starts a slot or more apart."""
    import test_gpu_etsi_mac as T
    nsym, nburst, bursts, nblock, blocks, type1 = T.random_case(rng, C, (0, 16) if C > 1 else (16,))
    for c in range(C):
        at = int(rng.integers(0, 200))
        for b in range(int(nburst[c])):
            bursts[c, b, 0] = at
            at += 510 * int(rng.choice((1, 1, 2))) + int(rng.choice((0, 0, 2, -4, 5, -100)))
    return nburst, bursts, nblock, blocks, type1


def test_one_row_groups_equal_tetra_etsi_mac():
    """G = 1, row_bits = 0, the same nsym on every row: slots, npdu, pdus and tdma are tetra_etsi_mac's
    over two chunks (the second on the carried timebases); the PDU walk holds every kind."""
    import test_gpu_etsi_mac as T
    rng = np.random.default_rng(6)
    C, nsym = 70, 5000
    ta = M.tdma_array([M.Tdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(C)])
    tb = ta.copy()
    for k in range(2):
        arrays = _lower_mac_case(rng, C)
        a = T.call_mac(np.full(C, nsym, np.int32), *arrays, ta)
        out, want, tb = check(1, 0, 32, 2 * (nsym - 1), arrays, tb, "chunk %d" % k)
        live = np.arange(M.MAXB)[None, :] < np.clip(arrays[0], 0, M.MAXB)[:, None]
        assert np.array_equal(a[0], out[0]) and np.array_equal(a[1], out[1]), k
        assert np.array_equal(a[2][live], out[2][live]) and ta.tolist() == tb.tolist(), k
        assert np.all(out[3][live] == 1)
    assert {r[0] for recs in want[1].values() for r in recs} == set(range(9))
    assert max(len(r) for r in want[1].values()) > M.MAXPDU


def test_device_pointers_equal_host_pointers():
    import torch
    from tetraear import _hip
    rng = np.random.default_rng(8)
    G, NG = 9, 40
    arrays = list(_lower_mac_case(rng, NG * G))
    arrays[1][..., 0] = MG.random_groups(rng, NG, G, 1966, full=True)[1][..., 0]   # overlapping rows' start bits
    state = M.tdma_array([MG.GroupTdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(NG)])
    th = state.copy()
    host, want, th = check(G, 1966, 32, 12345, arrays, th, "host")
    C = NG * G
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in arrays]
    td = torch.from_numpy(state.view(np.int64).reshape(NG, 3).copy()).cuda()
    outs = [torch.from_numpy(v).cuda() for v in _outputs(C)]
    nsym = torch.zeros(C, dtype=torch.int32, device="cuda")
    c = _hip.ctx()
    c.check(c.lib.tetra_etsi_mac_groups(c.handle, _hip.ptr(nsym), C, G, 1966, 32, 12345, *[_hip.ptr(v) for v in dev],
                                        _hip.ptr(td), *[_hip.ptr(v) for v in outs]), "tetra_etsi_mac_groups")
    keep, slots, npdu, pdus = (v.cpu().numpy() for v in outs)
    for name, x, y in zip(("npdu", "pdus", "slots", "keep"), host, (npdu, pdus, slots, keep)):
        assert np.array_equal(x, y), name
    assert td.cpu().numpy().view(M.TDMA_DTYPE).reshape(NG).tolist() == th.tolist()


def test_seeded_sweep():
    """A few hundred groups over seeds: group counts, G, row spacing, tolerance, the carried state."""
    groups = 0
    for seed in range(24 * SCALE):
        rng = np.random.default_rng(7000 + seed)
        G = int(rng.choice((1, 2, 3, 8, 9, 10, 33, 64)))
        NG = int(rng.choice((1, 2, 7, 16, 31)))
        row_bits, tol = int(rng.choice((1966, 1966, 510, 0, 1 << 33))), int(rng.choice((32, 32, 0, 3, 511)))
        tdma = M.tdma_array([MG.GroupTdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(NG)])
        gen_bits = min(row_bits, 1966)
        _, _, tdma = check(G, row_bits, tol, G * gen_bits - int(rng.integers(0, 1500)),
                           MG.random_groups(rng, NG, G, gen_bits, full=bool(seed % 3 == 0)), tdma, "seed %d, call 0" % seed)
        check(G, row_bits, tol, 0, MG.random_groups(rng, NG, G, gen_bits), tdma, "seed %d, call 1" % seed)
        groups += NG
    assert groups >= 200
