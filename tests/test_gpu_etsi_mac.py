"""tetra_etsi_mac (k_etsi_mac) on the GPU against tests/_etsi_mac_model.py: npdu everywhere, every live
PDU record and every live slot row, and the carried timebase -- integers, compared exactly.

  * direct calls on hand-made bursts / blocks / type1 with everything past the counts and past a
    block's n1 poisoned, at C = 1 and C = 70 (17 full waves of 4 channels and a partial one);
  * the timebase's edges over chunks with a carried tetra_etsi_tdma;
  * built rows through tetra_lmac_etsi_stream (cell acquisition) and then tetra_etsi_mac, with host
    and with device pointers, against the model run on LmacStreamModel's outputs;
  * a seeded sweep; the Python surface (EtsiLowerMac(mac=True), and mac=False unchanged).
tests/test_etsi_mac_model.py checks the model itself on the CPU.
"""
import functools
import os

import numpy as np
import pytest

import etsi as E
import _lmac_rows as R
import _etsi_mac_model as M

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("TETRA_FUZZ_SCALE", "1")))
POISON_KIND, POISON_BYTE, UNWRITTEN = 99, 0x7e, -77
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 9, 15, 20, 30, 33, 34, 35, 61, 62, 63)


# ------------------------------------------------------------------------------ the library's call

def call_mac(nsym, nburst, bursts, nblock, blocks, type1, tdma):
    """tetra_etsi_mac on host arrays; tdma (TDMA_DTYPE array) is updated in place.  The outputs
    start as UNWRITTEN, so what the call leaves alone shows."""
    from tetraear import _hip
    c = _hip.ctx()
    C = len(nsym)
    a = [np.ascontiguousarray(v, np.int32) for v in (nsym, nburst, bursts, nblock, blocks)]
    slots = np.full((C, M.MAXB, 4), UNWRITTEN, np.int32)
    npdu = np.full((C, M.MAXJ), UNWRITTEN, np.int32)
    pdus = np.full((C, M.MAXJ, M.MAXPDU, M.NF), UNWRITTEN, np.int32)
    c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(a[0]), C, _hip.ptr(a[1]), _hip.ptr(a[2]), _hip.ptr(a[3]),
                                 _hip.ptr(a[4]), _hip.ptr(np.ascontiguousarray(type1, np.uint8)), _hip.ptr(tdma),
                                 _hip.ptr(slots), _hip.ptr(npdu), _hip.ptr(pdus)), "tetra_etsi_mac")
    return npdu, pdus, slots


def assert_untouched(out, want, nburst):
    """Records past npdu (and MAXPDU) and slot rows past nburst still hold what the caller put there."""
    npdu, pdus, slots = out
    live = np.arange(M.MAXPDU)[None, None, :] < np.minimum(want[0], M.MAXPDU)[:, :, None]
    assert np.all(pdus[~live] == UNWRITTEN)
    rows = np.arange(M.MAXB)[None, :] < np.clip(np.asarray(nburst), 0, M.MAXB)[:, None]
    assert np.all(slots[~rows] == UNWRITTEN)


# ------------------------------------------------------------------------------ hand-made inputs

def random_pdu(rng):
    pick = int(rng.integers(0, 10))
    L = int(rng.choice(LENGTHS))
    if pick < 4:
        at = int(rng.integers(0, 8))
        if at == 0:
            return M.null_pdu(*rng.integers(0, 2, 2).tolist(), enc=int(rng.integers(0, 4)), length=L)
        return M.resource(rng, L, at, int(rng.integers(0, 1 << 24)), int(rng.integers(0, 64)),
                          *rng.integers(0, 2, 2).tolist(), nbits=None if 2 <= L <= 34 else int(rng.integers(16, 200)))
    if pick < 7:
        return M.mac_end(rng, L, *rng.integers(0, 2, 2).tolist(), nbits=None if 2 <= L <= 34 else 40)
    if pick == 7:
        return M.mac_frag(rng, int(rng.integers(16, 200)), int(rng.integers(0, 2)))
    if pick == 8:
        return M.sysinfo(M.random_fields(rng, M.SYSINFO_LAYOUT))
    return M.broadcast(rng, int(rng.integers(1, 4)), 60) if rng.integers(0, 2) else M.supplementary(rng, 60)


def random_block(rng, kind, slot=None):
    """Type-1 bits of one block: a SYNC PDU (of slot count `slot`, or any fields), a run of valid and
    malformed PDUs, or uniform random bits."""
    if rng.integers(0, 4) == 0:
        return rng.integers(0, 2, M.N1[kind]).astype(np.uint8)
    if kind == 2:
        f = M.random_fields(rng, M.SYNC_LAYOUT) if slot is None else M.sync_for_slot(rng, slot)
        return M.block(rng, 2, [M.sync(f)])
    short = []   # a quarter start with a run of short associated PDUs: more than MAXPDU in a block
    if rng.integers(0, 4) == 0:
        short = [M.mac_end(rng, int(rng.integers(2, 4))) if rng.integers(0, 2) else
                 M.resource(rng, int(rng.integers(4, 6)), 2, aux=int(rng.integers(0, 1024)))
                 for _ in range(int(rng.integers(3, 17)))]
    return M.block(rng, kind, short + [random_pdu(rng) for _ in range(int(rng.integers(1, 18)))])


def random_case(rng, C, force=()):
    """C channels of hand-made lower-MAC outputs, poisoned past the counts and past n1; bursts mostly
    510 bits apart with true slot counts in their SYNC PDUs, some off the grid.  force: nblock values
    the first channels must have (0 -> no burst, 16 -> eight two-block bursts)."""
    nsym = rng.integers(0, 2100, C).astype(np.int32)
    nburst = np.zeros(C, np.int32)
    nblock = np.zeros(C, np.int32)
    bursts = np.full((C, M.MAXB, 2), POISON_KIND, np.int32)
    blocks = np.full((C, M.MAXJ, 4), POISON_KIND, np.int32)
    type1 = np.full((C, M.MAXJ, 268), POISON_BYTE, np.uint8)
    for c in range(C):
        nb = int(rng.integers(0, M.MAXB + 1))
        kinds = rng.integers(0, 3, nb).tolist()
        if c < len(force):
            nb = 0 if force[c] == 0 else 8
            kinds = rng.integers(1, 3, nb).tolist()
        at, slot, j = int(rng.integers(-509, 400)), int(rng.integers(0, M.TDMA_SLOTS)), 0
        for b, bk in enumerate(kinds):
            bursts[c, b] = (at, bk)
            for i, k in enumerate(((0,), (1, 1), (2, 1))[bk]):
                blocks[c, j] = (k, int(rng.integers(0, 4) != 0), b, i)
                t = random_block(rng, k, slot if rng.integers(0, 8) else None)
                type1[c, j, :len(t)] = t | (rng.integers(0, 128, len(t)).astype(np.uint8) << 1)   # a bit is byte & 1
                j += 1
            step = int(rng.choice((1, 1, 1, 1, 2, 3)))
            at += 510 * step + int(rng.choice((0, 0, 0, 0, 1, -2, 4, -4, 5, -5, 100)))
            slot = (slot + step) % M.TDMA_SLOTS
        nburst[c], nblock[c] = nb, j
    return nsym, nburst, bursts, nblock, blocks, type1


def check_case(case, tdma=None, what=""):
    C = len(case[0])
    models = [M.Tdma(*s) for s in tdma.tolist()] if tdma is not None else [M.Tdma() for _ in range(C)]
    tdma = M.tdma_array(models)
    want = M.run(*case, models)
    out = call_mac(*case, tdma)
    M.assert_equal(out, want, what)
    assert_untouched(out, want, case[1])
    assert tdma.tolist() == M.tdma_array(models).tolist(), what
    return out, want


@pytest.mark.parametrize("C", [1, 70])
def test_direct_calls_on_hand_made_inputs(C):
    rng = np.random.default_rng(C)
    force = (16,) if C == 1 else (0, 16, 16, 0)
    case = random_case(rng, C, force)
    assert [int(v) for v in case[3][:len(force)]] == list(force)
    out, want = check_case(case, what="C=%d" % C)
    if C == 70:   # the case holds what it is meant to: every kind, blocks over MAXPDU, bad and good ones
        kinds = {r[0] for recs in want[1].values() for r in recs}
        assert kinds == set(range(9)), kinds
        assert max(len(r) for r in want[1].values()) > M.MAXPDU
        assert any(r[3] for recs in want[1].values() for r in recs)
        assert any(row[3] & 2 for row in want[2].values()) and any(row == [0, 0, 0, 0] for row in want[2].values())
        # a second chunk on the carried timebases, the first chunk's inputs poisoned differently
        tdma = M.tdma_array([M.Tdma() for _ in range(C)])
        call_mac(*case, tdma)
        check_case(random_case(rng, C), tdma, "second chunk")


def test_crc_bad_and_dead_blocks_count_zero():
    rng = np.random.default_rng(3)
    nsym, nburst, bursts, nblock, blocks, type1 = random_case(rng, 9)
    blocks[:, :, 1] = np.where(blocks[:, :, 1] == POISON_KIND, POISON_KIND, 0)   # every live block CRC-bad
    out, want = check_case((nsym, nburst, bursts, nblock, blocks, type1))
    assert not out[0].any() and not want[1]
    assert all(row == [0, 0, 0, 0] for row in want[2].values())   # no SYNC: no timebase


# ------------------------------------------------------------------------------ timebase edges

def _sb(rng, start, slot, **over):
    return (start, 2, M.block(rng, 2, [M.sync(M.sync_for_slot(rng, slot, **over))]))


def _scenarios():
    """(name, initial state, chunks [(nsym, [(start, kind, BSCH type-1 or None)])], final check)."""
    rng = np.random.default_rng(11)
    G = 510
    lock = (0, 1000, 10, 1)
    out = [
        ("wrap and a missed burst", (0, 0, 0, 0),
         [(1001, [(100, 0, None), _sb(rng, 610, 4318), (1120, 0, None), (1630, 1, None)]),
          (501, [(1630 + 2 * G - 2000, 0, None)])], (3000, 2650, 2, 1)),
        ("k = 71 taken", lock, [(0, []), (50, [(1000 + 71 * G, 0, None)])], (98, 1000 + 71 * G, 81, 1)),
        ("k = 72 drops the lock", lock, [(50, [(1000 + 72 * G, 0, None)]), (50, [(1000 + 73 * G - 98, 0, None)])],
         (196, 1000, 10, 0)),
        ("d < 0 drops the lock", lock, [(50, [(999, 0, None)])], (98, 1000, 10, 0)),
        ("a contradicting SB wins", lock,
         [(2001, [_sb(rng, 1510, 11), _sb(rng, 2020, 500), (2530, 0, None), _sb(rng, 3045, 7)])], (4000, 3045, 7, 1)),
        ("bit0 at 2^40, a burst from the carried tail", (1 << 40, 0, 0, 0),
         [(1001, [_sb(rng, -300, 8), (210, 0, None)]), (1, []), (256, [(-2000 + 210 + 3 * G, 1, None)])],
         ((1 << 40) + 2510, (1 << 40) + 210 + 3 * G, 12, 1)),
    ]
    for r in (4, -4):
        out.append(("r = %d taken" % r, lock, [(300, [(1510 + r, 0, None)])], (598, 1510 + r, 11, 1)))
    for r in (5, -5):
        out.append(("r = %d refused, anchor kept" % r, lock, [(300, [(1510 + r, 0, None)]), (300, [(2020 - 598, 0, None)])],
                    (1196, 2020, 12, 1)))
    for over in (dict(fn=0), dict(fn=19), dict(mn=0), dict(mn=61)):
        out.append(("SB with %r is no anchor" % over, (0, 0, 0, 0),
                    [(600, [_sb(rng, 10, 200, **over), (520, 0, None)])], (1198, 0, 0, 0)))
    return out


def test_timebase_edges():
    """One scenario per channel, chunk k of every scenario in call k, the tdma array carried."""
    sc = _scenarios()
    C, nchunk = len(sc), max(len(s[2]) for s in sc)
    models = [M.Tdma(*s[1]) for s in sc]
    tdma = M.tdma_array(models)
    rows_seen = {}
    for k in range(nchunk):
        nsym = np.zeros(C, np.int32)
        nburst, nblock = np.zeros(C, np.int32), np.zeros(C, np.int32)
        bursts = np.full((C, M.MAXB, 2), POISON_KIND, np.int32)
        blocks = np.full((C, M.MAXJ, 4), POISON_KIND, np.int32)
        type1 = np.full((C, M.MAXJ, 268), POISON_BYTE, np.uint8)
        for c, s in enumerate(sc):
            if k >= len(s[2]):
                continue
            nsym[c], bl = s[2][k]
            j = 0
            for b, (start, kind, t) in enumerate(bl):
                bursts[c, b] = (start, kind)
                for i, bk in enumerate(((0,), (1, 1), (2, 1))[kind]):
                    blocks[c, j] = (bk, int(bk == 2), b, i)   # only the BSCH blocks are CRC-good
                    if bk == 2:
                        type1[c, j, :60] = t
                    j += 1
            nburst[c], nblock[c] = len(bl), j
        case = (nsym, nburst, bursts, nblock, blocks, type1)
        want = M.run(*case, models)
        out = call_mac(*case, tdma)
        M.assert_equal(out, want, "chunk %d" % k)
        assert tdma.tolist() == M.tdma_array(models).tolist(), k
        rows_seen.update({(c, k, b): (row, want[1].get((c, 0))) for (c, b), row in want[2].items()})
    for c, s in enumerate(sc):
        assert tuple(tdma[c].tolist()) == s[3], (s[0], tdma[c])
    name = {s[0]: c for c, s in enumerate(sc)}
    c = name["wrap and a missed burst"]
    assert [rows_seen[(c, 0, b)][0] for b in range(4)] == [[0, 0, 0, 0], [3, 18, 60, 1], [4, 18, 60, 0], [1, 1, 1, 0]]
    assert rows_seen[(c, 1, 0)][0] == [3, 1, 1, 0]
    c = name["a contradicting SB wins"]
    assert [rows_seen[(c, 0, b)][0] for b in range(4)] == [[4, 3, 1, 1], [1, 18, 7, 3], [2, 18, 7, 0], [4, 2, 1, 3]]
    for over in ("fn", "mn"):
        for c in [v for n, v in name.items() if n.startswith("SB with {'%s'" % over)]:
            row, recs = rows_seen[(c, 0, 0)]
            assert row == [0, 0, 0, 0] and recs[0][0] == M.SYNC and recs[0][3] == 1
            assert rows_seen[(c, 0, 1)][0] == [0, 0, 0, 0]
    assert rows_seen[(name["r = 5 refused, anchor kept"], 0, 0)][0] == [0, 0, 0, 0]
    assert rows_seen[(name["r = 5 refused, anchor kept"], 1, 0)][0] == [1, 4, 1, 0]
    assert rows_seen[(name["k = 71 taken"], 1, 0)][0] == [2, 3, 2, 0]


# ------------------------------------------------------------------------------ through the pipeline

SMAX = 2048


@functools.lru_cache(maxsize=None)
def _pipeline_channels():
    """Rows of consecutive bursts (consecutive slots) whose payloads come from the builders: SBs carry
    the true TN/FN/MN and the cell, one SB is the row's second burst.  Half the rows are cut into
    random chunks, half inside bursts.  Returns [(hard, soft, cuts)], [[(start, kind, slot)]] and the
    planted PDU kinds per burst."""
    chans, planted_all = [], []
    for i in range(6):
        rng = np.random.default_rng(500 + i)
        init, cell = R.cell_fields(rng)
        slot0 = (4310, 17, 2000, 4319, 71, 1234)[i]
        kinds = [int(rng.integers(0, 2)), 2] + rng.integers(0, 3, 8).tolist()
        items = []
        for b, bk in enumerate(kinds):
            slot = (slot0 + b) % M.TDMA_SLOTS
            if bk == 2:
                pay = [M.block(rng, 2, [M.sync(M.sync_for_slot(rng, slot, cell))]),
                       M.block(rng, 1, [M.sysinfo(M.random_fields(rng, M.SYSINFO_LAYOUT))])]
            else:
                pay = [M.block(rng, k, [random_pdu(rng) for _ in range(int(rng.integers(1, 8)))])
                       for k in ((0,), (1, 1))[bk]]
            items.append((7 + i if b == 0 else 0, bk, init, pay))
        bits, planted, _ = R.place_bursts(rng, items, tail_gap=2 * i)
        hard = R.hard_of(bits)
        if i % 2:
            cuts = R.chunk_cuts(i, len(hard), (255, 256, 257, 700, 1500, 1790))
        else:
            cuts = R.cuts_at(len(hard), [(s + (6, 250, 100, 400, 505)[(i + j) % 5]) // 2
                                         for j, (s, _) in enumerate(planted)])
        assert max(n for _, n in cuts) + E.RESERVE <= SMAX - 1
        chans.append((hard, R.soft_of(bits), cuts))
        planted_all.append([(s, k, (slot0 + b) % M.TDMA_SLOTS) for b, (s, k) in enumerate(planted)])
    return chans, planted_all


def _model_arrays(results):
    """LmacStreamModel push results of one chunk, one per channel, in the library's output layout."""
    C = len(results)
    nburst, nblock = np.zeros(C, np.int32), np.zeros(C, np.int32)
    bursts = np.zeros((C, M.MAXB, 2), np.int32)
    blocks = np.zeros((C, M.MAXJ, 4), np.int32)
    type1 = np.zeros((C, M.MAXJ, 268), np.uint8)
    for c, r in enumerate(results):
        bu, bl, bits = R.flatten(r["bursts"])
        nburst[c], nblock[c] = len(bu), len(bl)
        for b, v in enumerate(bu):
            bursts[c, b] = v
        for j, (v, t) in enumerate(zip(bl, bits)):
            blocks[c, j] = v
            type1[c, j, :len(t)] = t
    return nburst, bursts, nblock, blocks, type1


def _run_pipeline(device):
    """Chunk by chunk: tetra_lmac_etsi_stream with cell acquisition, then tetra_etsi_mac on its
    outputs, on host arrays or (device) on torch tensors with nothing in between.  Returns per chunk
    (nsym, nburst, bursts, npdu, pdus, slots, tdma) as numpy arrays."""
    from tetraear import _hip
    c = _hip.ctx()
    chans, _ = _pipeline_channels()
    C, RES = len(chans), _hip.ETSI_RESERVE
    if device:
        import torch

        def arr(shape, dtype, fill=0):
            return torch.full(shape, fill, dtype=getattr(torch, dtype), device="cuda")
    else:
        def arr(shape, dtype, fill=0):
            return np.full(shape, fill, getattr(np, dtype))
    soft, hard = arr((C, 2 * SMAX), "int8"), arr((C, SMAX), "uint8")
    lead, cell_init = arr((C,), "int32", 2 * RES), arr((C,), "int32" if device else "uint32", 3)
    tdma = arr((C, 3), "int64")   # struct tetra_etsi_tdma: 24 bytes, all zero
    res = []
    for k in range(max(len(ch[2]) for ch in chans) + 1):
        nsym_h = np.ones(C, np.int32)
        hnew, snew = np.zeros((C, SMAX - RES), np.uint8), np.zeros((C, 2 * (SMAX - RES)), np.int8)
        for ch, (h, s, cuts) in enumerate(chans):
            at, n = cuts[k] if k < len(cuts) else (len(h), 0)
            hnew[ch, :n], snew[ch, :2 * n] = h[at:at + n], s[2 * at:2 * (at + n)]
            nsym_h[ch] = n + 1
        if device:
            hard[:, RES:], soft[:, 2 * RES:] = torch.from_numpy(hnew).cuda(), torch.from_numpy(snew).cuda()
            nsym = torch.from_numpy(nsym_h).cuda()
        else:
            hard[:, RES:], soft[:, 2 * RES:], nsym = hnew, snew, nsym_h
        nburst, bursts = arr((C,), "int32", UNWRITTEN), arr((C, M.MAXB, 2), "int32", POISON_KIND)
        nblock, blocks = arr((C,), "int32", UNWRITTEN), arr((C, M.MAXJ, 4), "int32", POISON_KIND)
        type1 = arr((C, M.MAXJ, 268), "uint8", POISON_BYTE)
        slots, npdu = arr((C, M.MAXB, 4), "int32", UNWRITTEN), arr((C, M.MAXJ), "int32", UNWRITTEN)
        pdus = arr((C, M.MAXJ, M.MAXPDU, M.NF), "int32", UNWRITTEN)
        p = _hip.ptr
        c.check(c.lib.tetra_lmac_etsi_stream(c.handle, p(soft), p(hard), p(nsym), C, SMAX, p(lead), p(soft), p(hard),
                                             p(cell_init), p(nburst), p(bursts), p(nblock), p(blocks), p(type1)),
                "tetra_lmac_etsi_stream")
        c.check(c.lib.tetra_etsi_mac(c.handle, p(nsym), C, p(nburst), p(bursts), p(nblock), p(blocks), p(type1),
                                     p(tdma), p(slots), p(npdu), p(pdus)), "tetra_etsi_mac")
        res.append([v.cpu().numpy().copy() if device else v.copy()
                    for v in (nsym, nburst, bursts, npdu, pdus, slots, tdma)])
    return res


@functools.lru_cache(maxsize=None)
def _host_pipeline():
    return _run_pipeline(False)


def test_pipeline_on_built_rows():
    chans, planted = _pipeline_channels()
    C = len(chans)
    res = _host_pipeline()
    rx = E.Receiver()
    lmac = [R.LmacStreamModel(rx, None) for _ in chans]
    tdma = [M.Tdma() for _ in chans]
    found, seams = [[] for _ in chans], 0
    for k, (nsym, nburst, bursts, npdu, pdus, slots, td) in enumerate(res):
        pushed = []
        for ch, (h, s, cuts) in enumerate(chans):
            at, n = cuts[k] if k < len(cuts) else (len(h), 0)
            pushed.append(lmac[ch].push(h[at:at + n], s[2 * at:2 * (at + n)]))
            found[ch] += [(2 * at + pos, kind, slots[ch, b].tolist()) for b, (pos, kind, _) in
                          enumerate(pushed[-1]["bursts"])]
        arrays = _model_arrays(pushed)
        assert np.array_equal(nburst, arrays[0])
        for ch in range(C):
            assert np.array_equal(bursts[ch, :nburst[ch]], arrays[1][ch, :nburst[ch]]), (k, ch)
        seams += sum(pos < 0 for r in pushed for pos, _, _ in r["bursts"])
        want = M.run(nsym, *arrays, tdma)
        M.assert_equal((npdu, pdus, slots), want, "chunk %d" % k)
        assert_untouched((npdu, pdus, slots), want, nburst)
        assert td.view(M.TDMA_DTYPE).reshape(C).tolist() == M.tdma_array(tdma).tolist(), k
    for ch, pl in enumerate(planted):   # every burst found once; the planted slot from the first SB on
        assert [(s, k) for s, k, _ in found[ch]] == [(s, k) for s, k, _ in pl]
        first_sb = next(b for b, (_, k, _) in enumerate(pl) if k == 2)
        assert first_sb == 1
        for b, ((_, _, row), (_, bk, slot)) in enumerate(zip(found[ch], pl)):
            if b < first_sb:
                assert row == [0, 0, 0, 0], (ch, b, row)
            else:
                assert row[:3] == [slot % 4 + 1, slot // 4 % 18 + 1, slot // 72 + 1], (ch, b, row, slot)
                assert row[3] == (1 if bk == 2 else 0), (ch, b, row)
    assert seams >= 10, seams   # bursts that began in a carried tail


def test_pipeline_device_pointers_equal_host():
    """The same chain on torch CUDA tensors, tetra_etsi_mac enqueued behind the lower MAC with no
    synchronisation in between: every output equals the host-pointer run's."""
    host, dev = _host_pipeline(), _run_pipeline(True)
    assert len(host) == len(dev)
    for k, (a, b) in enumerate(zip(host, dev)):
        live = np.arange(M.MAXB)[None, :] < a[1][:, None]   # the lower MAC's host staging rewrites the dead rows
        a[2][~live], b[2][~live] = POISON_KIND, POISON_KIND
        for name, x, y in zip(("nsym", "nburst", "bursts", "npdu", "pdus", "slots", "tdma"), a, b):
            assert np.array_equal(x, y), (k, name)


# ------------------------------------------------------------------------------ sweep

def test_seeded_sweep():
    for seed in range(40 * SCALE):
        rng = np.random.default_rng(9000 + seed)
        C = int(rng.choice((1, 2, 3, 4, 5, 7, 16, 17, 33)))
        tdma = M.tdma_array([M.Tdma(int(rng.integers(0, 1 << 45)), 0, 0, 0) for _ in range(C)])
        case = random_case(rng, C)
        check_case(case, tdma, "seed %d, chunk 0" % seed)
        call_mac(*case, tdma)
        check_case(random_case(rng, C), tdma, "seed %d, chunk 1" % seed)


# ------------------------------------------------------------------------------ Python surface

def _decode_stream(lm):
    chans, _ = _pipeline_channels()
    C = len(chans)
    frames = [[] for _ in chans]
    for k in range(max(len(ch[2]) for ch in chans) + 1):   # one more: an empty chunk
        n = [ch[2][k][1] if k < len(ch[2]) else 0 for ch in chans]
        smax = max(max(n), 1) + 2
        hard, soft, nsym = np.zeros((C, smax), np.uint8), np.zeros((C, 2 * smax), np.int8), np.ones(C, np.int32)
        for ch, (h, s, cuts) in enumerate(chans):
            at = cuts[k][0] if k < len(cuts) else len(h)
            hard[ch, :n[ch]], soft[ch, :2 * n[ch]], nsym[ch] = h[at:at + n[ch]], s[2 * at:2 * (at + n[ch])], n[ch] + 1
        for ch, fr in enumerate(lm.decode_stream(soft, hard, nsym)):
            frames[ch] += fr
    return frames


def test_python_frames_carry_the_timebase_and_pdus():
    from tetraear.core.etsi import EtsiLowerMac
    _, planted = _pipeline_channels()
    frames = _decode_stream(EtsiLowerMac(mac=True))
    for ch, pl in enumerate(planted):
        assert len(frames[ch]) == len(pl)
        for b, (f, (_, bk, slot)) in enumerate(zip(frames[ch], pl)):
            want = (None, None, None) if b == 0 else (slot % 4 + 1, slot // 4 % 18 + 1, slot // 72 + 1)
            assert (f["tn"], f["fn"], f["mn"]) == want and f["slot_flags"] == (1 if bk == 2 and b else 0)
            assert "timeslot" in f and (f["crc_ok"] or b == 0)   # burst 0 may come before the cell is known
            for blk in f["blocks"]:
                if not blk["crc_ok"]:
                    assert blk["npdu"] == 0 and blk["pdus"] == []
                    continue
                recs = M.walk(blk["bits"], {"SCH/F": 0, "SCH/HD": 1, "BSCH": 2}[blk["channel"]])
                assert blk["npdu"] == len(recs) and len(blk["pdus"]) == min(len(recs), M.MAXPDU)
                for d, r in zip(blk["pdus"], recs):
                    assert (d["kind"], d["offset"], d["nbits"], d["ok"]) == (M.KIND_NAMES[r[0]], r[1], r[2], r[3] == 0)
                    if r[0] == M.SYNC:
                        assert (d["tn"], d["fn"], d["mn"]) == (slot % 4, slot // 4 % 18 + 1, slot // 72 + 1)
                    if r[0] == M.SYSINFO and r[3] == 0:
                        assert d["downlink_hz"] == r[5] * 100e6 + r[4] * 25e3 + {0: 0, 1: 6250, 2: -6250, 3: 12500}[r[6]]
                    if r[0] == M.RESOURCE:
                        assert (d["ssi"], d["aux"]) == (None if r[8] < 0 else r[8], None if r[9] < 0 else r[9])


def test_python_frames_without_mac_are_unchanged():
    from tetraear.core.etsi import EtsiLowerMac
    frames = _decode_stream(EtsiLowerMac())
    assert sum(len(f) for f in frames) == 60
    for fr in frames:
        for f in fr:
            assert set(f) == {"position", "burst", "burst_kind", "timeslot", "blocks", "crc_ok"}
            assert all(set(b) == {"channel", "crc_ok", "bits", "block"} for b in f["blocks"])
