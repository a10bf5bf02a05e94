"""The CPU side of tetra_etsi_assign: the inputs the GPU tests rely on, every branch of
tests/_etsi_assign_model.py reached by hand with its outcome stated, the host's key helpers and the option
rules.  No GPU.

Passing on the parent commit by design (they check models and inputs only): test_planted_allocations_decode_
through_the_oracle, and every test_model_* below -- they use nothing the feature adds.  Failing there: the key
helpers, chain_options(follow=True), the header / binding test.
"""
import os
import re

import numpy as np
import pytest

import etsi as E
import _lmac_rows as R
import _etsi_mac_model as M
import _etsi_sdu_cases as K
import _etsi_sdu_model as S
import _etsi_assign_cases as AC
import _etsi_assign_model as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SB = 0, 2   # burst kinds
CTRL, FULL, HALF, LOST, NONE = A.TCH_CONTROL, A.TCH_FULL, A.TCH_HALF, A.TCH_LOST, A.TCH_NONE
OWN = AC.key_of(100)   # the carrier most cases run on: carrier number 100, no offset


def _rng(seed):
    return np.random.default_rng(seed)


def null(rng=None):
    return [[M.null_pdu()]]


def burst(slot, blocks, cls=CTRL, kind=N, jitter=0, fn=None):
    """A burst on slot `slot` of the carrier's grid: TN = slot % 4 + 1, FN = (slot // 4) % 18 + 1."""
    tn, f = AC.grid(slot * AC.SLOT)[:2]
    return (slot * AC.SLOT + jitter, kind, blocks, cls, (tn, f if fn is None else fn))


def states(n=1):
    return [A.State() for _ in range(n)]


# ------------------------------------------------------------------------------ the inputs

def test_planted_allocations_decode_through_the_oracle():
    """Bursts built from resource_pdu / end_pdu with a channel allocation element, decoded by the oracle's lower
    MAC and walked by the MAC and SDU models, hand the planted fields back with ELEMS bit 2 (and 3): what the GPU
    chain tests plant is what the chain reads.  (Passes on the parent commit by design.)"""
    rng = _rng(11)
    init, cell = R.cell_fields(rng)
    ca1 = AC.alloc(1201, 0b0010, updown=1)
    ca2 = AC.alloc(77, 0b1001, updown=3, ext=(4, 2), allocation_type=2, mon=0)
    first = K.first(K.payload(rng, K.FIRST_CAP), ssi=0x31337)
    pays = [[M.block(rng, 2, [M.sync(M.sync_for_slot(rng, 9, cell))]), M.block(rng, 1, [M.null_pdu()])],
            [M.block(rng, 0, AC.resource_alloc(rng, ca1, ssi=0xBEEF03, addr_type=6, aux=41))],
            [M.block(rng, 0, first)],
            [M.block(rng, 0, AC.end_alloc(rng, ca2, K.payload(rng, 50)))]]
    kinds = [R.SB, R.NDB_N, R.NDB_N, R.NDB_N]
    bits, planted, _ = R.place_bursts(rng, [(5 if i == 0 else 0, k, init, [p.copy() for p in pay])
                                            for i, (k, pay) in enumerate(zip(kinds, pays))])
    dec = E.Receiver().lower_mac(R.soft_of(bits), R.hard_of(bits), init)
    assert [(s, k) for s, k, _ in dec] == planted and all(ok for _, _, blocks in dec for _, _, ok in blocks)
    for b, (ca, pk) in ((1, (ca1, M.RESOURCE)), (3, (ca2, M.END))):
        k, t1, _ = dec[b][2][0]
        rec = M.walk(t1, k)[0]
        assert rec[0] == pk and rec[3] == 0
        s, _ = S.sdu_of([int(v) & 1 for v in t1[:M.N1[k]]], rec)
        assert s[S.STATUS] == S.OK and s[S.ELEMS] & 4 and bool(s[S.ELEMS] & 8) == (ca["extended"] is not None)
        head = s[S.CHAN] & 0x3FF
        assert (head >> 8, (head >> 4) & 15, (head >> 2) & 3) == (ca["allocation_type"], ca["timeslot_assigned"],
                                                                 ca["updownlink_assigned"])
        assert (s[S.CHAN] >> 16) & 0xFFF == ca["carrier"]
        if ca["extended"]:
            x = (s[S.POWER_GRANT] >> 16) & 0x3FF
            assert (x >> 6, (x >> 4) & 3, (x >> 1) & 7, x & 1) == (4, 2, 5, 1)
    k, t1, _ = dec[1][2][0]
    assert M.walk(t1, k)[0][7:10] == [6, 0xBEEF03, 41]


# ------------------------------------------------------------------------------ the carrier numbering

@pytest.mark.parametrize("off", [0, 1, 2, -1])
def test_model_target_keys_inherit_band_and_offset(off):
    """Not extended: band and offset are the sender's, whatever its two low bits (0, 1, 2, 3)."""
    own = AC.key_of(100, off)
    assert own & 3 == {0: 0, 1: 1, 2: 2, -1: 3}[off]
    assert A.target_key(1201, -1, own) == 4 * 16000 + 4 * 1201 + off
    assert A.target_key(0, -1, own) == 4 * 16000 + off
    assert A.target_key(1201, -1, AC.key_of(100, off, band=8)) == 8 * 16000 + 4 * 1201 + off


def test_model_target_keys_extended_and_unknown():
    """Extended: band and offset are the element's (0, +1, -1, +2 for the field's 0..3), the sender's key is not
    read; not extended from an unknown carrier: -1."""
    for field, d in ((0, 0), (1, 1), (2, -1), (3, 2)):
        ext = 3 << 6 | field << 4 | 0b1011
        assert A.target_key(500, ext, -1) == A.target_key(500, ext, AC.key_of(9, 1)) == 3 * 16000 + 2000 + d
    assert A.target_key(500, -1, -1) == -1 and A.target_key(500, -1, -7) == -1
    assert A.target_key(0, 2 << 4, OWN) == -1   # band 0, carrier 0, offset -6.25 kHz: no key, never a target


# ------------------------------------------------------------------------------ the walk, branch by branch

def test_model_event_record_and_equal_time():
    """A carrier allocates its own timeslot 3 in a burst on timeslot 3: the event record holds the planted fields;
    that burst itself reads STATE 0 (a burst at p <= T comes first), the next burst of the timeslot reads 1 with
    AGE 4, NALLOC 1, and the other timeslots stay 0."""
    rng = _rng(1)
    ca = AC.alloc(100, 0b0010)
    rows = [[burst(2, [AC.resource_alloc(rng, ca, ssi=0x123, addr_type=6, aux=9)]), burst(3, null()), burst(6, null()),
             burst(10, null(), jitter=3)]]
    call = AC.rows_call(rng, rows, bit0s=[(1 << 33) + 510 * 8])
    st = [A.State((1 << 33) + 510 * 8)]
    nev, ev, ta = AC.run_model(call, st, np.array([OWN], np.int32))
    p = (1 << 33) + 510 * 8 + 2 * 510
    assert nev.tolist() == [1]
    assert ev[(0, 0)] == [0, 0, 0, 0, M.RESOURCE, 0b0010 << 4 | 1 << 2, 100, -1, OWN, A.low32(p), 2, 3, 1, 0x123, 6, 9]
    assert ta[(0, 0)] == A.INACTIVE and ta[(0, 1)] == A.INACTIVE
    assert ta[(0, 2)] == [1, 0x123, 6, 9, OWN, 1, 0, 4]
    assert ta[(0, 3)] == [1, 0x123, 6, 9, OWN, 1, 1, 8]   # the control burst on slot 6 counted as idle
    e = st[0].slot[2]
    assert (e.active, e.since, e.last, e.nalloc, e.idle) == (1, p, p, 1, 2) and st[0].bit0 == (1 << 33) + 510 * 8 + 72 * 4 * 510


def test_model_uplink_only_and_empty_bitmap_are_ignored_and_two_bits_set_two():
    """Up/downlink 2 (uplink only) and a bitmap of 0 are listed and apply nowhere; a bitmap of 0b1001 sets
    timeslots 1 and 4; up/downlink 3 (both) applies."""
    rng = _rng(2)
    rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b0110, updown=2))]),
             burst(1, [AC.resource_alloc(rng, AC.alloc(100, 0))]),
             burst(2, [AC.resource_alloc(rng, AC.alloc(100, 0b1001, updown=3), ssi=5)])] +
            [burst(4 + i, null()) for i in range(4)]]
    st = states()
    nev, ev, ta = AC.run_model(AC.rows_call(rng, rows), st, np.array([OWN], np.int32))
    assert nev.tolist() == [3] and [ev[(0, k)][A.E_TARGET] for k in range(3)] == [OWN] * 3
    assert [ta[(0, b)][0] for b in range(3, 7)] == [1, 0, 0, 1] and [e.active for e in st[0].slot] == [1, 0, 0, 1]
    assert ta[(0, 3)][A.T_SSI] == 5


def test_model_shared_clock():
    """Carrier A names carrier B's key.  shared_clock 0: listed (TARGET is B's key), nothing assigned.  1: B's
    timeslot 2 reads assigned from the first burst behind the event, SRC_KEY A's key; A itself stays free."""
    rng = _rng(3)
    ka, kb = AC.key_of(100), AC.key_of(131)
    rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(131, 0b0100), ssi=77)]), burst(1, null()), burst(5, null())],
            [burst(1, null(), cls=FULL), burst(5, null(), cls=FULL), burst(6, null())]]
    keys = np.array([ka, kb], np.int32)
    for shared in (0, 1):
        st = states(2)
        nev, ev, ta = AC.run_model(AC.rows_call(_rng(3), rows), st, keys, shared_clock=shared)
        assert nev.tolist() == [1, 0] and ev[(0, 0)][A.E_TARGET] == kb
        assert [ta[(0, b)][0] for b in range(3)] == [0, 0, 0]
        assert [ta[(1, b)][0] for b in range(3)] == ([1, 1, 0] if shared else [0, 0, 0])
        if shared:
            assert ta[(1, 0)] == [1, 77, 1, -1, ka, 1, 0, 1] and st[1].slot[1].last == 5 * 510


def test_model_unknown_target_and_no_keys():
    """A sender without a key: TARGET -1, nothing applies; row_key None: the same for every group."""
    rng = _rng(4)
    rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b1000))]), burst(4, null())]]
    for keys in (np.array([-1], np.int32), None):
        st = states()
        nev, ev, ta = AC.run_model(AC.rows_call(_rng(4), rows), st, keys)
        assert nev.tolist() == [1] and ev[(0, 0)][A.E_TARGET] == -1 and ta[(0, 1)] == A.INACTIVE
    ext = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b1000, ext=(AC.BAND, 0)))]), burst(4, null())]]
    nev, ev, ta = AC.run_model(AC.rows_call(rng, ext), states(), None)
    assert ev[(0, 0)][A.E_TARGET] == OWN and ev[(0, 0)][A.E_EXT] == AC.BAND << 6 | 0b1011 and ta[(0, 1)] == A.INACTIVE


@pytest.mark.parametrize("hold,alive", [(8, True), (7, False)])
def test_model_expiry_at_the_hold_time(hold, alive):
    """Eight slots behind the allocation with nothing in between: hold_slots 8 keeps the entry (8 > 8 is false),
    7 frees it -- expired += 1, the burst reads STATE 0.  Without tq nothing refreshes or releases."""
    rng = _rng(5)
    rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b1000))]), burst(8, null())]]
    st = states()
    _, _, ta = AC.run_model(AC.rows_call(rng, rows), st, np.array([OWN], np.int32), hold_slots=hold, with_tq=False)
    assert ta[(0, 1)][0] == int(alive) and st[0].expired == int(not alive) and st[0].slot[0].active == int(alive)
    assert ta[(0, 1)][A.T_AGE] == (8 if alive else 0)


def test_model_full_refreshes_and_lost_does_not():
    """hold_slots 8: a FULL (or HALF) burst 8 slots behind the allocation moves `last`, so a burst 8 slots on
    still reads assigned; with LOST bursts instead the second one is 16 slots behind `last` and expires."""
    for cls, want in ((FULL, [1, 1]), (HALF, [1, 1]), (LOST, [1, 0])):
        rng = _rng(6)
        rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b1000))]), burst(8, null(), cls=cls),
                 burst(16, null(), cls=cls)]]
        st = states()
        _, _, ta = AC.run_model(AC.rows_call(rng, rows), st, np.array([OWN], np.int32), hold_slots=8)
        assert [ta[(0, 1)][0], ta[(0, 2)][0]] == want and st[0].expired == 1 - want[1]
        assert st[0].slot[0].last == (16 * 510 if cls != LOST else 0)


def test_model_release_after_idle_max_and_frame_18():
    """idle_max 2: decoded control bursts on the timeslot count up; the third frees the entry (released += 1) and
    still reads STATE 1 with IDLE 2; the next reads 0.  A CONTROL burst of frame 18 does not count, a traffic burst
    resets the count."""
    rng = _rng(7)
    alloc_burst = burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b1000))], cls=CTRL)
    seq = [(4, CTRL, None), (8, CTRL, 18), (12, CTRL, None), (16, FULL, None), (20, CTRL, None), (24, CTRL, None),
           ]
    rows = [[alloc_burst] + [burst(s, null(), cls=c, fn=f) for s, c, f in seq]]
    st = states()
    _, _, ta = AC.run_model(AC.rows_call(rng, rows), st, np.array([OWN], np.int32), idle_max=2)
    # the allocation's own burst is handled before the event; idle counts 1 (slot 4), stays (frame 18), 2, reset by FULL
    assert [ta[(0, b)][A.T_IDLE] for b in range(1, 7)] == [0, 1, 1, 2, 0, 1] and st[0].released == 0
    rows = [[alloc_burst] + [burst(4 * i, null()) for i in range(1, 6)]]
    st = states()
    _, _, ta = AC.run_model(AC.rows_call(rng, rows), st, np.array([OWN], np.int32), idle_max=2)
    assert [ta[(0, b)][0] for b in range(1, 6)] == [1, 1, 1, 0, 0] and ta[(0, 3)][A.T_IDLE] == 2
    assert st[0].released == 1 and st[0].expired == 0 and st[0].slot[0].idle == 3


def test_model_mac_end_takes_its_address_from_the_done_record():
    """A MAC-END that completes a chain carries the allocation of the chain's addressee: SSI / ADDR_TYPE / AUX are
    the done record's.  One that no chain awaits (an orphan) reads -1, -1, -1, and still applies."""
    rng = _rng(8)
    ca = AC.alloc(100, 0b0001)
    rows = [[burst(3, [K.first(K.payload(rng, K.FIRST_CAP), ssi=0xCAFE)]), burst(7, [AC.end_alloc(rng, ca, K.payload(rng, 30))]),
             burst(11, null())],
            [burst(3, [AC.end_alloc(rng, ca, K.payload(rng, 30))]), burst(7, null())]]
    st = states(2)
    call = AC.rows_call(rng, rows)
    assert call["ndone"].tolist() == [1, 0]
    nev, ev, ta = AC.run_model(call, st, np.array([OWN, OWN], np.int32))
    assert ev[(0, 0)][A.E_KIND] == M.END and ev[(0, 0)][A.E_SSI:] == [0xCAFE, 1, -1]
    assert ev[(1, 0)][A.E_SSI:] == [-1, -1, -1]
    assert ta[(0, 2)][:4] == [1, 0xCAFE, 1, -1] and ta[(1, 1)][:4] == [1, -1, -1, -1]
    # with maxd 0 the call has no done records to search
    nev, ev, _ = AC.run_model(dict(call, maxd=0), states(2), np.array([OWN, OWN], np.int32))
    assert ev[(0, 0)][A.E_SSI:] == [-1, -1, -1]


def test_model_events_past_maxe_do_not_apply():
    """Three events in a group, maxe 1: nev counts three, one is recorded, and only that one applies."""
    rng = _rng(9)
    rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b1000))]), burst(1, [AC.resource_alloc(rng, AC.alloc(100, 0b0100))]),
             burst(2, [AC.resource_alloc(rng, AC.alloc(100, 0b0010))])] + [burst(4 + i, null()) for i in range(3)]]
    for maxe, want in ((1, [1, 0, 0]), (3, [1, 1, 1]), (0, [0, 0, 0])):
        nev, ev, ta = AC.run_model(AC.rows_call(_rng(9), rows), states(), np.array([OWN], np.int32), maxe=maxe)
        assert nev.tolist() == [3] and sorted(ev) == [(0, k) for k in range(min(maxe, 3))]
        assert [ta[(0, b)][0] for b in range(3, 6)] == want


def test_model_two_sources_one_target_slot():
    """Two carriers allocate timeslot 1 of a third in one call.  At different times the later one's fields stand; at
    equal T the order is (T, source group, ordinal): the higher group's stand.  NALLOC counts both."""
    for slots_ab, winner in (((0, 1), 22), ((1, 0), 11), ((0, 0), 22)):
        rng = _rng(10)
        kt = AC.key_of(140)
        rows = [[burst(slots_ab[0], [AC.resource_alloc(rng, AC.alloc(140, 0b1000), ssi=11)])],
                [burst(slots_ab[1], [AC.resource_alloc(rng, AC.alloc(140, 0b1000), ssi=22)])],
                [burst(4, null(), cls=FULL)]]
        st = states(3)
        _, _, ta = AC.run_model(AC.rows_call(rng, rows), st, np.array([AC.key_of(100), AC.key_of(101), kt], np.int32),
                                shared_clock=1)
        assert ta[(2, 0)][:3] == [1, winner, 1] and ta[(2, 0)][A.T_NALLOC] == 2
        assert ta[(2, 0)][A.T_SRC_KEY] == AC.key_of(100 if winner == 11 else 101)
        assert st[2].slot[0].since == min(slots_ab) * 510 and ta[(2, 0)][A.T_AGE] == 4 - min(slots_ab)


def test_model_bursts_that_take_no_part():
    """A burst without a timeslot, with an invalid tq record, or (grouped) not kept reads STATE -1 and 0s, and
    changes nothing; without slots every burst does, and the events read TN = FN = 0."""
    rng = _rng(12)
    rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b1000))]), burst(4, null(), cls=-1),
             (8 * 510, N, null(), CTRL, (0, 0)), burst(12, null())]]
    st = states()
    call = AC.rows_call(rng, rows)
    _, _, ta = AC.run_model(call, st, np.array([OWN], np.int32), idle_max=0)
    assert ta[(0, 1)] == A.NOT_FOLLOWED and ta[(0, 2)] == A.NOT_FOLLOWED and ta[(0, 3)][0] == 1
    _, ev, ta = AC.run_model(call, states(), np.array([OWN], np.int32), with_slots=False)
    assert all(ta[(0, b)] == A.NOT_FOLLOWED for b in range(4)) and ev[(0, 0)][A.E_TN:A.E_SSI] == [0, 0]
    calls, keys = AC.random_stream(3, 6, 3)
    _, _, ta = AC.run_model(calls[0], states(2), keys)
    keep, nb = calls[0]["keep"], calls[0]["arrays"][0]
    dropped = [(c, b) for c in range(6) for b in range(nb[c]) if keep[c, b] == 0]
    assert dropped and all(ta[cb] == A.NOT_FOLLOWED for cb in dropped)


def test_model_sweep_reaches_the_follower():
    """The seeded sweep the GPU file runs exercises what it should: over its seeds the calls hold events, applied
    allocations, active entries, expiries and releases."""
    seen = dict(events=0, active=0, expired=0, released=0, end=0)
    for seed in range(6):
        calls, keys = AC.random_stream(100 + seed, 7, 1, ncalls=2)
        st = states(7)
        for call in calls:
            nev, ev, ta = AC.run_model(call, st, keys, hold_slots=6, idle_max=1, shared_clock=1)
            seen["events"] += int(nev.sum())
            seen["end"] += sum(r[A.E_KIND] == M.END for r in ev.values())
            seen["active"] += sum(r[0] == 1 for r in ta.values())
        seen["expired"] += sum(s.expired for s in st)
        seen["released"] += sum(s.released for s in st)
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------------------ the host's helpers

def test_key_helpers():
    from tetraear.core.etsi import allocation_key, carrier_key, key_hz
    assert carrier_key(420e6) == 67200 and carrier_key(420_006_250) == 67201 and carrier_key(0) == 0
    assert key_hz(67201) == 420_006_250 and key_hz(-1) is None and key_hz(None) is None
    for bad in (420e6 + 1, 420_003_125, 6250.5, -6250):
        with pytest.raises(ValueError):
            carrier_key(bad)
    rng = _rng(13)
    for _ in range(200):   # the host restatement against the model, every offset and both numberings
        own = int(rng.choice([-1, AC.key_of(int(rng.integers(4000)), int(rng.choice([0, 1, 2, -1])), int(rng.integers(16)))]))
        ext = (int(rng.integers(16)), int(rng.integers(4))) if rng.random() < 0.5 else None
        ca = AC.alloc(int(rng.integers(4096)), 5, ext=ext)
        x = -1 if ext is None else ext[0] << 6 | ext[1] << 4 | 0b1011
        assert allocation_key(ca, own) == A.target_key(ca["carrier"], x, own)
    assert allocation_key({"allocation_type": 0}, OWN) == -1   # the augmented form names no carrier
    assert allocation_key(AC.alloc(1201, 1), None) == -1


def test_chain_options_follow():
    from tetraear.core.etsi import ChainOptions, chain_options
    assert ChainOptions._fields[-1] == "follow" and chain_options(mac=True).follow is False
    assert chain_options(mac=True, sdu=True, follow=True).follow is True
    assert chain_options(mac=True, timebase="vote", sdu=True, follow=True, grouped=True).follow is True
    for kw in (dict(follow=True), dict(mac=True, follow=True), dict(mac=True, sdu=True, follow=True, grouped=True),
               dict(mac=True, timebase=True, follow=True, grouped=True)):
        with pytest.raises(ValueError):
            chain_options(**kw)


def test_frames_gain_the_keys_only_with_follow():
    """build_frames from records: without an Assign the frames are today's key for key; with one every frame
    gains the three keys, an event lands on the frame of its burst with target_hz / target_row."""
    from tetraear import _hip
    from tetraear.core import etsi as CE
    rng = _rng(14)
    rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b0100), ssi=0x77, addr_type=6, aux=5)]), burst(1, null(), cls=FULL)]]
    call = AC.rows_call(rng, rows)
    keys = np.array([OWN], np.int32)
    nev, ev, ta = AC.run_model(call, states(), keys)
    a = call["arrays"]
    lm = CE.LowerMac(a[0], a[1], a[2], a[3], a[4])
    mac = CE.Mac(call["slots"], a[5], a[6])
    eva, taa = A.expected_arrays(nev, ev, ta, np.full((1, 4, 16), -1, np.int32), np.full((1, 8, 8), -1, np.int32))
    plain = CE.build_frames(lm, mac)
    full = CE.build_frames(lm, mac, asg=CE.Assign(nev, eva, taa, keys))
    new = {"assigned", "assignment", "allocations"}
    assert all(set(f) - set(g) == new and all(np.array_equal(f[k], g[k]) if k != "blocks" else True for k in g if k != "blocks")
               for f, g in zip(full[0], plain[0]))
    assert full[0][0]["assigned"] is False and full[0][0]["allocations"][0]["target_hz"] == OWN * 6250
    assert full[0][0]["allocations"][0]["target_row"] == 0 and full[0][0]["allocations"][0]["timeslot_assigned"] == 0b0100
    assert full[0][1]["assigned"] is True and full[0][1]["allocations"] is None
    assert full[0][1]["assignment"] == dict(ssi=0x77, address_type=6, usage_marker=5, from_hz=OWN * 6250, age_slots=1,
                                            allocations=1, idle=0)
    frames = [dict(f, usage=u) for f, u in zip(full[0] * 2, ("control", "traffic", "traffic", "stolen"))]
    assert CE.assigned_streams(frames) == {2: [frames[1], frames[3]]}
    assert _hip.ETSI_ASSIGN.itemsize == 208 and _hip.AE_FIELDS == 16 and _hip.TA_FIELDS == 8


def test_header_declares_the_entry_point_and_hip_carries_its_constants():
    from tetraear import _hip
    text = open(os.path.join(REPO, "include", "tetra_hip.h")).read()
    assert re.search(r"\bint tetra_etsi_assign\(tetra_ctx \*ctx,", text)
    for name, val in (("TETRA_ASSIGN_HOLD_DEFAULT", _hip.ASSIGN_HOLD_DEFAULT), ("TETRA_ASSIGN_IDLE_DEFAULT", _hip.ASSIGN_IDLE_DEFAULT)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == val == {"H": A.HOLD_DEFAULT, "I": A.IDLE_DEFAULT}[name[13]]
    assert re.search(r"TETRA_AE_FIELDS = (\d+)", text).group(1) == "16" and re.search(r"TETRA_TA_FIELDS = (\d+)", text).group(1) == "8"
    assert "#define TETRA_ABI_VERSION 2" in text and "NOT pinned against a conformance vector (DESIGN.md §5.27)" in text
