"""tetra_etsi_assign (k_assign_scan, k_assign_events, k_assign_follow) on the GPU against
tests/_etsi_assign_model.py: nev, ev, ta and the carried state compared whole -- the outputs are poisoned
before the call, so what it leaves alone shows.

  * built rows (tests/_etsi_assign_cases.py: _etsi_sdu_cases.random_call with allocations planted; the rows
    are records, as the SDU call leaves them, not soft bits) at C = 1, 5, 7 and 6 groups of G = 3, three
    successive calls with the state carried, with host and with device pointers;
  * the hand-made cases of tests/test_etsi_assign_model.py that need more than one carrier, the optional
    arrays left out, maxe 0 and 1, counts out of range, every error return, the profile stage, a seeded sweep;
  * the smallest real chain through EtsiStream and EtsiLowerMac(follow=True), and one wideband capture through
    WidebandReceiver.decode / decode_acquire and WidebandStream.
All of it fails on the parent commit: there is no such symbol and no such keyword.
"""
import ctypes
import os

import numpy as np
import pytest

import etsi as E
import _lmac_rows as R
import _etsi_mac_model as M
import _etsi_sdu_cases as K
import _etsi_sdu_model as S
import _etsi_assign_cases as AC
import _etsi_assign_model as A

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("TETRA_FUZZ_SCALE", "1")))
INVALID = -1   # TETRA_E_INVALID
N = 0
CTRL, FULL = A.TCH_CONTROL, A.TCH_FULL
OWN = AC.key_of(100)


# ------------------------------------------------------------------------------ the library's call

def poisoned_outputs(seed, C, G, maxe):
    rng = np.random.default_rng(seed)
    return [np.full(C // G, -77, np.int32), rng.integers(-99, 99, (C // G, max(maxe, 1), A.AE_FIELDS)).astype(np.int32),
            rng.integers(-99, 99, (C, A.MAXB, A.TA_FIELDS)).astype(np.int32)]


def call_assign(call, state, keys, outs, device=False, hold_slots=A.HOLD_DEFAULT, idle_max=A.IDLE_DEFAULT, shared_clock=0,
                maxe=8, with_tq=True, with_slots=True, C=None, drop=()):
    """tetra_etsi_assign on host arrays or (device) on torch tensors; state and outs are updated in place.
    drop: names of arrays passed as NULL.  Returns the return code."""
    from tetraear import _hip
    c = _hip.ctx()
    a = call["arrays"]
    named = dict(nsym=call["nsym"], nburst=a[0], bursts=a[1], nblock=a[2], blocks=a[3], npdu=a[5], pdus=a[6],
                 keep=call["keep"], slots=call["slots"] if with_slots else None, tq=call["tq"] if with_tq else None,
                 sdu=call["sdu"], ndone=call["ndone"], done=call["done"] if call["maxd"] > 0 else None, row_key=keys,
                 state=None if state is None else state.view(np.uint8), nev=outs[0], ev=outs[1] if maxe > 0 else None,
                 ta=outs[2])
    named = {k: None if v is None or k in drop else np.ascontiguousarray(v) for k, v in named.items()}
    C = len(a[0]) if C is None else C
    if device:
        import torch
        dev = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in named.items()}
        p = {k: _hip.ptr(v) for k, v in dev.items()}
    else:
        p = {k: _hip.ptr(v) for k, v in named.items()}
    rc = c.lib.tetra_etsi_assign(c.handle, p["nsym"], C, call["G"], call["row_bits"], call["advance"], hold_slots, idle_max,
                                 shared_clock, p["nburst"], p["bursts"], p["nblock"], p["blocks"], p["npdu"], p["pdus"],
                                 p["keep"], p["slots"], p["tq"], p["sdu"], call["maxd"], p["ndone"], p["done"], p["row_key"],
                                 p["state"], maxe, p["nev"], p["ev"], p["ta"])
    if device:
        torch.cuda.synchronize()
        for k, host in (("state", None if state is None else state.view(np.uint8)), ("nev", outs[0]),
                        ("ev", outs[1] if maxe > 0 else None), ("ta", outs[2])):
            if host is not None and dev[k] is not None:
                host[...] = dev[k].cpu().numpy().reshape(host.shape)
    return rc


def check_call(call, state, models, keys, seed, device=False, what="", **kw):
    """One call on the library and on the model (models: [State] per group, state: their array so far)."""
    C, G, maxe = len(call["arrays"][0]), call["G"], kw.get("maxe", 8)
    outs = poisoned_outputs(seed, C, G, maxe)
    before = [o.copy() for o in outs]
    mkw = {k: v for k, v in kw.items() if k in ("hold_slots", "idle_max", "shared_clock", "maxe", "with_tq", "with_slots")}
    nev, ev, ta = AC.run_model(call, models, keys, **mkw)
    assert call_assign(call, state, keys, outs, device, **kw) == 0, what
    want_ev, want_ta = A.expected_arrays(nev, ev, ta, before[1], before[2])
    assert outs[0].tolist() == nev.tolist(), (what, "nev", outs[0].tolist(), nev.tolist())
    assert np.array_equal(outs[1], want_ev), (what, "ev", np.argwhere(outs[1] != want_ev)[:4].tolist())
    assert np.array_equal(outs[2], want_ta), (what, "ta", [(i, outs[2][tuple(i[:2])].tolist(), want_ta[tuple(i[:2])].tolist())
                                                           for i in np.argwhere(outs[2] != want_ta)[:3].tolist()])
    want = A.state_array(models)
    assert state.tobytes() == want.tobytes(), (what, "state", [n for n in ("bit0", "expired", "released", "slot")
                                                               if not np.array_equal(state[n], want[n])])
    return outs, (nev, ev, ta)


def run_stream(calls, keys, seed, device=False, what="", **kw):
    NG = len(calls[0]["arrays"][0]) // calls[0]["G"]
    models, state = [A.State() for _ in range(NG)], np.zeros(NG, A.STATE_DTYPE)
    seen = []
    for n, call in enumerate(calls):
        seen.append(check_call(call, state, models, keys, seed + n, device, (what, n), **kw)[1])
    return seen, models


# ------------------------------------------------------------------------------ built rows

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("C,G", [(1, 1), (5, 1), (7, 1), (18, 3)])
def test_built_rows_equal_the_model(C, G, device):
    """Three successive calls with the state carried, short hold and idle times so that entries expire and are
    released inside the stream, the carriers on one clock; then the same rows with the defaults and own clocks."""
    calls, keys = AC.random_stream(40 + C, C, G, ncalls=3)
    seen, models = run_stream(calls, keys, 7, device, (C, G), hold_slots=6, idle_max=1, shared_clock=1)
    if C > 1:
        assert sum(int(nev.sum()) for nev, _, _ in seen) > 0 and any(r[0] == 1 for _, _, ta in seen for r in ta.values())
    run_stream(calls, keys, 8, device, (C, G, "defaults"))


def test_state_all_zero_and_freed_entries_compare_whole():
    """The sweep's comparison is of the whole state array: a freed entry keeps the fields it held."""
    calls, keys = AC.random_stream(47, 7, 1, ncalls=3)
    _, models = run_stream(calls, keys, 9, hold_slots=2, idle_max=0, shared_clock=1)
    assert sum(m.expired + m.released for m in models) > 0
    assert any(not e.active and e.nalloc for m in models for e in m.slot)


# ------------------------------------------------------------------------------ hand-made cases

def null():
    return [[M.null_pdu()]]


def burst(slot, blocks, cls=CTRL, jitter=0):
    tn, fn = AC.grid(slot * AC.SLOT)[:2]
    return (slot * AC.SLOT + jitter, N, blocks, cls, (tn, fn))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("slots_ab", [(0, 1), (1, 0), (0, 0)], ids=["a first", "b first", "equal T"])
def test_two_sources_allocate_one_target_slot(slots_ab, device):
    """Two carriers name timeslot 1 of a third in one call, at different and at equal T; a fourth is its own target
    on a stream far above 2^32 bits; a fifth hears a MAC-END that completes a chain and one that does not."""
    rng = np.random.default_rng(10)
    big = (1 << 33) + 5
    rows = [[burst(slots_ab[0], [AC.resource_alloc(rng, AC.alloc(140, 0b1000), ssi=11)])],
            [burst(slots_ab[1], [AC.resource_alloc(rng, AC.alloc(140, 0b1000), ssi=22)])],
            [burst(4, null(), cls=FULL), burst(8, null())],
            [burst(2, [AC.resource_alloc(rng, AC.alloc(150, 0b0010), ssi=33, addr_type=6, aux=7)]), burst(6, null(), cls=FULL),
             burst(10, null())],
            [burst(3, [K.first(K.payload(rng, K.FIRST_CAP), ssi=0xCAFE)]), burst(7, [AC.end_alloc(rng, AC.alloc(160, 1), [1, 0, 1])]),
             burst(11, null()), burst(12, [AC.end_alloc(rng, AC.alloc(160, 0b1000), [1])]), burst(16, null())]]
    keys = np.array([AC.key_of(100), AC.key_of(101), AC.key_of(140), AC.key_of(150), AC.key_of(160)], np.int32)
    bit0s = [big] * 5
    call = AC.rows_call(rng, rows, bit0s=bit0s)
    models, state = [A.State(big) for _ in range(5)], np.zeros(5, A.STATE_DTYPE)
    state["bit0"] = big
    _, (nev, ev, ta) = check_call(call, state, models, keys, 3, device, slots_ab, shared_clock=1)
    assert nev.tolist() == [1, 1, 0, 1, 2]
    assert ta[(2, 0)][:3] == [1, 22 if slots_ab != (1, 0) else 11, 1] and ta[(2, 0)][A.T_NALLOC] == 2
    assert ta[(3, 1)] == [1, 33, 6, 7, AC.key_of(150), 1, 0, 4] and ev[(3, 0)][A.E_P_HI] == 2
    assert ev[(4, 0)][A.E_SSI:] == [0xCAFE, 1, -1] and ev[(4, 1)][A.E_SSI:] == [-1, -1, -1]
    assert ta[(4, 2)][:2] == [1, 0xCAFE] and ta[(4, 4)][:2] == [1, -1]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_optional_arrays_and_maxe(device):
    """row_key NULL (events listed, nothing assigned), tq NULL (step 3 skipped), slots NULL (no burst takes part),
    maxe 0 with ev NULL, maxe 1 with three events in a group (nev 3, one recorded, one applied), maxd 0."""
    rng = np.random.default_rng(9)
    rows = [[burst(0, [AC.resource_alloc(rng, AC.alloc(100, 0b1000))]), burst(1, [AC.resource_alloc(rng, AC.alloc(100, 0b0100))]),
             burst(2, [AC.resource_alloc(rng, AC.alloc(100, 0b0010))])] + [burst(4 + i, null()) for i in range(3)]]
    call = AC.rows_call(rng, rows)
    keys = np.array([OWN], np.int32)
    for kw, states in ((dict(maxe=1), [1, 0, 0]), (dict(maxe=0), [0, 0, 0]), (dict(maxe=3), [1, 1, 1]),
                       (dict(with_tq=False), [1, 1, 1]), (dict(with_slots=False), [-1, -1, -1])):
        models, state = [A.State()], np.zeros(1, A.STATE_DTYPE)
        _, (nev, ev, ta) = check_call(call, state, models, keys, 4, device, str(kw), **kw)
        assert nev.tolist() == [3] and [ta[(0, b)][0] for b in range(3, 6)] == states, kw
    models, state = [A.State()], np.zeros(1, A.STATE_DTYPE)
    _, (nev, ev, ta) = check_call(call, state, models, None, 4, device, "row_key NULL")
    assert nev.tolist() == [3] and all(ev[(0, k)][A.E_TARGET] == -1 for k in range(3)) and not state["slot"]["active"].any()
    calls, keys = AC.random_stream(60, 5, 1)
    for kw in (dict(), dict(with_tq=False), dict(with_slots=False, with_tq=False)):
        run_stream([dict(calls[0], maxd=0)], keys, 5, device, "maxd 0", shared_clock=1, **kw)
        run_stream(calls, None, 5, device, "no keys", shared_clock=1, **kw)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_counts_out_of_range_are_clamped(device):
    """nburst / nblock of 99 read MAXB bursts / MAXJ blocks of whatever the arrays hold, negative ones none; npdu
    of 99 reads MAXPDU records, negative none; ndone of 99 reads maxd records."""
    calls, keys = AC.random_stream(61, 6, 1)
    call = calls[0]
    a = [x.copy() for x in call["arrays"]]
    a[0][:] = [99, -3, a[0][2], 99, a[0][4], -1]
    a[2][:] = [99, a[2][1], -2, 99, -1, a[2][5]]
    a[5][0, :] = 99
    a[5][2, :] = -4
    a[5][4, :] = 0
    a[6][0] = np.random.default_rng(5).integers(0, 3, a[6][0].shape)   # PDU kinds 0..2 over row 0's poison
    call = dict(call, arrays=tuple(a), ndone=np.array([99, -5, 0, 1, 99, 2], np.int32))
    run_stream([call], keys, 6, device, "clamped", shared_clock=1, hold_slots=5, idle_max=1)


def test_invalid_arguments_write_nothing():
    calls, keys = AC.random_stream(62, 6, 1)
    good = calls[0]
    bad = [dict(G=0), dict(G=4), dict(G=65), dict(row_bits=-1, G=2), dict(maxd=-1), dict(nsym=None)]
    kws = [dict(maxe=-1), dict(hold_slots=-1), dict(idle_max=-1), dict(C=0), dict(C=(1 << 24) + 1)]
    kws += [dict(drop=(n,)) for n in ("nburst", "bursts", "nblock", "blocks", "npdu", "pdus", "sdu", "ndone", "done", "nev",
                                      "ev", "ta")]
    for over, kw in [(o, {}) for o in bad] + [({}, k) for k in kws]:
        state = np.zeros(6, A.STATE_DTYPE)
        state["bit0"] = 5
        outs = poisoned_outputs(3, 6, 1, 8)
        before = [o.copy() for o in outs]
        assert call_assign(dict(good, **over), state, keys, outs, **kw) == INVALID, (over, kw)
        assert all(np.array_equal(x, y) for x, y in zip(outs, before)) and (state["bit0"] == 5).all(), (over, kw)
        assert not state["slot"]["active"].any()
    outs = poisoned_outputs(3, 6, 1, 8)
    assert call_assign(good, None, keys, outs) == INVALID
    # a good call after the refusals; maxd 0 needs no done array, maxe 0 no ev
    state, outs = np.zeros(6, A.STATE_DTYPE), poisoned_outputs(3, 6, 1, 0)
    assert call_assign(dict(good, maxd=0), state, keys, outs, maxe=0, drop=("done", "ev")) == 0
    assert (state["bit0"] == 4080).all() and (outs[0] >= 0).all()


def test_three_kernels_under_the_profile_stage():
    """With device pointers the call is three launches under the stage etsi_assign."""
    import torch
    from tetraear import _hip
    calls, keys = AC.random_stream(63, 5, 1)
    c = _hip.ctx()
    c.check(c.lib.tetra_profile(c.handle, 1), "tetra_profile")
    try:
        rc = call_assign(calls[0], np.zeros(5, A.STATE_DTYPE), keys, poisoned_outputs(1, 5, 1, 8), device=True)
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(4096)
        ms, cnt, n = (ctypes.c_double * 64)(), (ctypes.c_int64 * 64)(), ctypes.c_int()
        c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    finally:
        c.check(c.lib.tetra_profile(c.handle, 0), "tetra_profile")
    stages = [s.decode() for s in names.raw.split(b"\0")[:n.value]]
    assert rc == 0 and "etsi_assign" in stages and cnt[stages.index("etsi_assign")] == 1


SWEEP = ((1, 1), (5, 1), (17, 1), (33, 1), (34, 2), (33, 3), (64, 64), (128, 64))


@pytest.mark.parametrize("C,G", SWEEP)
def test_seeded_sweep(C, G):
    """Random calls over C rows in groups of G, two successive calls a seed, random hold / idle times, shared and
    own clocks, every frequency offset; odd seeds on device pointers."""
    for seed in range(3 * SCALE):
        rng = np.random.default_rng(1000 * C + seed)
        calls, keys = AC.random_stream(2000 * C + seed, C, G, ncalls=2)
        run_stream(calls, keys, seed, bool(seed & 1), (C, G, seed), hold_slots=int(rng.choice([0, 3, 6, 720])),
                   idle_max=int(rng.choice([0, 1, 72])), shared_clock=int(rng.integers(2)), maxe=int(rng.choice([1, 2, 8, 64])))


# ------------------------------------------------------------------------------ the smallest real chain

CELL = (262, 1017, 33)
CHAIN_HZ = 421_512_500          # key 67442: band 4, carrier 860, offset +12.5 kHz
CHAIN_SSI = 0xBEEF07
# slot = burst index: a burst the stream's start may cost, an SB on slot 1, the allocation on slot 4 (TN 1) naming
# TN 3, the traffic on slot 6 (TN 3); slot 2 is the TN 3 burst before the allocation
CHAIN_ALLOC, CHAIN_TRAFFIC, CHAIN_BURSTS = 4, 6, 13


def chain_bits(rng, cell, slot0, alloc_at, ca, traffic_at, nbursts, lead, ssi=CHAIN_SSI):
    """Consecutive bursts from slot count slot0 on: an SB first, a MAC-RESOURCE carrying ca in burst alloc_at
    (None: nowhere), a full traffic slot of random bits in burst traffic_at (None: nowhere), null PDUs everywhere
    else -- as tests/test_gpu_etsi_traffic.py plants them.  Returns (bits, the traffic slot's 432 bits)."""
    import _etsi_traffic_model as T
    init = E.scramble_init(*cell)
    scr = E.scramble_seq(init, 432)
    parts, t4 = [rng.integers(0, 2, lead).astype(np.uint8)], rng.integers(0, 2, 432).astype(np.uint8)
    for b in range(nbursts):
        if b == 0:
            pay = [M.block(rng, 2, [M.sync(M.sync_for_slot(rng, slot0, cell))]), M.block(rng, 1, [M.null_pdu()])]
            parts.append(E.make_burst(E.BURST_SB, rng, scr, pay)[0])
        elif b == traffic_at:
            parts.append(T.traffic_burst(0, t4, scr, rng)[0])
        elif b == alloc_at:
            parts.append(E.make_burst(0, rng, scr, [M.block(rng, 0, AC.resource_alloc(rng, ca, ssi=ssi, addr_type=6, aux=21))])[0])
        else:
            parts.append(E.make_burst(0, rng, scr, [M.block(rng, 0, [M.null_pdu()])])[0])
    parts.append(rng.integers(0, 2, 400).astype(np.uint8))
    return np.concatenate(parts), t4


def chain_frames(**kw):
    """One channel at 2.4 MSps, four 131072-sample chunks, through EtsiStream and EtsiLowerMac(mac, sdu, traffic,
    **kw) with the cell given: (the frames in order, the receiver, the planted traffic bits)."""
    from tetraear.signal.etsi import EtsiStream
    from tetraear.core.etsi import EtsiLowerMac
    rng = np.random.default_rng(3141)
    scr = E.scramble_seq(E.scramble_init(*CELL), 432)
    first = E.make_burst(0, rng, scr, [M.block(rng, 0, [M.null_pdu()])])[0]
    bits, t4 = chain_bits(rng, CELL, 1, CHAIN_ALLOC - 1, AC.alloc(860, 0b0010), CHAIN_TRAFFIC - 1, CHAIN_BURSTS - 1, 0)
    bits = np.concatenate([rng.integers(0, 2, 60).astype(np.uint8), first, bits])
    L = 131072
    x = E.modulate(bits, 4 * L, t0=0.4, phase0=1.1, cfo=120.0)
    st = EtsiStream(2.4e6, 1)
    lm = EtsiLowerMac(*CELL, mac=True, sdu=True, traffic=True, **kw)
    frames = []
    for k in range(4):
        d = st.demod(x[None, k * L:(k + 1) * L])
        frames += lm.decode_stream(d[1], d[0], d[3])[0]
    return frames, lm, t4


def plain(v):
    """A frame (or anything in it) with its arrays as lists, for ==."""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v.tolist() if isinstance(v, np.ndarray) else v


NEW_KEYS = ("assigned", "assignment", "allocations")


def without(frames):
    return [{k: v for k, v in plain(f).items() if k not in NEW_KEYS} for f in frames]


def test_chain_marks_the_planted_slot_assigned():
    import _etsi_traffic_model as T
    from tetraear.core.etsi import assigned_streams, traffic_streams
    frames, lm, t4 = chain_frames(follow=True, carrier_hz=CHAIN_HZ)
    assert len(frames) >= CHAIN_BURSTS - 1 and all(f["assigned"] is None for f in frames if f["tn"] is None)
    heard = [f for f in frames if f["allocations"]]
    assert len(heard) == 1 and heard[0]["tn"] == 1 and heard[0]["assigned"] is False
    a = heard[0]["allocations"][0]
    assert (a["carrier"], a["timeslot_assigned"], a["updownlink_assigned"], a["extended"]) == (860, 0b0010, 1, None)
    assert (a["target_hz"], a["target_row"], a["ssi"], a["address_type"], a["aux"]) == (CHAIN_HZ, 0, CHAIN_SSI, 6, 21)
    at = frames.index(heard[0])
    tn3 = [(i, f) for i, f in enumerate(frames) if f["tn"] == 3]
    assert [f["assigned"] for i, f in tn3 if i < at] == [False] and all(f["assigned"] is True for i, f in tn3 if i > at)
    slot = [f for f in frames if f["usage"] == "traffic"]
    assert len(slot) == 1 and np.array_equal(T.signs(slot[0]["traffic"]["soft"]), t4)
    assert slot[0]["assignment"] == dict(ssi=CHAIN_SSI, address_type=6, usage_marker=21, from_hz=CHAIN_HZ, age_slots=2,
                                         allocations=1, idle=0)
    assert all(f["assigned"] is False for f in frames if f["tn"] in (1, 2, 4))
    assert assigned_streams(frames) == {3: slot} and traffic_streams(frames) == {3: slot}
    later = [f for i, f in tn3 if i > frames.index(slot[0])]
    assert later and later[0]["assignment"]["idle"] == 0 and later[0]["assignment"]["age_slots"] == 6
    st = lm.assign_stats
    assert st["expired"].tolist() == [0] and st["released"].tolist() == [0]
    lm.reset_stream()
    assert lm._assign is None


def test_chain_without_a_carrier_frequency_lists_and_assigns_nothing():
    frames, lm, _ = chain_frames(follow=True)
    heard = [f for f in frames if f["allocations"]]
    assert len(heard) == 1 and heard[0]["allocations"][0]["target_hz"] is None
    assert heard[0]["allocations"][0]["target_row"] is None and heard[0]["allocations"][0]["carrier"] == 860
    assert all(f["assigned"] is False and f["assignment"] is None for f in frames if f["tn"] is not None)
    # follow=False: the frames are today's, key for key
    off, _, _ = chain_frames()
    assert not any(k in f for f in off for k in NEW_KEYS) and without(frames) == plain(off)
    from tetraear.core.etsi import EtsiLowerMac
    for kw in (dict(follow=True), dict(mac=True, follow=True), dict(mac=True, sdu=True, follow=True, carrier_hz=421_512_501)):
        with pytest.raises(ValueError):
            EtsiLowerMac(*CELL, **kw)


# ------------------------------------------------------------------------------ the wideband chain

NW = 2_000_000
WB_A, WB_B = 130, 401            # carrier 130 announces, carrier 401 carries the call
WB_CENTER = 420_000_000          # row 401 is bin 401 - 800: 410.025 MHz, band 4, carrier number 401
WB_NUMBER, WB_B_HZ = 401, (WB_B - 800) * 25000
WB_SLOT0 = (20, 40)              # the SBs' slot counts; carrier 401's burst 4 is slot 44: TN 1, FN 12
WB_SSI = 0xBEEF08


@pytest.fixture(scope="module")
def capture():
    return build_capture()


def build_capture():
    """(x [NW] complex64, cells [800], the planted traffic bits): both carriers start with a burst the filter bank's
    start costs, then an SB; 130 sends the allocation in its third burst, 401 a full traffic slot in its sixth.  White noise 40 dB under a
    carrier in its 25 kHz: in a noiseless synthetic capture a dozen empty rows hold a carrier's float32 rounding
    residue (150 dB down in the float64 oracle), decode it in acquisition, and would hear its announcement too."""
    import wideband as W
    d = W.design()
    nbb = NW // d["D"] + 1
    s = np.zeros((d["M"], nbb), np.complex128)
    cells = np.full(d["M"], 3, np.uint32)
    t4 = None
    for i, k in enumerate((WB_A, WB_B)):
        rng = np.random.default_rng(990 + i)
        cells[k] = E.scramble_init(*CELL)
        scr = E.scramble_seq(int(cells[k]), 432)
        first = E.make_burst(0, rng, scr, [M.block(rng, 0, [M.null_pdu()])])[0]
        bits, t = chain_bits(rng, CELL, WB_SLOT0[i], 1 if i == 0 else None, AC.alloc(WB_NUMBER, 0b1000), 4 if i == 1 else None, 6,
                             0, ssi=WB_SSI)
        t4 = t if i == 1 else t4
        bits = np.concatenate([rng.integers(0, 2, (0, 100)[i]).astype(np.uint8), first, bits])
        s[k] = E.modulate(bits, nbb, fs=d["fs"] / d["D"], t0=0.1 + 0.13 * i, phase0=0.7 * i, cfo=(-40.0, 25.0)[i])
    x = W.synthesize(s, d, NW)
    rng = np.random.default_rng(999)
    sigma = np.sqrt(np.mean(np.abs(x) ** 2) / 2 * d["M"] / 1e4 / 2)   # per component: carrier power x 800 rows / 10^4
    x = x + sigma * (rng.standard_normal(NW) + 1j * rng.standard_normal(NW))
    return x.astype(np.complex64), cells, t4


def judge(frames, t4, center, what):
    """The planted slot is reported once on carrier 401, assigned from carrier 130's frequency; carrier 130 lists the
    allocation with row 401 as its target; nothing else on either carrier is assigned."""
    import _etsi_traffic_model as T
    heard = [a for f in frames[WB_A] for a in f["allocations"] or ()]
    assert len(heard) == 1, (what, len(heard))
    assert (heard[0]["carrier"], heard[0]["target_row"], heard[0]["target_hz"]) == (WB_NUMBER, WB_B, center + WB_B_HZ), what
    slot = [f for f in frames[WB_B] if f["usage"] == "traffic" and np.array_equal(T.signs(f["traffic"]["soft"]), t4)]
    assert len(slot) == 1 and slot[0]["assigned"] is True and (slot[0]["tn"], slot[0]["fn"]) == (1, 12), what
    a = slot[0]["assignment"]
    assert (a["ssi"], a["address_type"], a["usage_marker"], a["from_hz"], a["allocations"]) == \
        (WB_SSI, 6, 21, center + WB_A * 25000, 1), (what, a)
    assert not any(f["assigned"] for f in frames[WB_A]) and not any(f["allocations"] for f in frames[WB_B]), what
    when = lambda f: f.get("stream_sample", f["sample"])
    assert all(f["assigned"] is (f["tn"] == 1 and when(f) > when(slot[0]) - 100) for f in frames[WB_B]
               if f["tn"] is not None), what
    return slot[0]


def test_wideband_joins_the_carriers(capture):
    from tetraear.signal.wideband import WidebandReceiver
    x, cells, t4 = capture
    rx = WidebandReceiver()
    kw = dict(mac=True, timebase="vote", traffic=True, sdu=True)
    full = rx.decode(x, cells, follow=True, center_hz=WB_CENTER, **kw)
    judge(full, t4, WB_CENTER, "decode")
    assert rx.assign_stats["expired"].sum() == 0 and rx.assign_stats["released"].sum() == 0
    # follow=False: today's frames, key for key
    off = rx.decode(x, cells, **kw)
    for k in (WB_A, WB_B):
        assert len(off[k]) >= 4 and not any(key in f for f in off[k] for key in NEW_KEYS)
        assert without(full[k]) == plain(off[k]), k
    # another raster: the carrier number still resolves, because the offset is inherited
    moved = rx.decode(x, cells, follow=True, center_hz=WB_CENTER + 6250, **kw)
    judge(moved, t4, WB_CENTER + 6250, "offset +6.25 kHz")
    for bad in (dict(follow=True), dict(follow=True, center_hz=WB_CENTER + 1)):
        with pytest.raises(ValueError):
            rx.decode(x[:1000], cells, **kw, **bad)
    with pytest.raises(ValueError):
        rx.decode(x[:1000], cells, mac=True, timebase="vote", follow=True, center_hz=WB_CENTER)   # no sdu
    import types
    from tetraear.signal.wideband import row_keys
    with pytest.raises(ValueError):
        row_keys(types.SimpleNamespace(fs=19.2e6, M=800), WB_CENTER)   # rows 24 kHz apart
    keys = row_keys(rx.plan, WB_CENTER)
    assert keys.dtype == np.int32 and keys[[0, 1, 399, 400, 799]].tolist() == [67200, 67204, 68796, 65600, 67196]


def test_wideband_acquire_and_stream(capture):
    from tetraear.signal.wideband import WidebandReceiver, WidebandStream
    x, cells, t4 = capture
    kw = dict(mac=True, timebase="vote", traffic=True, sdu=True, follow=True, center_hz=WB_CENTER)
    rx = WidebandReceiver()
    want = judge(rx.decode(x, cells, **kw), t4, WB_CENTER, "decode")
    got = judge(rx.decode_acquire(x, cells, **kw)[0], t4, WB_CENTER, "decode_acquire")   # the cells handed in as acquired
    assert got["assignment"] == want["assignment"] and got["sample"] == want["sample"]
    with pytest.raises(ValueError):
        WidebandStream(cells, mac=True, timebase="vote", sdu=True, follow=True)
    st = WidebandStream(cells, **kw)
    frames = [[] for _ in cells]
    for a, b in ((0, 611_111), (611_111, 700_001), (700_001, NW)):
        for k, fr in enumerate(st.decode(x[a:b])):
            frames[k] += fr
    once = judge(frames, t4, WB_CENTER, "stream")   # once, though the carried tails are decoded twice
    assert once["assignment"] == want["assignment"] and st.assign_stats["expired"].sum() == 0
    st.reset()
    assert not st.assign["slot"]["active"].any() and not st.assign["bit0"].any()
