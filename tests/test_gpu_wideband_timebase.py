"""The wideband chain's TDMA timebase (WidebandReceiver.decode / decode_acquire(timebase=True),
WidebandStream(timebase=True), synth_wideband(grid=True), BenchStep with TETRA_WB_MAC=timebase).

The truth of the first part is built on the CPU from the oracles alone: six carriers of the 800 carry a
continuous downlink of oracle/etsi.py bursts whose SBs announce consecutive slot counts, modulated at
the carriers' 50 kHz and put on the 20 MSps capture by oracle/wideband.py's synthesis filter bank.  The
capture gives two timing chunks per carrier, so one overlap.  A decoded frame is matched to its
planted burst by its blocks' type-1 bits, never by position.  Slots are integers: compared exactly.
"""
import numpy as np
import pytest

import etsi as E
import wideband as W
import _etsi_mac_model as MM

pytestmark = pytest.mark.gpu

NW_CPU = 1_700_000
CARRIERS = (3, 130, 257, 401, 640, 797)
# burst kinds per carrier: the first SB is burst 1, 2, 3 or 4 (burst 4 starts in the chunks' overlap)
KINDS = ((0, 2, 1, 0, 2, 0, 1, 0), (1, 0, 2, 0, 1, 2, 0, 0), (0, 1, 0, 2, 0, 1, 0, 0), (1, 0, 0, 1, 2, 0, 1, 0),
         (0, 2, 0, 1, 2, 1, 0, 0), (1, 1, 2, 2, 0, 0, 1, 0))
SLOT0 = (4316, 70, 2000, 17, 4319, 1234)
PIECES_CPU = ((0, 611_111), (611_111, 700_001), (700_001, NW_CPU))
NW_GPU = 3_300_000
TODAY = {"position", "burst", "burst_kind", "timeslot", "blocks", "crc_ok", "chunk", "sample"}


def row_of(slot):
    return (slot % 4 + 1, slot // 4 % 18 + 1, slot // 72 + 1)


def key_of(blocks):
    return tuple(np.asarray(b, np.uint8).tobytes() for b in blocks)


@pytest.fixture(scope="module")
def planted():
    """(x [NW_CPU] complex64, cells [800] uint32, {type-1 bits of a burst's blocks: (carrier, b, slot)})."""
    d = W.design()
    M, D = d["M"], d["D"]
    nbb = NW_CPU // D + 1
    s = np.zeros((M, nbb), np.complex128)
    cells = np.full(M, 3, np.uint32)
    truth = {}
    for i, k in enumerate(CARRIERS):
        rng = np.random.default_rng(900 + i)
        cell = (int(rng.integers(1, 1024)), int(rng.integers(0, 1 << 14)), int(rng.integers(0, 64)))
        cells[k] = E.scramble_init(*cell)
        scr = E.scramble_seq(int(cells[k]))
        bits = []
        for b, kind in enumerate(KINDS[i]):
            slot = (SLOT0[i] + b) % MM.TDMA_SLOTS
            pay = None
            if kind == E.BURST_SB:
                pay = [MM.block(rng, 2, [MM.sync(MM.sync_for_slot(rng, slot, cell))]), rng.integers(0, 2, 124).astype(np.uint8)]
            bb, jobs = E.make_burst(kind, rng, scr, pay)
            bits.append(bb)
            truth[key_of(t for _, t in jobs)] = (k, b, slot)
        s[k] = E.modulate(np.concatenate(bits), nbb, fs=d["fs"] / D, t0=0.1 + 0.13 * i, phase0=0.7 * i,
                          cfo=(-100.0, -40.0, 0.0, 25.0, 60.0, 100.0)[i])
    return W.synthesize(s, d, NW_CPU).astype(np.complex64), cells, truth


def judge(frames, truth, order="sample", what=""):
    """The conditions on one decode of the planted capture; frames [800][frame].  Returns (known share
    from the first SYNC on, largest |r| between consecutive frames of a carrier, frames judged)."""
    known = after = judged = 0
    rmax = 0
    for k, fr in enumerate(frames):
        if k not in CARRIERS:
            assert all(f["tn"] is None for f in fr), (what, k)
            continue
        assert [f[order] for f in fr] == sorted(f[order] for f in fr)
        synced = False
        seen = []
        for f in fr:
            hit = truth.get(key_of(b["bits"] for b in f["blocks"]))
            own = f["burst_kind"] == 2 and f["blocks"][0]["crc_ok"]
            if hit is None:   # a burst the capture's edge cut, or one decoded before the cell was acquired
                assert not f["crc_ok"], (what, k, f[order])
                synced |= bool(own)
                continue
            assert hit[0] == k and hit[1] not in seen, (what, k, hit)
            seen.append(hit[1])
            judged += 1
            if not synced and not own:
                assert (f["tn"], f["fn"], f["mn"], f["slot_flags"]) == (None, None, None, 0), (what, k, hit)
                continue
            synced = True
            after += 1
            if f["tn"] is not None:
                assert (f["tn"], f["fn"], f["mn"]) == row_of(hit[2]), (what, k, hit, f["tn"], f["fn"], f["mn"])
                assert f["slot_flags"] == (1 if own else 0), (what, k, hit, f["slot_flags"])
                known += 1
        assert seen == sorted(seen) and synced and len(seen) >= 2, (what, k, seen)
        pos = [f[order] // 2 for f in fr]
        rmax = max([rmax] + [abs((q - p + 255) % 510 - 255) for p, q in zip(pos, pos[1:])])
    return known / after, rmax, judged


@pytest.fixture(scope="module")
def decoded(planted):
    from tetraear.signal.wideband import WidebandReceiver
    x, cells, _ = planted
    rx = WidebandReceiver()
    given = rx.decode(x, cells, timebase=True)
    got, state, ngood = rx.decode_acquire(x, np.full(len(cells), 3, np.uint32), timebase=True)
    return given, got, state, ngood


def view(f, key="sample"):
    return (f[key], f["position"], f["burst_kind"], f["chunk"], f["crc_ok"], f["tn"], f["fn"], f["mn"], f["slot_flags"],
            [(b["channel"], b["crc_ok"], b["block"], b["bits"].tobytes(), b["npdu"]) for b in f["blocks"]])


def test_planted_slots_are_decoded(planted, decoded):
    share, rmax, judged = judge(decoded[0], planted[2], what="decode")
    print("timebase: known share from the first SYNC on %.4f, largest |r| %d bits, %d frames judged" % (share, rmax, judged))
    assert judged >= 4 * len(CARRIERS)
    assert share >= 0.95
    assert any(f["chunk"] == 1 and f["tn"] is not None for k in CARRIERS for f in decoded[0][k])


def test_decode_and_decode_acquire_agree(planted, decoded):
    given, got, state, ngood = decoded
    cells = planted[1]
    for k in CARRIERS:
        assert int(state[k]) == int(cells[k]) and ngood[k] > 0
        assert [view(f) for f in got[k]] == [view(f) for f in given[k]], k
    judge(got, planted[2], what="decode_acquire")


def test_timebase_false_returns_todays_frames(planted, decoded):
    """decode() and decode(mac=True) carry exactly today's keys, and timebase=True keeps the same bursts
    (the device's keep is merge_chunks') with the same blocks."""
    from tetraear.signal.wideband import WidebandReceiver, WidebandStream
    x, cells, _ = planted
    rx = WidebandReceiver()
    plain, mac = rx.decode(x, cells), rx.decode(x, cells, mac=True)
    for k in CARRIERS:
        assert len(plain[k]) == len(mac[k]) == len(decoded[0][k]) > 0
        for f, g, h in zip(plain[k], mac[k], decoded[0][k]):
            assert set(f) == set(g) == TODAY and set(h) == TODAY | {"tn", "fn", "mn", "slot_flags"}
            assert all(set(b) == {"channel", "crc_ok", "bits", "block"} for b in f["blocks"])
            assert all(set(b) == {"channel", "crc_ok", "bits", "block", "npdu", "pdus"} for b in g["blocks"] + h["blocks"])
            assert view(dict(g, tn=0, fn=0, mn=0, slot_flags=0)) == view(dict(h, tn=0, fn=0, mn=0, slot_flags=0))
    st = WidebandStream(cells)
    assert st.tdma is None and all(set(f) == TODAY | {"stream_sample"} for fr in st.decode(x[:PIECES_CPU[0][1]]) for f in fr)
    for bad in (dict(tol=63), ):
        with pytest.raises(ValueError):
            rx.decode(x, cells, timebase=True, **bad)
    with pytest.raises(ValueError):
        WidebandReceiver(m2=3931).decode(x, cells, timebase=True)
    with pytest.raises(ValueError):
        WidebandStream(cells, m2=3931, timebase=True)


def test_stream_carries_the_timebase(planted):
    from tetraear.signal.wideband import WidebandStream
    x, cells, truth = planted
    for given in (True, False):
        st = WidebandStream(cells if given else None, timebase=True)
        frames = [[] for _ in cells]
        for a, b in PIECES_CPU:
            for k, fr in enumerate(st.decode(x[a:b])):
                frames[k] += fr
        share, rmax, judged = judge(frames, truth, "stream_sample", "stream given=%s" % given)
        print("stream (cells %s): known share %.4f, largest |r| %d bits, %d frames judged" %
              ("given" if given else "acquired", share, rmax, judged))
        assert share >= 0.95 and judged >= (4 if given else 2) * len(CARRIERS)
        assert st.tdma["locked"][list(CARRIERS)].all() and st.tdma["bit0"][0] == st.y0 // 2 > 0
        st.reset()
        assert not st.tdma.view(np.uint8).any()


# ------------------------------------------------------------------------------ the synthesiser's grid

def _synth(c, Nw, seed):
    from tetraear import _hip
    from tetraear.signal.wideband import wb_plan
    p = wb_plan()
    nb = c.lib.tetra_synth_bursts_per_channel(Nw // p.D + 1, p.fs / p.D)
    out = (np.empty(Nw, np.complex64), np.empty(p.M, np.uint32), np.empty((p.M, nb), np.int32),
           np.empty((p.M, nb, 2, 268), np.uint8), np.empty(p.M, np.float64))
    c.check(c.lib.tetra_synth_wideband(c.handle, p.c, Nw, seed, 25.0, 300.0, *[_hip.ptr(v) for v in out]), "synth_wideband")
    return out


def test_grid_flag_off_is_bit_identical():
    """A context of its own: the capture recorded before the flag was ever set on it, the one with the
    flag on (only the SBs' TN / FN / MN bits differ, and they are the planted slots), and the one with
    the flag off again, which equals the recording bit for bit."""
    from tetraear import _hip
    from tetraear.signal.wideband import planted_slots
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    rec = _synth(c, 150_000, 17)
    c.check(c.lib.tetra_synth_set_grid(c.handle, 1), "set_grid")
    on = _synth(c, 150_000, 17)
    c.check(c.lib.tetra_synth_set_grid(c.handle, 0), "set_grid")
    off = _synth(c, 150_000, 17)
    for a, b in zip(rec, off):
        assert a.tobytes() == b.tobytes()
    for i in (1, 2, 4):
        assert np.array_equal(rec[i], on[i])
    sb = on[2] == 2
    field = np.zeros(268, bool)
    field[10:23] = True
    assert np.array_equal(on[3][..., ~field], rec[3][..., ~field]) and np.array_equal(on[3][~sb], rec[3][~sb])
    assert not np.array_equal(on[0], rec[0]) and sb.sum() > 100
    slots = planted_slots(17, *on[2].shape)
    bits = on[3][:, :, 0, 10:23].astype(np.int64)
    val = (bits << np.arange(12, -1, -1)).sum(axis=-1)
    want = (slots % 4) << 11 | (slots // 4 % 18 + 1) << 6 | (slots // 72 + 1)
    assert np.array_equal(val[sb], want[sb])
    assert len(np.unique(slots[:, 0])) > 500 and slots.min() >= 0 and slots.max() < 4320


@pytest.fixture(scope="module")
def capture_grid():
    from tetraear.signal.wideband import synth_wideband
    return synth_wideband(NW_GPU, seed=17, snr_db=25.0, cfo_max=300.0, grid=True)


def test_synthesised_grid_is_decoded(capture_grid):
    """All 800 carriers, three chunks each: no frame carries a slot other than the planted one, the
    bursts kept are merge_chunks', and most frames after a carrier's first SYNC are known."""
    from tetraear.signal.wideband import WidebandReceiver, planted_slots
    x, cells, kinds, payload, _ = capture_grid
    slots = planted_slots(17, *kinds.shape)
    rx = WidebandReceiver()
    frames, host = rx.decode(x, cells, timebase=True), rx.decode(x, cells)
    known = judged = after = 0
    for k, fr in enumerate(frames):
        assert [(f["sample"], f["position"], f["chunk"]) for f in fr] == [(f["sample"], f["position"], f["chunk"]) for f in host[k]], k
        synced = False
        for f in fr:
            b0 = f["blocks"][0]
            n1 = len(b0["bits"])
            hit = np.flatnonzero((payload[k, :, 0, :n1] == (b0["bits"] & 1)).all(axis=1) & (kinds[k] == f["burst_kind"]))
            own = f["burst_kind"] == 2 and b0["crc_ok"]
            synced |= own
            after += synced
            if f["tn"] is None:
                assert not own
                continue
            known += 1
            if b0["crc_ok"] and len(hit) == 1:
                judged += 1
                assert (f["tn"], f["fn"], f["mn"]) == row_of(int(slots[k, hit[0]])), (k, f["sample"], int(hit[0]))
    print("synthesised grid: %d frames known, %d judged, %.4f of those from a carrier's first SYNC on" %
          (known, judged, known / max(after, 1)))
    assert judged > 5000 and known > 0


@pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])
def test_bench_step_timebase(pipelined, monkeypatch):
    import torch
    from tetraear import _hip
    from tetraear.signal.wideband import BenchStep
    dev = torch.device("cuda", 0)
    steps = []
    for mode in (None, "timebase"):
        if mode is None:
            monkeypatch.delenv("TETRA_WB_MAC", raising=False)
        else:
            monkeypatch.setenv("TETRA_WB_MAC", mode)
        c = _hip.Context()
        c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
        st = BenchStep(c, NW_GPU, seed=3, device=dev)
        if pipelined and mode:
            st.pipeline()
        for _ in range(2 if mode else 1):
            st()
        torch.cuda.synchronize(dev)
        steps.append(st)
    ref, tb = steps
    q0, q = ref.quality(), tb.quality()
    assert set(q0) == {"blocks", "crc_ok", "bursts", "decoded_frac", "per_chunk"}
    assert set(ref.config(1)) == set(tb.config(1)) - {"mac"} and tb.config(1)["mac"] == "timebase"
    print("bench step: %s" % {k: q[k] for k in ("bursts", "timebase_known", "timebase_wrong", "timebase_checked")})
    assert q["timebase_wrong"] == 0 and q["timebase_known"] > 0 and q["timebase_checked"] > 5000
    monkeypatch.setenv("TETRA_WB_MAC", "slots")
    with pytest.raises(ValueError):
        BenchStep(_hip.ctx(), NW_GPU, seed=3, device=dev)
