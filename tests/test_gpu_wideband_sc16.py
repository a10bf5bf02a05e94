"""Wideband chain (C3) on SC16 captures: the channeliser's SC16 loaders against their specification,
"cf32 of x / 32768" -- bit for bit in every analysis form of both designs, at the shortest capture, on
the conversion's edge values and from device pointers; then the chain, the stream and the bench step
on quantised captures.

Measured on the MI355X, 1_120_000 samples at 30 dB, seed 11, CRC-good blocks of all blocks decoded
(test_round_trip_16_bit, test_round_trip_counts): unquantised 3494 of 3494, 16-bit 3494 of 3494, 12-bit
3494 of 3494.
"""
import os

import numpy as np
import pytest

import wideband as W
from _wb_sc16 import canon, q16, twin

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("TETRA_FUZZ_SCALE", "1")))
FORMS = [(2, "1"), (2, "2"), (2, "3"), (2, "4"), (4, "1"), (4, "2")]   # (oversample, TETRA_WB_ANALYSIS)
E_INVALID = -1
EDGE = np.array([-32768, 32767, -1, 0, 1], np.int16)


def min_nw(plan):
    """The shortest capture with one 72 kHz output: Q filter-bank blocks."""
    nw = plan.c.M * plan.c.P + (plan.c.Lg // plan.c.up - 1) * plan.c.D
    assert plan.lengths(nw)[1] >= 1 and plan.lengths(nw - 1)[1] == 0
    return nw


def rx_of(oversample):
    from tetraear.signal.wideband import WidebandReceiver
    return WidebandReceiver(oversample=oversample)


@pytest.fixture(scope="module")
def cap400():
    """(q [Nw, 2] int16, twin [Nw] complex64): several blocks per workgroup, a ragged last workgroup,
    an odd length."""
    from tetraear.signal.wideband import synth_wideband
    q = q16(synth_wideband(400_037, seed=5, snr_db=20)[0])
    return q, twin(q)


@pytest.mark.parametrize("oversample,form", FORMS)
def test_sc16_is_cf32_of_the_scaled_capture(cap400, oversample, form, monkeypatch):
    monkeypatch.setenv("TETRA_WB_ANALYSIS", form)
    from tetraear import _hip
    q, t = cap400
    rx = rx_of(oversample)
    y = rx.channelize(q)
    assert y.shape[1] == rx.plan.lengths(len(q))[1] and np.abs(y).max() > 0
    assert np.array_equal(y, rx.channelize(t))
    assert np.array_equal(rx.channelize(q, 1000), y[:, :1000])   # a partial row is the full row's prefix
    if oversample == 2:
        yo, om = rx.channelize_om(q)
        yt, omt = rx.channelize_om(t)
        assert np.array_equal(yo, y) and np.array_equal(yt, y) and np.array_equal(om, omt) and om.max() > 0
    n = min_nw(rx.plan)
    y1 = rx.channelize(q[:n])
    assert y1.shape == (rx.plan.M, rx.plan.lengths(n)[1]) and np.array_equal(y1, rx.channelize(t[:n]))
    c = _hip.ctx()
    for x, fmt in ((q, _hip.TETRA_SC16), (t, _hip.TETRA_CF32)):   # one sample fewer: no output to ask for
        assert c.lib.tetra_channelize_fmt(c.handle, rx.plan.c, _hip.ptr(x), fmt, n - 1, _hip.ptr(y1), 1) == E_INVALID


@pytest.mark.parametrize("oversample", [2, 4])
def test_conversion_edges(oversample):
    """Full scale both ways, -1, 0 and 1 on I and on Q in every combination (sign extension, I / Q
    order), at the shortest capture and at ~20 000 samples; and all zeros."""
    rx = rx_of(oversample)
    n0 = min_nw(rx.plan)
    for n in (n0, 20_003):
        i = np.arange(n)
        q = np.stack([EDGE[i % 5], EDGE[(i // 5) % 5]], axis=1)
        y = rx.channelize(q)
        assert np.abs(y).max() > 0 and np.array_equal(y, rx.channelize(twin(q))), n
        z = rx.channelize(np.zeros((n, 2), np.int16))
        assert z.shape == y.shape and not z.any()


@pytest.mark.parametrize("oversample", [2, 4])
def test_sc16_against_the_oracle(cap400, oversample):
    from test_wideband import Y_TOL
    q, t = cap400
    q, t = q[:100_003], t[:100_003]
    want = W.channelize(t.astype(np.complex128), W.design(oversample=oversample))
    y = rx_of(oversample).channelize(q)
    assert y.shape == want.shape
    assert np.abs(y - want).max() <= Y_TOL * np.abs(want).max()


@pytest.fixture(scope="module")
def chain():
    """The 1_120_000-sample capture at 30 dB (test_wideband.py's), its 16- and 12-bit forms with their
    twins, and the decodes the tests share."""
    from tetraear.signal.wideband import synth_wideband
    x, cells, kinds, payload, t0 = synth_wideband(1_120_000, seed=11, snr_db=30.0, cfo_max=300.0)
    q = {b: q16(x, b) for b in (16, 12)}
    return dict(x=x, cells=cells, payload=payload, q=q, t={b: twin(v) for b, v in q.items()})


@pytest.mark.parametrize("bits", [16, 12])
def test_decode_frames_equal(chain, bits):
    rx = rx_of(None)
    a = rx.decode(chain["q"][bits], chain["cells"])
    b = rx.decode(chain["t"][bits], chain["cells"])
    assert sum(len(f) for f in a) > 800 and canon(a) == canon(b)


@pytest.mark.parametrize("bits", [16, 12])
def test_decode_acquire_frames_equal(chain, bits):
    rx = rx_of(None)
    init = np.full(rx.plan.M, 3, np.uint32)
    fa, sa, ga = rx.decode_acquire(chain["q"][bits], init, mac=True, timebase=True)
    fb, sb, gb = rx.decode_acquire(chain["t"][bits], init, mac=True, timebase=True)
    assert sum(len(f) for f in fa) > 800 and canon(fa) == canon(fb)
    assert np.array_equal(sa, sb) and np.array_equal(ga, gb) and ga.sum() > 0


def _round_trip(x, cells, payload):
    """test_wideband_round_trip's count: (CRC-good blocks, blocks); every CRC-good one was sent."""
    from tetraear.core.etsi import EtsiLowerMac
    hard, soft, sym, ns = rx_of(None).demod(x)
    M, nchunk = ns.shape
    res = EtsiLowerMac().decode_batch(soft.reshape(M * nchunk, -1), hard.reshape(M * nchunk, -1), ns.reshape(-1),
                                      np.repeat(cells, nchunk))
    nblk = nok = 0
    for i, frames in enumerate(res):
        sent = {tuple(p) for bb in payload[i // nchunk] for p in bb}
        for f in frames:
            for b in f["blocks"]:
                nblk += 1
                if b["crc_ok"]:
                    nok += 1
                    assert tuple(np.pad(b["bits"], (0, 268 - len(b["bits"])))) in sent
    return nok, nblk


def test_round_trip_16_bit(chain):
    nok, nblk = _round_trip(chain["q"][16], chain["cells"], chain["payload"])
    print("round trip, 16-bit capture:", nok, "of", nblk)
    assert nblk >= 2 * 800
    assert nok / nblk > 0.97, (nok, nblk)


def test_round_trip_counts(chain):
    """The CRC-good counts of the unquantised and the 12-bit capture beside the 16-bit one's (DESIGN
    §5.19 records them): a quantised capture decodes only what was sent."""
    for name, x in (("unquantised", chain["x"]), ("12-bit", chain["q"][12])):
        nok, nblk = _round_trip(x, chain["cells"], chain["payload"])
        print("round trip,", name, "capture:", nok, "of", nblk)
        assert nblk >= 2 * 800 and nok > 0


def _collect(st, pieces):
    got = [[] for _ in range(st.M)]
    for p in pieces:
        for k, fr in enumerate(st.decode(p)):
            got[k].extend(fr)
    return got


CUTS = (0, 1_234_567, 1_300_001, 2_711_113, 3_300_000)


@pytest.fixture(scope="module")
def stream3():
    """The 3_300_000-sample capture quantised, its twin, the cells, and the frames of the complex64
    stream over the twin's pieces (uneven, one shorter than a chunk)."""
    from tetraear.signal import wideband as WB
    x, cells = WB.synth_wideband(3_300_000, seed=17, snr_db=25.0, cfo_max=300.0)[:2]
    q = q16(x)
    t = twin(q)
    ref = canon(_collect(WB.WidebandStream(cells), [t[a:b] for a, b in zip(CUTS, CUTS[1:])]))
    assert sum(len(f) for f in ref) > 2 * 800
    return q, t, cells, ref


def test_stream_on_int16_pieces(stream3):
    """WidebandStream on int16 pieces gives the frames of the complex64 stream on the twin pieces; its
    tail stays int16, and reset() empties it."""
    from tetraear.signal import wideband as WB
    q, t, cells, ref = stream3
    st = WB.WidebandStream(cells)
    got = [[] for _ in range(st.M)]
    for a, b in zip(CUTS, CUTS[1:]):
        for k, fr in enumerate(st.decode(q[a:b])):
            got[k].extend(fr)
        assert st.tail.dtype == np.int16 and len(st.tail) > 0
    assert canon(got) == ref
    st.reset()
    assert len(st.tail) == 0


def test_stream_on_alternating_formats(stream3):
    from tetraear.signal import wideband as WB
    q, t, cells, ref = stream3
    st = WB.WidebandStream(cells)
    mixed = _collect(st, [q[a:b] if i % 2 == 0 else t[a:b] for i, (a, b) in enumerate(zip(CUTS, CUTS[1:]))])
    assert st.tail.dtype == np.complex64 and canon(mixed) == ref


def _step_outputs(st, torch):
    ns, nb, nk = st.nsym.cpu(), st.nburst.cpu(), st.nblock.cpu()
    soft, hard, bursts, blocks, t1 = st.soft.cpu(), st.hard.cpu(), st.bursts.cpu(), st.blocks.cpu(), st.type1.cpu()
    n1 = {0: 268, 1: 124, 2: 60}
    return [ns, nb, nk, st.wf.cpu()] + [x for ch in range(st.C) for x in (
        soft[ch, :2 * max(int(ns[ch]) - 1, 0)], hard[ch, :max(int(ns[ch]) - 1, 0)], bursts[ch, :int(nb[ch])],
        blocks[ch, :int(nk[ch])])] + [t1[ch, j, :n1[int(blocks[ch, j, 0])]] for ch in range(st.C)
                                      for j in range(int(nk[ch]))]


def test_bench_step_sc16(monkeypatch):
    """BenchStep on device pointers with TETRA_WB_IQ=sc16, serial and in the three-stream pipeline,
    against a cf32 step on that capture / 32768: counts, soft and hard bits, bursts, blocks, type-1
    bits up to the counts, and the waterfall rows."""
    import torch
    from tetraear import _hip
    from tetraear.signal.wideband import BenchStep
    dev = torch.device("cuda", 0)
    monkeypatch.setenv("TETRA_WB_STAGES", "3")

    def run(iq, pipe, x=None):
        monkeypatch.setenv("TETRA_WB_IQ", iq)
        c = _hip.Context()
        c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
        st = BenchStep(c, 2_000_000, seed=3, device=dev)
        if x is not None:
            st.x.copy_(x)
        if pipe:
            st.pipeline()
        for _ in range(3):
            st()
        torch.cuda.synchronize(dev)
        return st

    s16 = run("sc16", False)
    assert s16.x.dtype == torch.int16 and s16.x.shape == (2_000_000, 2) and int(s16.x.abs().max()) > 16384
    cfg = s16.config(1)
    assert cfg["iq"] == "sc16" and s16.workload_key() in cfg["workload"]
    assert s16.stage_bytes()["wb_analysis"] == (4.0 + 16.0, "k_pfb_analysis1_sc16")
    want = _step_outputs(s16, torch)
    assert int(want[1].sum()) > 800 and s16.quality()["crc_ok"] > 0
    f32 = run("cf32", False, s16.x.to(torch.float32) / 32768)
    cf = f32.config(1)
    assert "iq" not in cf and f32.workload_key() in cf["workload"] and f32.workload_key() not in cfg["workload"]
    assert s16.workload_key() not in cf["workload"]
    assert f32.stage_bytes()["wb_analysis"] == (8.0 + 16.0, "k_pfb_analysis1")
    for st in (f32, run("sc16", True)):
        got = _step_outputs(st, torch)
        assert len(got) == len(want)
        for a, b in zip(want, got):
            assert torch.equal(a, b)
    monkeypatch.setenv("TETRA_WB_IQ", "int16")
    with pytest.raises(ValueError, match="TETRA_WB_IQ"):
        BenchStep(_hip.ctx(), 2_000_000, seed=3, device=dev)


@pytest.mark.parametrize("seed", range(8 * SCALE))
def test_sc16_random_cases(seed, monkeypatch):
    """Random length, design, analysis form, scale and host or device pointers: SC16 equals its twin."""
    import torch
    from tetraear import _hip
    from tetraear.signal.wideband import synth_wideband
    rng = np.random.default_rng(21000 + seed)
    oversample = int(rng.choice([2, 4]))
    form = str(rng.choice(["1", "2", "3", "4"] if oversample == 2 else ["1", "2"]))
    monkeypatch.setenv("TETRA_WB_ANALYSIS", form)
    rx = rx_of(oversample)
    n0 = min_nw(rx.plan)
    Nw = int(rng.integers(n0, n0 + 3000 if rng.uniform() < 0.3 else 300_000))
    x = synth_wideband(Nw, seed=22000 + seed, snr_db=float(rng.uniform(5, 30)), oversample=oversample)[0]
    bits = int(rng.integers(4, 17))
    q = q16(x, bits)
    t = twin(q)
    device = bool(rng.integers(2))
    case = (seed, oversample, form, Nw, bits, device)
    if not device:
        assert np.array_equal(rx.channelize(q), rx.channelize(t)), case
        return
    c = _hip.ctx()
    dev = torch.device("cuda", 0)
    n72 = rx.plan.lengths(Nw)[1]
    ys = []
    for a, fmt in ((q, _hip.TETRA_SC16), (t.view(np.float32).reshape(-1, 2), _hip.TETRA_CF32)):
        xd = torch.from_numpy(a).to(dev)
        yd = torch.zeros((rx.plan.M, n72, 2), dtype=torch.float32, device=dev)
        c.check(c.lib.tetra_channelize_fmt(c.handle, rx.plan.c, _hip.ptr(xd), fmt, Nw, _hip.ptr(yd), n72), "channelize")
        c.synchronize()
        ys.append(yd.cpu())
    assert torch.equal(ys[0], ys[1]) and bool(ys[0].any()), case
    assert np.array_equal(ys[0].numpy().view(np.complex64)[..., 0], rx.channelize(q)), case


def test_errors(cap400):
    """A format the channeliser does not take, and an SC16 device pointer off the 8-byte grid of its
    pair loads, are TETRA_E_INVALID with a message, nothing launched; the same samples on the grid go
    through."""
    import torch
    from tetraear import _hip
    q, t = cap400
    rx = rx_of(None)
    c = _hip.ctx()
    n = 40_001
    n72 = rx.plan.lengths(n)[1]
    y = np.zeros((rx.plan.M, n72), np.complex64)
    om = np.zeros((rx.plan.M, -(-n72 // rx.plan.c.up), 4), np.float32)
    for fmt in (_hip.TETRA_CF64, _hip.TETRA_F32, 7, -1):
        assert c.lib.tetra_channelize_fmt(c.handle, rx.plan.c, _hip.ptr(t), fmt, n, _hip.ptr(y), n72) == E_INVALID
        assert b"TETRA_CF32 or TETRA_SC16" in c.lib.tetra_last_error(c.handle)
        assert c.lib.tetra_channelize_om_fmt(c.handle, rx.plan.c, _hip.ptr(t), fmt, n, _hip.ptr(y), n72,
                                             _hip.ptr(om)) == E_INVALID
    assert not y.any()
    dev = torch.device("cuda", 0)
    qd = torch.from_numpy(q[:n + 1]).to(dev)
    yd = torch.zeros((rx.plan.M, n72, 2), dtype=torch.float32, device=dev)
    off = qd[1:]
    assert off.data_ptr() % 8 == 4
    assert c.lib.tetra_channelize_fmt(c.handle, rx.plan.c, _hip.ptr(off), _hip.TETRA_SC16, n, _hip.ptr(yd), n72) == E_INVALID
    assert b"8-byte" in c.lib.tetra_last_error(c.handle)
    c.synchronize()
    assert not bool(yd.any())
    on = off.clone()
    assert on.data_ptr() % 8 == 0
    c.check(c.lib.tetra_channelize_fmt(c.handle, rx.plan.c, _hip.ptr(on), _hip.TETRA_SC16, n, _hip.ptr(yd), n72), "channelize")
    c.synchronize()
    assert np.array_equal(yd.cpu().numpy().view(np.complex64)[..., 0], rx.channelize(q[1:n + 1]))
    assert np.array_equal(rx.channelize(q[1:n + 1]), rx.channelize(t[1:n + 1]))   # a host array may sit anywhere
