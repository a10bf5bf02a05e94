"""GPU parity of the ETSI chain over the whole plan space (tests/_etsi_rates.py RATES), not only at
the reference GUI's slider rates: the generic channel filter k_chanfilt_g at every q1 in 1..13, with
stage 1 absent, with no resampling, with the largest prototype and the widest stage-2 window, at the
tile boundaries of each plan's own stride and at the plan limits the ABI accepts; the whole chain and
the streaming receiver at the extremes.

Bar: bit-identical to the oracle (np.array_equal; SC16 against the oracle on its 1/32768-scaled
samples).  One cf32 case per rate is also held to the float64 restatement of tests/_etsi_rates.py,
which shares no code or operation order with the oracle, within the a-priori rounding bound.
"""
import numpy as np
import pytest

import etsi as E

import _etsi_rates as R

pytestmark = pytest.mark.gpu

INVALID = -1   # TETRA_E_INVALID


def _chanfilt(plan, x, fmt, M2):
    """tetra_etsi_chanfilt_fmt on [C, N] complex64 or [C, N, 2] int16 -> (rc, y [C, M2]); y is filled
    with a sentinel first, so a refused call shows that nothing was written."""
    from tetraear import _hip
    c = _hip.ctx()
    y = np.full((x.shape[0], max(M2, 1)), np.complex64(7 + 7j))
    x = np.ascontiguousarray(x)
    rc = c.lib.tetra_etsi_chanfilt_fmt(c.handle, plan, _hip.ptr(x), fmt, x.shape[0], x.shape[1], _hip.ptr(y))
    return rc, y


@pytest.mark.parametrize("fs", list(R.RATES))
def test_chanfilt_over_the_plan_space(fs):
    """k_chanfilt_g at one rate of the table, C = 3 channels (ch = blockIdx / ntiles), cf32 and SC16, at
    six lengths around the plan's own tile stride S1 = 512 - window: M1 = S1, S1 + 1, 512, 2 S1,
    2 S1 + 1 and a ragged third tile.  Every channel bit-identical to the oracle; the longest cf32 case
    also within the rounding bound of the float64 restatement."""
    from tetraear import _hip
    from tetraear.signal.etsi import etsi_plan, lengths
    q1, L1, up, down, Lp, win = R.RATES[fs]
    plan, orc = etsi_plan(fs), E.Receiver(fs)
    assert (plan.q1, plan.L1, plan.up, plan.down, plan.Lp) == (q1, L1, up, down, Lp)
    C = 3
    ns = R.chanfilt_lengths(q1, L1, win)
    sig = np.stack([R.signal(E, fs, max(ns), seed=fs // 1000 + ch) for ch in range(C)])
    q, xq = R.to_sc16(sig)
    for n in ns:
        M1, M2, _ = lengths(plan, n)
        assert (M1, M2) == R.plan_lengths(q1, L1, up, down, Lp, n)
        want = [orc.chanfilt(xq[ch, :n]) for ch in range(C)]
        for name, x, fmt in (("cf32", xq[:, :n], _hip.TETRA_CF32), ("sc16", q[:, :n], _hip.TETRA_SC16)):
            rc, y = _chanfilt(plan, x, fmt, M2)
            assert rc == 0, (fs, n, name)
            for ch in range(C):
                assert len(want[ch]) == M2 and np.array_equal(y[ch], want[ch]), (fs, n, name, ch)
            if name == "cf32":
                ycf = y
    d = orc.d   # the last (longest, three-tile) cf32 case, its last channel
    R.check_against_f64(ycf[C - 1], xq[C - 1, :ns[-1]], d["h1"], d["hp"], q1, up, down, fs)


def _custom_plan(q1, L1, up, down, Lp, seed):
    """A plan the designer never makes: the integers as given, seeded random taps."""
    from tetraear import _hip
    from tetraear.signal.etsi import etsi_plan
    p = _hip.EtsiPlan.from_buffer_copy(etsi_plan(1.8e6))
    rng = np.random.default_rng(seed)
    h1 = rng.uniform(-1, 1, 64).astype(np.float32)
    hp = rng.uniform(-1, 1, 4096).astype(np.float32)
    p.q1, p.L1, p.up, p.down, p.Lp, p.flags = q1, L1, up, down, Lp, 0
    np.ctypeslib.as_array(p.h1)[:] = h1
    np.ctypeslib.as_array(p.hp)[:] = hp
    return p, h1[:max(0, min(L1, 64))].copy(), hp[:max(0, min(Lp, 4096))].copy()


def _eo_chanfilt(x, h1, q1, hp, up, down):
    """eo_chanfilt through the oracle library on given taps."""
    xv = np.ascontiguousarray(x, np.complex64).view(np.float32)
    N, L1, Lp = len(xv) // 2, len(h1), len(hp)
    M1 = (N - L1) // q1 + 1
    x1 = np.zeros(2 * M1, np.float32)
    y = np.zeros(2 * (M1 * up // down + 2), np.float32)
    M2 = E.lib().eo_chanfilt(xv, N, np.ascontiguousarray(h1), L1, q1, np.ascontiguousarray(hp), Lp, up, down, x1, y)
    return y[:2 * M2].view(np.complex64).copy()


@pytest.mark.parametrize("q1,L1,up,down,Lp", [
    (13, 64, 3, 16, 513),     # the longest stage 1 at the largest decimation: the tile's input fills xin
    (3, 14, 17, 40, 4096),    # the longest prototype (window 242)
    (2, 10, 16, 45, 4049),    # a window of exactly 255: the smallest stride, S1 = 257
    (5, 24, 17, 5, 801),      # up > down: several outputs per stage-1 sample
])
def test_chanfilt_custom_plans_at_the_kernel_limits(q1, L1, up, down, Lp):
    """Plans at the limits etsi_generic_unsupported accepts, random taps, noise input on the SC16 grid:
    equal to eo_chanfilt on every channel in both formats, at 2 S1 + 1 stage-1 outputs and at a ragged
    third tile."""
    from tetraear import _hip
    from tetraear.signal.etsi import lengths
    plan, h1, hp = _custom_plan(q1, L1, up, down, Lp, seed=Lp + up)
    win = (Lp - 1) // up + 2
    assert win < 256
    C = 3
    rng = np.random.default_rng(q1 * 1000 + L1)
    for n in R.chanfilt_lengths(q1, L1, win)[-2:]:
        q, xq = R.to_sc16(0.25 * (rng.standard_normal((C, n)) + 1j * rng.standard_normal((C, n))))
        M1, M2, _ = lengths(plan, n)
        assert M2 > 0 and M1 > 2 * (512 - win)
        want = [_eo_chanfilt(xq[ch], h1, q1, hp, up, down) for ch in range(C)]
        for name, x, fmt in (("cf32", xq, _hip.TETRA_CF32), ("sc16", q, _hip.TETRA_SC16)):
            rc, y = _chanfilt(plan, x, fmt, M2)
            assert rc == 0, (n, name)
            for ch in range(C):
                assert len(want[ch]) == M2 and np.array_equal(y[ch], want[ch]), (n, name, ch)


@pytest.mark.parametrize("q1,L1,up,down,Lp", [
    (14, 64, 3, 16, 513),     # q1 = 14
    (13, 65, 3, 16, 513),     # L1 = 65
    (3, 14, 17, 40, 4097),    # Lp = 4097
    (2, 10, 16, 45, 4065),    # a window of 256
    (5, 24, 0, 5, 801),       # up = 0
])
def test_chanfilt_refuses_plans_past_the_kernel_limits(q1, L1, up, down, Lp):
    """TETRA_E_INVALID before any launch: nothing is written to y."""
    from tetraear import _hip
    plan, _, _ = _custom_plan(q1, L1, up, down, Lp, seed=1)
    x = np.zeros((3, 8192), np.complex64)
    for fmt, xx in ((_hip.TETRA_CF32, x), (_hip.TETRA_SC16, np.zeros((3, 8192, 2), np.int16))):
        rc, y = _chanfilt(plan, xx, fmt, 4096)
        assert rc == INVALID and np.all(y == np.complex64(7 + 7j)), (fmt, rc)


def _kernel_name(plan, N):
    import ctypes
    from tetraear import _hip
    c = _hip.ctx()
    name = ctypes.create_string_buffer(64)
    lds = ctypes.c_int64(0)
    c.check(c.lib.tetra_etsi_kernel_info(c.handle, plan, _hip.TETRA_CF32, N, 1, name, 64, ctypes.byref(lds)),
            "kernel_info")
    return name.value.decode()


@pytest.mark.parametrize("fs", [72_000, 127_000, 1_000_000, 2_750_000, 3_948_000, 4_953_000])
def test_whole_chain_at_the_extremes(fs):
    """Two channels of 60 ms (four bursts) at 18 dB: the demod's symbols, soft bits, hard dibits and
    nsym bit-identical to the oracle, SC16 equal to cf32, the lower MAC equal to the oracle's, at
    least one CRC-good block per channel and every CRC-good block a transmitted payload."""
    from tetraear.signal.etsi import EtsiReceiver, synth
    from tetraear.core.etsi import EtsiLowerMac
    C = 2
    N = 2 * int(round(0.060 * fs / 2))
    iq, cells, kinds, payload, t0 = synth(C, N, fs=fs, seed=fs // 1000 + 3, snr_db=18.0)
    q, xq = R.to_sc16(iq)
    rx, orc = EtsiReceiver(fs), E.Receiver(fs)
    assert _kernel_name(rx.plan, N) == "k_chanfilt_g"
    hard, soft, sym, ns = rx.demod_batch(xq)
    for a, b in zip((hard, soft, sym, ns), rx.demod_batch(q)):
        assert np.array_equal(a, b), fs
    res = EtsiLowerMac().decode_batch(soft, hard, ns, cells)
    for ch in range(C):
        so, sbo, ho, _ = orc.demod(xq[ch])
        n = int(ns[ch])
        assert n == len(so) and n > 1000, (fs, ch, n, len(so))
        assert np.array_equal(sym[ch, :n], so), (fs, ch)
        assert np.array_equal(soft[ch, :2 * (n - 1)], sbo) and np.array_equal(hard[ch, :n - 1], ho), (fs, ch)
        want = orc.lower_mac(sbo, ho, int(cells[ch]))
        got = res[ch]
        assert [(f["position"], f["burst_kind"]) for f in got] == [(s, k) for s, k, _ in want], (fs, ch)
        sent = {tuple(p) for bb in payload[ch] for p in bb}
        nok = 0
        for f, (_, _, dec) in zip(got, want):
            assert len(f["blocks"]) == len(dec), (fs, ch)
            for b, (kind, bits, ok) in zip(f["blocks"], dec):
                assert b["crc_ok"] == ok and np.array_equal(b["bits"], bits), (fs, ch)
                if ok:
                    nok += 1
                    assert tuple(np.pad(b["bits"], (0, 268 - len(b["bits"])))) in sent, (fs, ch)
        assert nok >= 1, (fs, ch)


STREAM_CHUNKS = [50000, 77778, 131072, 3000, 2, 40000]


@pytest.mark.parametrize("fs", [2_750_000, 4_953_000, 127_000, 2_100_000])
def test_stream_at_the_rates_that_need_long_history(fs):
    """EtsiStream and SignalProcessor(mode='etsi').process chunk by chunk against the oracle stream, at
    the two rates whose windows re-read more than 4096 samples (2.75 MSps: an odd period doubled;
    4.953 MSps: the most of any plannable rate, 5604 on these chunks), at 127 kHz (q1 = 1, the largest
    prototype) and at 2.1 MSps (an odd period among the slider rates, the control).  No call raises.
    The first new output of a window lies up to MARGIN + 2 up outputs into it (yoff = 73 at 2.75 MSps
    and 126 at 127 kHz on these chunks, against 17 at 2.1 MSps): k_timing's LDS ring has to start
    there, not at the window's first output."""
    _stream_vs_oracle(fs)


@pytest.mark.parametrize("ring", [0, 2])
def test_stream_far_first_output_every_timing_form(ring, monkeypatch):
    """The same at 127 kHz with k_timing's other forms (TETRA_TIMING_RING: no ring, two blocks ahead)."""
    monkeypatch.setenv("TETRA_TIMING_RING", str(ring))
    _stream_vs_oracle(127_000)


def _stream_vs_oracle(fs):
    from tetraear.signal import SignalProcessor
    from tetraear.signal.etsi import EtsiStream, synth
    C = 2
    iq = synth(C, sum(STREAM_CHUNKS), fs=fs, seed=fs // 1000 + 11, snr_db=18.0)[0]
    want = [E.Stream(fs) for _ in range(C)]
    st, sp = EtsiStream(fs, C), SignalProcessor(fs, mode="etsi")
    at = 0
    for k, n in enumerate(STREAM_CHUNKS):
        x = iq[:, at:at + n]
        at += n
        hard, soft, sym, ns = st.demod(x)
        for ch in range(C):
            w = want[ch].push(x[ch])
            m = int(ns[ch])
            assert m == len(w["symbols"]), (fs, k, ch, m, len(w["symbols"]))
            assert np.array_equal(sym[ch, :m], w["symbols"]), (fs, k, ch)
            assert np.array_equal(hard[ch, :max(m - 1, 0)], w["hard"]), (fs, k, ch)
            assert np.array_equal(soft[ch, :2 * max(m - 1, 0)], w["soft"]), (fs, k, ch)
            if ch == 0:
                h0 = sp.process(x[0])
                assert np.array_equal(sp.symbols, w["symbols"]) and np.array_equal(np.asarray(h0), w["hard"]), (fs, k)
                assert np.array_equal(h0.soft_bits, w["soft"]), (fs, k)
    assert (np.asarray(st.track["acquired"]) == 1).all()
