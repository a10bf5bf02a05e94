"""Wideband chain on SC16 captures, the host side (no device): WidebandStream's tail over int16
pieces, the int16 input's validation, and the bench step's TETRA_WB_IQ."""
import numpy as np
import pytest

from _wb_sc16 import q16, shift_of, twin


def _stub(monkeypatch, WB, p, seen):
    """WidebandReceiver.decode stubbed as in test_wideband_stream_host_logic: a burst every 1020
    stream outputs on two carriers; records each buffer it is handed."""
    box = {}

    def fake_decode(self, x, cells):
        _, n72 = p.lengths(len(x))
        seen.append(x)
        y0 = box["st"].y0
        out = [[], []]
        for k in range(2):
            a0 = (y0 - 500 * k + 1019) // 1020 * 1020 + 500 * k
            for a in range(a0, y0 + n72 - 1020, 1020):
                out[k].append({"sample": a - y0 + (3 if len(seen) % 2 else 0), "blocks": []})
        return out

    monkeypatch.setattr(WB.WidebandReceiver, "decode", fake_decode)
    st = WB.WidebandStream(np.zeros(p.M, np.uint32))
    st.M = 2
    st.last = np.full(2, -(1 << 62), np.int64)
    box["st"] = st
    return st


def test_stream_keeps_an_int16_tail(monkeypatch):
    """int16 pieces: the buffers reach decode as int16, the tail stays int16 (and holds the stream's
    last samples), and the period / position invariants are those of the complex64 stream."""
    from tetraear.signal import wideband as WB
    p = WB.wb_plan()
    seen = []
    st = _stub(monkeypatch, WB, p, seen)
    assert len(st.tail) == 0
    rng = np.random.default_rng(1)
    whole = rng.integers(-32768, 32768, size=(5_005_002, 2), dtype=np.int16)
    got = [[], []]
    total = 0
    for n in (700_000, 5_000, 1_300_000, 2_000_003, 999_999):
        before = len(st.tail)
        fr = st.decode(whole[total:total + n])
        total += n
        assert st.tail.dtype == np.int16 and st.tail.shape == (len(st.tail), 2)
        assert np.array_equal(st.tail, whole[total - len(st.tail):total])
        assert (total - len(st.tail)) % st.per == 0
        assert st.y0 == (total - len(st.tail)) // st.per * st.ups
        _, n72 = p.lengths(before + n)
        if n72 > st.CARRY_Y:
            assert p.lengths(len(st.tail))[1] >= st.CARRY_Y - st.ups
        for k in range(2):
            got[k].extend(f["stream_sample"] for f in fr[k])
    assert all(b.dtype == np.int16 and b.ndim == 2 for b in seen)
    n72 = p.lengths(total)[1]
    for k in range(2):
        want = list(range(500 * k, n72 - 1020, 1020))
        assert len(got[k]) == len(want) and all(0 <= g - w <= 3 for g, w in zip(got[k], want)), k
    st.reset()
    assert len(st.tail) == 0 and st.y0 == 0


def test_stream_converts_the_tail_on_a_format_switch(monkeypatch):
    """Pieces that change format: whichever of tail and piece is int16 becomes x / 32768 exactly, so
    every buffer holds the samples the complex64 stream's does."""
    from tetraear.signal import wideband as WB
    p = WB.wb_plan()
    seen, seen_ref = [], []
    st = _stub(monkeypatch, WB, p, seen)
    rng = np.random.default_rng(2)
    whole = rng.integers(-32768, 32768, size=(3_000_000, 2), dtype=np.int16)
    ref = twin(whole)
    cuts = (0, 700_001, 1_400_000, 2_100_003, 3_000_000)
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        st.decode(whole[a:b] if i % 2 == 0 else ref[a:b])
        assert st.tail.dtype == (np.int16 if i == 0 else np.complex64)
    tails = [len(st.tail), st.y0]
    st2 = _stub(monkeypatch, WB, p, seen_ref)
    for a, b in zip(cuts, cuts[1:]):
        st2.decode(ref[a:b])
    assert tails == [len(st2.tail), st2.y0]
    assert len(seen) == len(seen_ref) == 4
    for i, (g, w) in enumerate(zip(seen, seen_ref)):
        g = twin(g) if g.dtype == np.int16 else g
        assert g.dtype == np.complex64 and np.array_equal(g, w), i


@pytest.mark.parametrize("bad", [np.zeros(10, np.int16), np.zeros((10, 3), np.int16), np.zeros((2, 10, 2), np.int16),
                                 np.zeros((2, 10), np.int16)])
def test_int16_input_shape_is_checked(bad):
    from tetraear.signal import wideband as WB
    rx = WB.WidebandReceiver()
    for call in (rx.channelize, rx.channelize_om, rx.demod, lambda x: rx.decode(x, np.zeros(800, np.uint32)),
                 lambda x: rx.decode_acquire(x, np.full(800, 3, np.uint32)),
                 WB.WidebandStream(np.zeros(800, np.uint32)).decode):
        with pytest.raises(ValueError, match=r"SC16 input must be \[Nw, 2\] int16"):
            call(bad)


def test_capture_formats():
    from tetraear import _hip
    from tetraear.signal import wideband as WB
    q = np.arange(40, dtype=np.int16).reshape(20, 2)
    a, fmt = WB._capture(q[::2])   # not contiguous: copied, still int16
    assert fmt == _hip.TETRA_SC16 and a.dtype == np.int16 and a.flags.c_contiguous and np.array_equal(a, q[::2])
    a, fmt = WB._capture(np.arange(5, dtype=np.complex128))
    assert fmt == _hip.TETRA_CF32 and a.dtype == np.complex64
    assert np.array_equal(WB.sc16_to_cf32(q), twin(q))


def test_q16_scale():
    x = (np.array([0.5 + 7.9j, -3.0 - 0.25j, 1e-3])).astype(np.complex64)
    assert shift_of(x) == 3 and shift_of(x / 8) == 0 and shift_of(np.array([32767 / 32768], np.complex64)) == 0
    assert shift_of(np.array([1.0], np.complex64)) == 1
    q = q16(x)
    assert q.dtype == np.int16 and q[0].tolist() == [2048, 32358] and q[1].tolist() == [-12288, -1024]
    assert np.abs(q16(x, 12)).max() <= 2047


def test_bench_step_iq_env(monkeypatch):
    """TETRA_WB_IQ as far as it goes without a device: cf32 by default, sc16, anything else raises (as
    TETRA_WB_CELLS and TETRA_WB_MAC do); the full-scale shift is the smallest that fits."""
    from tetraear.signal.wideband import BenchStep
    monkeypatch.delenv("TETRA_WB_IQ", raising=False)
    assert BenchStep.iq_format() == "cf32"
    monkeypatch.setenv("TETRA_WB_IQ", "sc16")
    assert BenchStep.iq_format() == "sc16"
    for bad in ("SC16", "cf64", "", "int16"):
        monkeypatch.setenv("TETRA_WB_IQ", bad)
        with pytest.raises(ValueError, match="TETRA_WB_IQ"):
            BenchStep.iq_format()
    with pytest.raises(ValueError, match="TETRA_WB_IQ"):
        BenchStep(None, 2_000_000, seed=1, device=None)   # refused before anything touches a device
    assert [BenchStep.sc16_shift(p) for p in (0.0, 0.5, 32767 / 32768, 1.0, 1.99, 2.0, 37.2)] == [0, 0, 0, 1, 1, 2, 6]
