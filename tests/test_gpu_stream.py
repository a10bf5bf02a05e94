"""GPU parity of the streaming ETSI receiver (tetra_etsi_stream_window + tetra_demod_etsi_stream +
tetra_lmac_etsi_stream) against its CPU restatement oracle/etsi.py Stream, chunk after chunk of one
continuous capture (the reference's capture loops stream 128 Ki chunks,
/root/reference/tetraear/ui/modern.py:1901-1919, continuous_capture.py:20).

Bar: bit-identical -- per chunk the symbols (the carried one first), soft bits, hard dibits, the burst
positions (relative to the chunk, negative across the seam), kinds, decoded type-1 bits, CRC flags and
the acquired cells; and on the synthesised capture >= 99 % of the bursts on air after the first chunk
decoded.  Parity unpinned against the reference (it has no ETSI chain).
"""
import ctypes

import numpy as np
import pytest

import etsi as E

pytestmark = pytest.mark.gpu

L = 131072


def _oracle_chunks(iq, fs, sizes, cells=None, fmt="cf32"):
    """The oracle stream of each channel over the chunk sequence: per chunk per channel its dict."""
    C = iq.shape[0]
    streams = [E.Stream(fs, cell_init=None if cells is None else int(cells[ch])) for ch in range(C)]
    out = []
    for at, n in sizes:
        out.append([streams[ch].push(iq[ch, at:at + n]) for ch in range(C)])
    return out


def _chunk_plan(n_total, sizes):
    out, at, i = [], 0, 0
    while at < n_total:
        n = min(sizes[i % len(sizes)], n_total - at)
        n -= n % 2
        if n == 0:
            break
        out.append((at, n))
        at += n
        i += 1
    return out


def _compare(k, got_demod, got_frames, want, C):
    hard, soft, sym, ns = got_demod
    for ch in range(C):
        w = want[ch]
        n = int(ns[ch])
        case = (k, ch)
        assert n == len(w["symbols"]), case + (n, len(w["symbols"]))
        assert np.array_equal(sym[ch, :n], w["symbols"]), case
        assert np.array_equal(hard[ch, :max(n - 1, 0)], w["hard"]), case
        assert np.array_equal(soft[ch, :2 * max(n - 1, 0)], w["soft"]), case
        if got_frames is None:   # the demod alone
            continue
        got = got_frames[ch]
        assert [(f["position"], f["burst_kind"]) for f in got] == [(p, kd) for p, kd, _ in w["bursts"]], case
        for f, (_, _, dec) in zip(got, w["bursts"]):
            assert len(f["blocks"]) == len(dec), case
            for b, (kind, bits, ok) in zip(f["blocks"], dec):
                assert b["crc_ok"] == ok and np.array_equal(b["bits"], bits), case


@pytest.mark.parametrize("sizes,acquire", [([L], False), ([L], True), ([50000, 77778, L, 3000], False)])
def test_stream_bit_identical_to_oracle(sizes, acquire):
    from tetraear.signal.etsi import EtsiStream, synth
    from tetraear.core.etsi import EtsiLowerMac
    C, K = 6, 6
    iq, cells, kinds, payload, t0 = synth(C, K * L, seed=31, snr_db=16.0, cfo_max=600.0)
    plan = _chunk_plan(K * L, sizes)
    want = _oracle_chunks(iq, 2.4e6, plan, None if acquire else cells)
    st, lm = EtsiStream(2.4e6, C), EtsiLowerMac()
    for k, (at, n) in enumerate(plan):
        d = st.demod(iq[:, at:at + n])
        frames = lm.decode_stream(d[1], d[0], d[3], None if acquire else cells)
        _compare(k, d, frames, want[k], C)
        if acquire:
            assert [int(v) for v in lm.cell_state] == [want[k][ch]["cell"] for ch in range(C)], k
    assert (np.asarray(st.track["acquired"]) == 1).all()


def _profile_stages(c):
    """The stage names the context's profile recorded since the previous read."""
    names = ctypes.create_string_buffer(4096)
    ms, cnt, n = (ctypes.c_double * 64)(), (ctypes.c_int64 * 64)(), ctypes.c_int()
    c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    return {s.decode() for s in names.raw.split(b"\0")[:n.value]}


_DEMOD_STAGES = {"etsi_demod", "etsi_chanfilt", "etsi_timing"}
_LAUNCHES = {"skip": set(), "fused": {"etsi_demod"}, "pair": {"etsi_chanfilt", "etsi_timing"}}


@pytest.mark.parametrize("fmt", ["cf32", "sc16"])
@pytest.mark.parametrize("sizes,paths", [
    ([40, 50002, 50000, 3000], ["skip", "fused", "fused", "fused"]),
    ([134410, 134408], ["pair", "pair"]),
    ([131072, 131072], ["fused", "fused"]),
    ([131072, 131072], {"pad": 2, "cf32": ["fused", "fused"], "sc16": ["fused", "pair"]}),
])
def test_stream_every_demod_path_vs_oracle(sizes, paths, fmt):
    """Every launch path of tetra_demod_etsi_stream, chunk by chunk against the oracle stream (nsym,
    symbols, hard dibits and soft bits bit-identical; SC16 against the oracle on its 1/32768-scaled
    samples), and the path each chunk took from the profile's stage names:
    [40, ...]: a first window shorter than the filter (M2 <= 0: k_track_skip, nsym = 0, no demod
    stage), then windows of W = 2 (mod 4) samples -- SC16 leaves the per-wave kernel for
    k_chanfilt<uint2> fused with a carried track, cf32 stays per-wave;
    [134410, 134408]: M2 = 4000 > YLDS in the first window and more in the second -- the unfused
    k_chanfilt + k_timing pair with track, yoff > 0 and an acquired loop (SC16 rows not a multiple
    of four samples);
    [131072, 131072]: the per-wave fused kernel for both formats;
    the same with pad = 2: the windows (W = 0 mod 4: 131072, then 132444) lie in rows of pitch
    W + 2 = 2 (mod 4), so SC16's rows are not whole 16-B groups and it takes k_chanfilt -- fused for
    the first window, and for the second (M2 = 3940, 988 symbol rows: 4928 > the 4920 float2 of
    k_chanfilt<uint2>'s LDS, where the per-wave kernel would still fuse) the pair; cf32 stays
    per-wave.  The stage names do not tell the two fused kernels apart (both record etsi_demod), and
    tetra_etsi_kernel_info names a kernel for ld = N only: in this row it is the second window's pair
    that shows the pitch kept SC16 off the per-wave kernel; the first pins k_chanfilt<uint2>'s fused
    results on such rows."""
    from tetraear import _hip
    from tetraear.signal.etsi import EtsiStream, synth
    pad = 0
    if isinstance(paths, dict):   # a row with a row pitch of its own and the paths per format
        pad, paths = paths["pad"], paths[fmt]
    C, total = 2, sum(sizes)
    iq = synth(C, total, seed=67, snr_db=18.0, cfo_max=600.0)[0]
    inp = iq
    if fmt == "sc16":
        inp = np.stack([np.round(iq.real * 32768), np.round(iq.imag * 32768)], -1).clip(-32768, 32767).astype(np.int16)
        iq = (inp[..., 0].astype(np.float32) / 32768 + 1j * (inp[..., 1].astype(np.float32) / 32768)).astype(np.complex64)
    plan = _chunk_plan(total, sizes)
    assert [n for _, n in plan] == sizes
    want = _oracle_chunks(iq, 2.4e6, plan)
    st, c = EtsiStream(2.4e6, C), _hip.ctx()
    c.check(c.lib.tetra_profile(c.handle, 1), "tetra_profile")
    try:
        _profile_stages(c)   # drop earlier records
        for k, (at, n) in enumerate(plan):
            d = st.demod(inp[:, at:at + n], row_pad=pad)
            assert _profile_stages(c) & _DEMOD_STAGES == _LAUNCHES[paths[k]], (k, paths[k])
            if paths[k] == "skip":
                assert not d[3].any()
            _compare(k, d, None, want[k], C)
    finally:
        c.check(c.lib.tetra_profile(c.handle, 0), "tetra_profile")
    assert (np.asarray(st.track["acquired"]) == 1).all()


def test_stream_decodes_every_burst_on_air():
    """8 consecutive 128 Ki chunks of 32 channels, cells acquired: the bursts decoded per channel-chunk
    after the first chunk are >= 99 % of those on air (3.86 per chunk), the blocks >= 97 % CRC-good."""
    from tetraear.signal.etsi import EtsiStream, synth
    from tetraear.core.etsi import EtsiLowerMac
    C, K = 32, 8
    iq, cells, kinds, payload, t0 = synth(C, K * L, seed=41, snr_db=18.0, cfo_max=600.0)
    st, lm = EtsiStream(2.4e6, C), EtsiLowerMac()
    nb = nblk = nok = 0
    for k in range(K):
        hard, soft, sym, ns = st.demod(iq[:, k * L:(k + 1) * L])
        frames = lm.decode_stream(soft, hard, ns)
        if k == 0:
            continue
        for ch in range(C):
            nb += len(frames[ch])
            for f in frames[ch]:
                nblk += len(f["blocks"])
                nok += sum(b["crc_ok"] for b in f["blocks"])
    on_air = C * (K - 1) * L / 34000   # one 255-symbol slot = 34000 samples at 2.4 MSps
    assert nb >= 0.99 * on_air, (nb, on_air)
    assert nok >= 0.97 * nblk, (nok, nblk)
    assert sum(int(v) == int(c) for v, c in zip(lm.cell_state, cells)) >= 0.9 * C


def test_sc16_stream_equals_cf32_stream():
    from tetraear.signal.etsi import EtsiStream, synth
    C, K = 4, 4
    iq, cells = synth(C, K * L, seed=43, snr_db=18.0)[:2]
    q = np.stack([np.rint(iq.real * 32768), np.rint(iq.imag * 32768)], -1).clip(-32768, 32767).astype(np.int16)
    a, b = EtsiStream(2.4e6, C), EtsiStream(2.4e6, C)
    for k in range(K):
        ra = a.demod(iq[:, k * L:(k + 1) * L])
        rb = b.demod(q[:, k * L:(k + 1) * L])
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y), k


def test_stream_mixed_formats_continue_in_cf32():
    """Chunks of one stream in different formats -- SC16, then cf32, then SC16 with the AFC mixer on
    (which takes cf32) -- decode as the all-cf32 stream of the same samples does (SC16 -> cf32 is
    exact), instead of failing."""
    from tetraear.signal.etsi import EtsiStream, synth
    C, K = 2, 4
    iq = synth(C, K * L, seed=45, snr_db=18.0)[0]
    q = np.stack([np.rint(iq.real * 32768), np.rint(iq.imag * 32768)], -1).clip(-32768, 32767).astype(np.int16)
    f = (q[..., 0].astype(np.float32) / 32768 + 1j * (q[..., 1].astype(np.float32) / 32768)).astype(np.complex64)
    offs = [None, None, [100.0, -50.0], None]
    a, b = EtsiStream(2.4e6, C), EtsiStream(2.4e6, C)
    for k in range(K):
        sl = slice(k * L, (k + 1) * L)
        ra = a.demod(f[:, sl], offs[k])
        rb = b.demod(f[:, sl] if k == 1 else q[:, sl], offs[k])
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y), k


@pytest.mark.parametrize("fs", [1.8e6, 2.1e6])
def test_stream_other_rates_vs_oracle(fs):
    """The generic-rate chain (k_chanfilt_g + k_timing) streams the same way."""
    from tetraear.signal.etsi import EtsiStream, synth
    from tetraear.core.etsi import EtsiLowerMac
    C = 3
    n = int(L * fs / 2.4e6) // 2 * 2
    iq, cells = synth(C, 5 * n, fs=fs, seed=47, snr_db=18.0)[:2]
    plan = _chunk_plan(5 * n, [n])
    want = _oracle_chunks(iq, fs, plan, cells)
    st, lm = EtsiStream(fs, C), EtsiLowerMac()
    for k, (at, m) in enumerate(plan):
        d = st.demod(iq[:, at:at + m])
        _compare(k, d, lm.decode_stream(d[1], d[0], d[3], cells), want[k], C)


def test_resident_capture_windows_in_place():
    """A capture resident on the device as [C][K N] rows streamed in place (ld = K N, the window a
    pointer into the row: the bench's layout) equals the host-window path, and the lower MAC writing
    its tail into the next buffer of a double-buffered pair equals it writing into its own rows."""
    import torch
    from tetraear import _hip
    from tetraear.signal.etsi import EtsiStream, etsi_plan, lengths, stream_window, synth, TRACK, RESERVE
    C, K = 5, 4
    iq, cells = synth(C, K * L, seed=53, snr_db=18.0)[:2]
    host = EtsiStream(2.4e6, C)
    dev = torch.from_numpy(iq.view(np.float32).reshape(C, K * L, 2).copy()).cuda()
    plan = etsi_plan(2.4e6)
    c = _hip.ctx()
    track = torch.zeros(C * TRACK.itemsize // 4, dtype=torch.int32, device="cuda")
    x_total = y_done = 0
    _, M2max, smx = lengths(plan, L + 4096)
    stride = RESERVE + smx + 1
    bufs = [(torch.zeros((C, stride, 2), dtype=torch.float32, device="cuda"),
             torch.zeros((C, 2 * stride), dtype=torch.int8, device="cuda"),
             torch.zeros((C, stride), dtype=torch.uint8, device="cuda"),
             torch.zeros(C, dtype=torch.int32, device="cuda")) for _ in range(2)]
    lead = torch.full((C,), 2 * RESERVE, dtype=torch.int32, device="cuda")
    c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(cells), C), "set_cells")
    from tetraear.core.etsi import EtsiLowerMac
    lm = EtsiLowerMac()
    for k in range(K):
        want = host.demod(iq[:, k * L:(k + 1) * L])
        wf = lm.decode_stream(want[1], want[0], want[3], cells)
        s, W, yoff, y_next = stream_window(plan, x_total, y_done, L)
        sym, soft, hard, ns = bufs[k & 1]
        _, M2, sm = lengths(plan, W)
        smax = sm + 1
        ptr = dev.data_ptr() + 8 * s
        c.check(c.lib.tetra_demod_etsi_stream(c.handle, plan, ctypes.c_void_p(ptr), _hip.TETRA_CF32, C, K * L, W,
                                              int(yoff), _hip.ptr(track), ctypes.c_void_p(sym.data_ptr() + 8 * RESERVE),
                                              ctypes.c_void_p(soft.data_ptr() + 2 * RESERVE),
                                              ctypes.c_void_p(hard.data_ptr() + RESERVE), _hip.ptr(ns), smax, stride,
                                              None), "demod_stream")
        nsym = ns
        nb = torch.zeros(C, dtype=torch.int32, device="cuda")
        bursts = torch.zeros((C, 8, 2), dtype=torch.int32, device="cuda")
        nk = torch.zeros(C, dtype=torch.int32, device="cuda")
        blocks = torch.zeros((C, 16, 4), dtype=torch.int32, device="cuda")
        t1 = torch.zeros((C, 16, 268), dtype=torch.uint8, device="cuda")
        _, nsoft, nhard, _ = bufs[(k + 1) & 1]
        c.check(c.lib.tetra_lmac_etsi_stream(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, stride,
                                             _hip.ptr(lead), _hip.ptr(nsoft), _hip.ptr(nhard), None, _hip.ptr(nb),
                                             _hip.ptr(bursts), _hip.ptr(nk), _hip.ptr(blocks), _hip.ptr(t1)),
                "lmac_stream")
        c.synchronize()
        x_total += L
        y_done = y_next
        n = ns.cpu().numpy()
        h = hard.cpu().numpy()
        sy = sym.cpu().numpy().view(np.complex64)[..., 0]
        for ch in range(C):
            assert n[ch] == want[3][ch], (k, ch)
            assert np.array_equal(h[ch, RESERVE:RESERVE + n[ch] - 1], want[0][ch, :n[ch] - 1]), (k, ch)
            assert np.array_equal(sy[ch, RESERVE:RESERVE + n[ch]], want[2][ch, :n[ch]]), (k, ch)
        bt = bursts.cpu().numpy()
        nbh = nb.cpu().numpy()
        for ch in range(C):
            assert [tuple(bt[ch, b]) for b in range(nbh[ch])] == [(f["position"], f["burst_kind"]) for f in wf[ch]]


def test_process_and_decode_stream_across_seams():
    """The GUI's call pattern -- SignalProcessor(mode='etsi').process(chunk) then
    TetraDecoder(mode='etsi').decode(hard), chunk after chunk -- is the stream: the frames equal the
    oracle stream's bursts chunk by chunk, every slot after the first chunk decoded."""
    from tetraear.signal import SignalProcessor
    from tetraear.core import TetraDecoder
    from tetraear.signal.etsi import synth
    K = 6
    iq, cells = synth(1, K * L, seed=59, snr_db=18.0, cfo_max=300.0)[:2]
    p, d = SignalProcessor(2.4e6, mode="etsi"), TetraDecoder(mode="etsi")
    orc = E.Stream(2.4e6)
    nslots = 0
    for k in range(K):
        hard = p.process(iq[0, k * L:(k + 1) * L])
        assert len(p.symbols) == len(hard) + 1
        raw = d._etsi_rx().decode(hard)
        w = orc.push(iq[0, k * L:(k + 1) * L])
        assert np.array_equal(np.asarray(hard), w["hard"]) and np.array_equal(p.symbols, w["symbols"]), k
        assert [(f["position"], f["burst_kind"]) for f in raw] == [(q, kd) for q, kd, _ in w["bursts"]], k
        nslots += len(raw) if k else 0
    assert nslots >= int((K - 1) * L / 34000)


def test_process_odd_chunks_carry_the_last_sample():
    """process() chunks of odd length: the stream takes whole sample pairs, so each odd chunk's last
    sample goes in front of the next call's -- no sample is dropped and the stream stays the
    capture's: each call equals the oracle stream pushed with the pieces the carry produces."""
    from tetraear.signal.etsi import EtsiReceiver, synth
    iq = synth(1, 4 * L, seed=63, snr_db=18.0)[0][0]
    sizes = [65537, 65535, 131071, 131073, 3, 1, 50000]
    rx, orc = EtsiReceiver(), E.Stream(2.4e6)
    at, carry = 0, np.zeros(0, np.complex64)
    for k, n in enumerate(sizes):
        hard, sym = rx.process(iq[at:at + n])
        piece = np.concatenate([carry, iq[at:at + n]])
        carry = piece[len(piece) - len(piece) % 2:]
        piece = piece[:len(piece) - len(piece) % 2]
        at += n
        if len(piece) == 0:
            assert len(hard) == 0, k
            continue
        w = orc.push(piece)
        assert np.array_equal(np.asarray(hard), w["hard"]) and np.array_equal(sym, w["symbols"]), k
    assert orc.x_total == at - len(carry)


def test_stream_mixer_phase_is_continuous():
    """With an AFC offset the mixer runs on each window at the capture's global sample index, so the
    stream with the offset decodes as the stream of the pre-shifted capture does (every slot after
    the first chunk, CRC-good), and its first chunk equals the chunk mixed from its start."""
    from tetraear.signal.etsi import EtsiStream, EtsiReceiver, synth
    from tetraear.core.etsi import EtsiLowerMac
    C, K, f = 2, 5, 4 * 1171.875
    iq, cells = synth(C, K * L, seed=61, snr_db=20.0, cfo_max=100.0)[:2]
    n = np.arange(K * L)
    shifted = (iq * np.exp(2j * np.pi * f * n / 2.4e6)[None, :]).astype(np.complex64)   # +f, the mixer removes it
    st, lm = EtsiStream(2.4e6, C), EtsiLowerMac()
    good = total = 0
    for k in range(K):
        d = st.demod(shifted[:, k * L:(k + 1) * L], [f] * C)
        if k == 0:
            one = EtsiReceiver()
            h0, s0 = one.process(shifted[0, :L], f, stream=False)
            assert np.array_equal(d[0][0, :len(h0)], np.asarray(h0))
        fr = lm.decode_stream(d[1], d[0], d[3], cells)
        if k:
            for ch in range(C):
                total += len(fr[ch])
                good += sum(all(b["crc_ok"] for b in x["blocks"]) for x in fr[ch])
    assert total >= int(C * (K - 1) * L / 34000) and good >= 0.97 * total
