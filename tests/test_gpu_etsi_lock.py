"""GPU parity of the loss-of-lock monitor (tetra_etsi_lock, k_etsi_lock) and of the receiver around it
against tests/_etsi_lock_model.py: the records, state and track bit for bit on hand-made rows, and
EtsiStream(lock=True, redo=...) chunk by chunk against the model wrapped around oracle/etsi.py Stream;
then what the layers above do with a re-acquisition -- EtsiLowerMac.reset_channels, the drop-in
SignalProcessor / TetraDecoder pair with relock=True, and their reset().  Parity unpinned against the
reference (it has no ETSI chain and demodulates every chunk on its own).
"""
import functools

import numpy as np
import pytest

import _etsi_lock_model as M

pytestmark = pytest.mark.gpu

CHUNK, NCHUNK, FS = 32768, 6, 2.4e6
NSYMS = [0, 1, 2, 64, 65, 66, 2049]
OSTRIDE = 2051   # odd: rows 4102 bytes apart start at every even offset of a 16-byte line


# ------------------------------------------------------------------------------ 1. the kernel on hand-made rows

def _case(C, seed, patience):
    """Rows of every kind at every length, every byte past a row's 2 N set to 127; tracks and states."""
    rng = np.random.default_rng(seed)
    soft = np.full((C, 2 * OSTRIDE), 127, np.int8)
    nsym = np.array([NSYMS[(c + seed) % len(NSYMS)] for c in range(C)], np.int32)
    for c in range(C):
        n = max(int(nsym[c]) - 1, 0)
        kind = (c // len(NSYMS) + c) % 6
        if kind == 0:     # every byte value, -128 and +-127 among them
            v = rng.integers(-128, 128, 2 * n)
        elif kind == 1:   # silence
            v = np.zeros(2 * n, np.int64)
        elif kind == 2:   # every dibit weak at the default threshold
            v = rng.integers(-7, 8, 2 * n)
        elif kind == 3:   # a clean decision: |s0| = |s1|, at the rails
            m = rng.choice([127, -127, -128, 64], n)
            v = np.stack([m, np.where(rng.random(n) < 0.5, m, -np.clip(m, -127, 127))], 1).reshape(-1)
        elif kind == 4:   # noise-like: the balance near the threshold
            v = np.clip(np.rint(rng.standard_normal(2 * n) * 40), -127, 127)
        else:             # half weak, half strong
            v = np.where(np.repeat(rng.random(n) < 0.5, 2), rng.integers(-7, 8, 2 * n), rng.integers(-128, 128, 2 * n))
        soft[c, :2 * n] = v
    track = np.zeros(C, M.E.TRACK)
    track["base"], track["pr"], track["pi"] = rng.random(C), rng.standard_normal(C), rng.standard_normal(C)
    track["delta"] = rng.choice(np.array([0.0, 0.3, -1.2, 1.5, -1.5, 1.4999999, np.nan], np.float32), C)
    track["acquired"] = 1
    track["reserved"] = rng.integers(0, 1 << 30, (C, 3))
    state = np.zeros(C, M.LOCK_STATE)
    pick = rng.integers(0, 4, C)   # a new stream, a searching one, a locked one, one a bad chunk short of a drop
    state["searching"] = pick == 1
    state["chunks"] = np.where(pick == 0, 0, rng.integers(1, 100, C))
    state["bad_run"] = np.where(pick == 3, max(patience - 1, 0), 0)
    state["relocks"] = np.where(pick == 0, 0, rng.integers(0, 5, C))
    state["reserved"] = np.where((pick == 0)[:, None], 0, rng.integers(0, 1 << 30, (C, 4)))
    return soft, nsym, track, state


def _lock(args, soft, nsym, ostride, track, state, rec):
    from tetraear import _hip
    c = _hip.ctx()
    C = 5 if nsym is None else len(nsym)
    return c.lib.tetra_etsi_lock(c.handle, _hip.ptr(soft), _hip.ptr(nsym), C, ostride, *args, _hip.ptr(track),
                                 _hip.ptr(state), _hip.ptr(rec))


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("args", [(M.NUM, M.DEN, M.WEAK, M.NMIN, M.PATIENCE), (3, 5, 20, 2, 3), (1, 2, 0, 64, 1),
                                  (0, 1, 200, 1, 2)])
@pytest.mark.parametrize("C", [1, 5, 65])
def test_records_state_and_track_equal_the_model(C, args):
    import torch
    from tetraear import _hip
    num, den, weak, nmin, patience = args
    soft, nsym, track, state = _case(C, 3 + C, patience)
    t_want, s_want = track.copy(), state.copy()
    want = M.lock(soft, nsym, OSTRIDE, t_want, s_want, num, den, weak, nmin, patience)
    assert want[:, M.R_FLAGS].max() > 0 or C == 1
    # host pointers
    t_got, s_got, rec = track.copy(), state.copy(), np.full((C, 8), -7, np.int32)
    assert _lock(args, soft, nsym, OSTRIDE, t_got, s_got, rec) == 0
    assert np.array_equal(rec, want)
    assert np.array_equal(_bytes(s_got), _bytes(s_want)) and np.array_equal(_bytes(t_got), _bytes(t_want))
    # device pointers, the rows at an aligned, an even and an odd address
    for off in (0, 6, 1):
        buf = torch.zeros(soft.size + 16, dtype=torch.int8, device="cuda")
        buf[off:off + soft.size] = torch.from_numpy(soft.reshape(-1)).cuda()
        d_ns = torch.from_numpy(nsym).cuda()
        d_t = torch.from_numpy(_bytes(track).copy()).cuda()
        d_s = torch.from_numpy(_bytes(state).copy()).cuda()
        d_rec = torch.full((C, 8), -7, dtype=torch.int32, device="cuda")
        import ctypes
        c = _hip.ctx()
        c.check(c.lib.tetra_etsi_lock(c.handle, ctypes.c_void_p(buf.data_ptr() + off), _hip.ptr(d_ns), C, OSTRIDE, *args,
                                      _hip.ptr(d_t), _hip.ptr(d_s), _hip.ptr(d_rec)), "tetra_etsi_lock")
        c.synchronize()
        assert np.array_equal(d_rec.cpu().numpy(), want), off
        assert np.array_equal(d_s.cpu().numpy(), _bytes(s_want)) and np.array_equal(d_t.cpu().numpy(), _bytes(t_want)), off


def test_invalid_arguments_write_nothing():
    from tetraear import _hip
    ok = (M.NUM, M.DEN, M.WEAK, M.NMIN, M.PATIENCE)
    soft, nsym, track, state = _case(5, 9, 1)
    keep = [a.copy() for a in (track, state)]
    rec = np.full((5, 8), -7, np.int32)
    bad = [(ok, None, nsym, OSTRIDE, track, state, rec), (ok, soft, None, OSTRIDE, track, state, rec),
           (ok, soft, nsym, OSTRIDE, None, state, rec), (ok, soft, nsym, OSTRIDE, track, None, rec),
           (ok, soft, nsym, OSTRIDE, track, state, None), (ok, soft, nsym, 0, track, state, rec),
           (ok, soft, nsym, (1 << 23) + 1, track, state, rec), (ok, soft, nsym[:0], OSTRIDE, track, state, rec),
           ((1, 0, 8, 64, 1), soft, nsym, OSTRIDE, track, state, rec),
           ((1, -2, 8, 64, 1), soft, nsym, OSTRIDE, track, state, rec),
           ((-1, 2, 8, 64, 1), soft, nsym, OSTRIDE, track, state, rec),
           ((1, 2, 8, 64, 0), soft, nsym, OSTRIDE, track, state, rec)]
    for i, a in enumerate(bad):
        assert _lock(*a) == -1, i   # TETRA_E_INVALID
        assert np.array_equal(_bytes(track), _bytes(keep[0])) and np.array_equal(_bytes(state), _bytes(keep[1])), i
        assert (rec == -7).all(), i
    assert _lock(ok, soft, nsym, OSTRIDE, track, state, rec) == 0 and (rec[:, 7] == 0).all()


# ------------------------------------------------------------------------------ 2. the stream

@functools.lru_cache(maxsize=None)
def _capture(fmt):
    """(the samples EtsiStream is fed, the complex64 samples the model is fed)"""
    iq = M.three_channels(11, CHUNK, NCHUNK, FS)
    if fmt == "cf32":
        return iq, iq
    q = np.clip(np.round(iq.view(np.float32).reshape(3, -1, 2) * (32768 * 0.25)), -32768, 32767).astype(np.int16)
    x = ((q[..., 0].astype(np.float32) + 1j * q[..., 1].astype(np.float32)) / np.float32(32768)).astype(np.complex64)
    return q, x


@functools.lru_cache(maxsize=None)
def _model(fmt, redo, patience):
    want = M.run_model(_capture(fmt)[1], CHUNK, FS, lock=True, redo=redo, consts=dict(patience=patience))
    # the CPU check first: with these exact arrays the model drops channel 1 (the slip before chunk 3) and
    # channel 2 (the noise chunk 2) where expected, and never channel 0
    drops = [[k for k, w in enumerate(want) if w[c]["dropped"]] for c in range(3)]
    assert drops == [[], [2 + patience], [1 + patience]], drops
    return want


@functools.lru_cache(maxsize=None)
def _gpu(fmt, lock, redo, patience):
    """EtsiStream over the capture: per chunk dict(out, fresh, dropped, rec, track, state, before)."""
    from tetraear.signal.etsi import EtsiStream
    x = _capture(fmt)[0]
    st = EtsiStream(FS, 3, lock=lock, redo=redo, lock_patience=patience) if lock else EtsiStream(FS, 3)
    got = []
    for k in range(NCHUNK):
        before = (None if st.hist is None else st.hist.copy(), st.x_total, st.y_done)
        out = st.demod(x[:, k * CHUNK:(k + 1) * CHUNK])
        got.append(dict(out=tuple(a.copy() for a in out), fresh=st.fresh.copy(), dropped=st.dropped.copy(),
                        rec=st.lock_records.copy(), track=st.track.copy(), state=st.lock_state.copy(), before=before))
    return got


def _rows_equal(a, b, ca, cb, what):
    (ha, sa, ya, na), (hb, sb, yb, nb) = a, b
    n = int(na[ca])
    assert n == int(nb[cb]), what
    assert np.array_equal(ya[ca, :n], yb[cb, :n]) and np.array_equal(ha[ca, :max(n - 1, 0)], hb[cb, :max(n - 1, 0)]), what
    assert np.array_equal(sa[ca, :2 * max(n - 1, 0)], sb[cb, :2 * max(n - 1, 0)]), what


@pytest.mark.parametrize("fmt,redo,patience", [("cf32", True, 1), ("cf32", False, 1), ("cf32", True, 2), ("sc16", True, 1)])
def test_stream_equals_the_model(fmt, redo, patience):
    want, got = _model(fmt, redo, patience), _gpu(fmt, True, redo, patience)
    plain = _gpu(fmt, False, False, 0)
    for k in range(NCHUNK):
        hard, soft, sym, ns = got[k]["out"]
        for c in range(3):
            w, case = want[k][c], (fmt, redo, patience, k, c)
            n = int(ns[c])
            assert n == len(w["symbols"]), case
            assert np.array_equal(sym[c, :n], w["symbols"]) and np.array_equal(hard[c, :n - 1], w["hard"]), case
            assert np.array_equal(soft[c, :2 * (n - 1)], w["soft"]), case
            assert bool(got[k]["fresh"][c]) == w["fresh"] and bool(got[k]["dropped"][c]) == w["dropped"], case
            assert np.array_equal(got[k]["rec"][c], w["rec"]), case
            assert np.array_equal(_bytes(got[k]["state"][c:c + 1]), _bytes(w["state"])), case
            # the fields the monitor reads and writes (the loop's offset is the oracle's bit for bit)
            assert got[k]["track"]["acquired"][c] == w["track"]["acquired"][0], case
            assert got[k]["track"]["delta"][c:c + 1].tobytes() == w["track"]["delta"].tobytes(), case
        # the continuous channel: bit for bit the receiver without the monitor, in every chunk
        _rows_equal(got[k]["out"], plain[k]["out"], 0, 0, ("plain", k))


@pytest.mark.parametrize("redo", [True, False])
def test_a_reacquired_row_is_a_fresh_stream_on_the_same_window(redo):
    """From the chunk that starts a new chain on (the redone one; without redo the one after the drop), a
    channel's rows are those of a new EtsiStream handed the same window history and started there -- until
    the channel starts another chain."""
    from tetraear.signal.etsi import EtsiStream
    got = _gpu("cf32", True, redo, 1)
    x = _capture("cf32")[0]
    starts = [(k, c) for c in (1, 2) for k in range(1, NCHUNK) if got[k]["fresh"][c]]
    assert starts == ([(3, 1), (2, 2), (3, 2)] if redo else [(4, 1), (3, 2)])
    for k0, c in starts:
        hist, x_total, y_done = got[k0]["before"]
        new = EtsiStream(FS, 1)
        new.hist, new.x_total, new.y_done = hist[c:c + 1].copy(), x_total, y_done
        for k in range(k0, NCHUNK):
            if k > k0 and got[k]["fresh"][c]:
                break
            out = new.demod(x[c:c + 1, k * CHUNK:(k + 1) * CHUNK])
            _rows_equal(got[k]["out"], out, c, 0, (redo, k0, c, k))


# ------------------------------------------------------------------------------ 3. the lower MAC's reset_channels

def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def test_reset_channels_is_a_new_lower_mac_with_the_cell():
    from tetraear.core.etsi import EtsiLowerMac
    got = _gpu("cf32", True, True, 1)
    opts = dict(mac=True, sdu=True, timebase_vote=False)
    masked, unmasked = EtsiLowerMac(**opts), EtsiLowerMac(**opts)
    news = []   # (first chunk, channel, the new lower MAC, its frames per chunk)
    frames_m, frames_u = [], []
    for k in range(NCHUNK):
        hard, soft, sym, ns = got[k]["out"]
        fresh = got[k]["fresh"]
        for c in np.nonzero(fresh)[0] if k else []:
            new = EtsiLowerMac(**opts)
            new.cell_state, new.acquired = masked.cell_state.copy(), masked.acquired.copy()
            news.append((k, int(c), new, []))
        for k0, c, new, fr in news:   # the same rows from that call on (and the same masks after it)
            fr.append(new.decode_stream(soft, hard, ns, fresh=fresh if k > k0 else None))
        frames_m.append(masked.decode_stream(soft, hard, ns, fresh=fresh))
        frames_u.append(unmasked.decode_stream(soft, hard, ns))
    assert [(k, c) for k, c, _, _ in news] == [(2, 2), (3, 1), (3, 2)]
    for k0, c, _, fr in news:
        for k in range(k0, NCHUNK):
            assert _same(frames_m[k][c], fr[k - k0][c]), (k0, c, k)
    assert sum(len(f[c]) for f in frames_m for c in range(3)) >= 8   # the stream does hold bursts
    for k in range(NCHUNK):   # the channel no mask names: as without masks
        assert _same(frames_m[k][0], frames_u[k][0]), k
    # what a reset clears and what it keeps
    from tetraear import _hip
    cells, lead0 = masked.cell_state.copy(), masked._rows[2].copy()
    masked.reset_channels([False, True, False])
    srow, hrow, lead = masked._rows
    assert lead[1] == 2 * _hip.ETSI_RESERVE and lead[0] == lead0[0] and lead[2] == lead0[2]
    assert not srow[1, :2 * _hip.ETSI_RESERVE].any() and not hrow[1, :_hip.ETSI_RESERVE].any()
    assert not _bytes(masked._tdma[1:2]).any() and not _bytes(masked._frag[1:2]).any()
    assert np.array_equal(masked.cell_state, cells) and masked.acquired.any()


# ------------------------------------------------------------------------------ 4, 5. the drop-in pair

def _view(frames):
    return [(f["position"], f["burst_kind"], f["burst_crc"],
             [(b["channel"], b["crc_ok"], np.asarray(b["bits"]).tobytes()) for b in f["blocks"]]) for f in frames]


def _pair(relock):
    from tetraear.signal import SignalProcessor
    from tetraear.core import TetraDecoder
    return SignalProcessor(FS, mode="etsi", relock=relock), TetraDecoder(auto_decrypt=False, mode="etsi")


def test_drop_in_pair_flags_the_reacquired_chunk():
    from tetraear.signal.etsi import EtsiReceiver, stream_window
    x = _capture("cf32")[0][2]   # channel 2: signal, noise, another cell's signal
    want = _model("cf32", True, M.PATIENCE)
    expect = [k > 0 and want[k][2]["fresh"] for k in range(NCHUNK)]
    assert expect == [False, False, True, True, False, False]
    p, d = _pair(True)
    flags, frames, starts = [], [], []
    for k in range(NCHUNK):
        s = p._etsi._stream if p._etsi is not None else None
        starts.append((0, 0) if s is None else (s.x_total, s.y_done))
        hard = p.process(x[k * CHUNK:(k + 1) * CHUNK])
        assert np.array_equal(hard, want[k][2]["hard"]) and np.array_equal(hard.soft_bits, want[k][2]["soft"]), k
        assert np.array_equal(p.symbols, want[k][2]["symbols"]), k
        flags.append(hard.new_stream)
        if k == 3:
            cell = (d._etsi.cell_state.copy(), d._etsi.acquired.copy())
        frames.append(_view(d.decode(hard)))
    assert flags == expect
    # from the last re-acquired chunk on: a fresh pair that is handed the cell and fed the same window
    k0 = 3
    s0 = stream_window(p._etsi.plan, starts[k0][0], starts[k0][1], CHUNK)[0]
    p2, d2 = _pair(True)
    d2._etsi_rx().cell_state, d2._etsi.acquired = cell
    for k in range(k0, NCHUNK):
        hard = p2.process(x[s0 if k == k0 else k * CHUNK:(k + 1) * CHUNK])
        assert not hard.new_stream and np.array_equal(hard, want[k][2]["hard"]), k
        assert _view(d2.decode(hard)) == frames[k], k
    # relock=False: new_stream never set, and the outputs are today's (EtsiReceiver.process, EtsiLowerMac.decode)
    p, d = _pair(False)
    rx, d0 = EtsiReceiver(FS), _pair(False)[1]
    plain = _gpu("cf32", False, False, 0)
    for k in range(NCHUNK):
        hard = p.process(x[k * CHUNK:(k + 1) * CHUNK])
        h0, y0 = rx.process(x[k * CHUNK:(k + 1) * CHUNK])
        assert not hard.new_stream and not h0.new_stream
        assert np.array_equal(hard, h0) and np.array_equal(hard.soft_bits, h0.soft_bits) and np.array_equal(p.symbols, y0)
        assert np.array_equal(hard, plain[k]["out"][0][2, :len(hard)]) and len(hard) == plain[k]["out"][3][2] - 1, k
        assert _view(d.decode(hard)) == _view(d0.decode(h0)), k


def test_reset_makes_the_next_chunk_a_new_objects_chunk():
    x = _capture("cf32")[0][0]
    p, d = _pair(True)
    for k in range(2):
        d.decode(p.process(x[k * CHUNK:(k + 1) * CHUNK]))
    p.reset()
    d.reset()
    cell = (d._etsi.cell_state.copy(), d._etsi.acquired.copy())
    p2, d2 = _pair(True)
    d2._etsi_rx().cell_state, d2._etsi.acquired = cell   # TetraDecoder.reset keeps the acquired cell
    for k in range(2, 4):
        a, b = p.process(x[k * CHUNK:(k + 1) * CHUNK]), p2.process(x[k * CHUNK:(k + 1) * CHUNK])
        assert np.array_equal(a, b) and np.array_equal(a.soft_bits, b.soft_bits) and np.array_equal(p.symbols, p2.symbols)
        assert not a.new_stream and len(a) > 200
        assert _view(d.decode(a)) == _view(d2.decode(b)), k
    # compat mode: reset() exists and does nothing
    from tetraear.signal import SignalProcessor
    from tetraear.core import TetraDecoder
    SignalProcessor(FS, mode="compat").reset()
    TetraDecoder(auto_decrypt=False, mode="compat").reset()
