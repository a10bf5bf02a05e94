"""The timebase vote through the Python surface (WidebandReceiver.decode(timebase="vote"),
WidebandStream(timebase="vote"), EtsiLowerMac(mac=True, timebase_vote=True), TetraDecoder) on the grid capture
tests/test_gpu_wideband_timebase.py synthesises (all 800 carriers, three chunks each) and on the streamed
channels of tests/test_gpu_etsi_mac.py.  On a clean single-cell capture the vote places what
tetra_etsi_mac_groups places and never keeps a worse copy; tests/test_gpu_etsi_tdma_vote.py holds the
entry point to its rule."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NW_GPU = 3_300_000   # tests/test_gpu_wideband_timebase.py's capture
PIECES = ((0, 1_211_111), (1_211_111, 1_400_001), (1_400_001, NW_GPU))
SLOT_KEYS = ("tn", "fn", "mn")


@pytest.fixture(scope="module")
def capture_grid():
    from tetraear.signal.wideband import synth_wideband
    return synth_wideband(NW_GPU, seed=17, snr_db=25.0, cfo_max=300.0, grid=True)


@pytest.fixture(scope="module")
def decoded(capture_grid):
    """(frames of timebase=True, frames of timebase="vote", the vote's ballots [M, 4])."""
    from tetraear.signal.wideband import WidebandReceiver
    x, cells = capture_grid[:2]
    rx = WidebandReceiver()
    plain = rx.decode(x, cells, timebase=True)
    assert rx.tvote is None
    vote = rx.decode(x, cells, timebase="vote")
    return plain, vote, rx.tvote.copy()


def _good(f):
    return sum(b["crc_ok"] for b in f["blocks"])


def test_vote_places_what_the_timebase_places(decoded):
    """Every frame carries the tn / fn / mn that timebase=True gives the burst at that position, no kept
    frame has fewer CRC-good blocks than the one timebase=True keeps there, and the keys are the same."""
    plain, vote, tvote = decoded
    frames = better = moved = 0
    differ, worse = [], []
    for k, (fa, fb) in enumerate(zip(plain, vote)):
        assert len(fa) == len(fb), k
        for f, g in zip(fa, fb):
            assert abs(f["sample"] - g["sample"]) <= 64 and f["burst_kind"] == g["burst_kind"], (k, f["sample"], g["sample"])
            if [f[key] for key in SLOT_KEYS] != [g[key] for key in SLOT_KEYS]:
                differ.append((k, f["sample"], [f[key] for key in SLOT_KEYS], [g[key] for key in SLOT_KEYS], f["chunk"], g["chunk"]))
            if _good(g) < _good(f):
                worse.append((k, f["sample"]))
            assert set(f) == set(g) and all(set(a) == set(b) for a, b in zip(f["blocks"], g["blocks"]))
            assert g["slot_flags"] in (0, 1)   # one cell, one grid: nothing contradicts, nothing is outvoted
            better += _good(g) > _good(f)
            moved += f["chunk"] != g["chunk"]
            frames += 1
    print("vote against timebase=True: %d frames, %d from the other chunk, %d of them with more CRC-good blocks; "
          "ballots %s" % (frames, moved, better, tvote.sum(axis=0).tolist()))
    print("slots that differ: %d %s; worse copies kept: %d" % (len(differ), differ[:5], len(worse)))
    assert not differ and not worse
    assert frames > 8000   # (about 10 frames a carrier: the capture holds 11 slots)
    assert tvote[:, 0].sum() > 2000 and np.array_equal(tvote[:, 1] + (tvote[:, 0] > 0), tvote[:, 0])   # one locks, the rest agree
    assert not tvote[:, 2:].any()


def test_vote_frames_gain_quality_keys_only_when_asked(capture_grid):
    """One chunk: the link-quality keys reach the frames only with link_quality=True, decode_acquire takes
    the mode too, and the arguments are checked."""
    from tetraear.signal.wideband import WidebandReceiver
    x, cells = capture_grid[:2]
    n = 400_000   # one chunk
    rx = WidebandReceiver()
    a = rx.decode(x[:n], cells, timebase="vote")
    b = rx.decode(x[:n], cells, timebase="vote", link_quality=True)
    fa, fb = [f for fr in a for f in fr], [f for fr in b for f in fr]
    assert len(fa) == len(fb) > 200
    assert all("soft_sum" not in f and "channel_errors" not in f["blocks"][0] for f in fa)
    assert all("soft_sum" in f and "channel_errors" in f["blocks"][0] for f in fb)
    assert [(f["sample"], f["tn"], f["fn"], f["mn"], f["slot_flags"]) for f in fa] == \
           [(f["sample"], f["tn"], f["fn"], f["mn"], f["slot_flags"]) for f in fb]
    got, state, ngood = rx.decode_acquire(x[:n], np.full(len(cells), 3, np.uint32), timebase="vote")
    assert sum(len(fr) for fr in got) == len(fa) and rx.tvote[:, 0].sum() > 0
    for bad in (dict(timebase="votes"), dict(timebase="vote", tdma_cap=0), dict(timebase="vote", tol=63)):
        with pytest.raises(ValueError):
            rx.decode(x[:n], cells, **bad)


def test_stream_carries_the_scores(capture_grid):
    """Three uneven pieces: the stream with timebase="vote" reports the frames of the stream with
    timebase=True, slot for slot, and ends with scores; reset() clears them."""
    from tetraear import _hip
    from tetraear.signal.wideband import WidebandStream
    x, cells = capture_grid[:2]
    out = []
    for mode in (True, "vote"):
        st = WidebandStream(cells, timebase=mode)
        frames = [[] for _ in cells]
        for a, b in PIECES:
            for k, fr in enumerate(st.decode(x[a:b])):
                frames[k] += fr
        out.append(frames)
        if mode is True:
            assert st.tdma_scores is None and st.tdma_score is None
            tdma = st.tdma.copy()
    scores = st.tdma_scores
    assert scores.shape == (len(cells),) and scores.dtype == np.int32
    assert (scores > 0).sum() > 700 and scores.max() <= _hip.TETRA_TDMA_VOTE_CAP_DEFAULT
    # (the anchors may sit a bit or two apart: an SB in an overlap anchors at its heavier copy)
    assert np.array_equal((scores > 0), st.tdma["locked"] != 0) and np.array_equal(st.tdma["locked"], tdma["locked"])
    assert np.array_equal(st.tdma["bit0"], tdma["bit0"]) and np.abs(st.tdma["anchor_bit"] - tdma["anchor_bit"]).max() <= 32
    n, differ = 0, []
    for k, (fa, fb) in enumerate(zip(*out)):
        assert len(fa) == len(fb), k
        for f, g in zip(fa, fb):
            assert abs(f["stream_sample"] - g["stream_sample"]) <= 64, (k, f["stream_sample"])
            if [f[key] for key in SLOT_KEYS] != [g[key] for key in SLOT_KEYS]:
                differ.append((k, f["stream_sample"], [f[key] for key in SLOT_KEYS], [g[key] for key in SLOT_KEYS]))
            assert _good(g) >= _good(f)
            n += 1
    print("stream: %d frames, slots that differ: %d %s" % (n, len(differ), differ[:5]))
    assert not differ and n > 8000
    st.reset()
    assert not st.tdma_score.any() and not st.tdma.view(np.uint8).any()
    with pytest.raises(ValueError):
        WidebandStream(cells, timebase="vote", tdma_cap=0)
    with pytest.raises(ValueError):
        WidebandStream(cells, timebase="yes")


def test_lower_mac_stream_with_the_vote():
    """EtsiLowerMac(mac=True, timebase_vote=True) over the streamed chunks of tests/test_gpu_etsi_mac.py (chunk
    lengths differ from channel to channel): tn / fn / mn, slot_flags and the PDUs are mac=True's, the
    scores are kept beside the timebases and reset_stream() clears them."""
    import test_gpu_etsi_mac as T
    from tetraear.core.etsi import EtsiLowerMac
    from tetraear.core import TetraDecoder
    plain = T._decode_stream(EtsiLowerMac(mac=True))
    lm = EtsiLowerMac(mac=True, timebase_vote=True)
    vote = T._decode_stream(lm)
    assert sum(len(fr) for fr in plain) == sum(len(fr) for fr in vote) == 60
    for ch, (fa, fb) in enumerate(zip(plain, vote)):
        for f, g in zip(fa, fb):
            assert set(f) == set(g)
            assert [f[k] for k in SLOT_KEYS + ("slot_flags", "position")] == [g[k] for k in SLOT_KEYS + ("slot_flags", "position")], ch
            assert [(b["npdu"], b["pdus"]) for b in f["blocks"]] == [(b["npdu"], b["pdus"]) for b in g["blocks"]]
    assert any(g["tn"] is not None for fr in vote for g in fr)
    assert lm.tdma_score.shape == (len(vote),) and (lm.tdma_score > 0).any() and lm.tdma_votes.shape == (len(vote), 4)
    assert np.array_equal(lm.tdma_score > 0, lm._tdma["locked"] != 0)
    lm.reset_stream()
    assert lm.tdma_score is None and lm._tdma is None
    with pytest.raises(ValueError):
        EtsiLowerMac(timebase_vote=True)
    with pytest.raises(ValueError):
        EtsiLowerMac(mac=True, timebase_vote=True, tdma_cap=0)
    d = TetraDecoder(auto_decrypt=False, mode="etsi", mac=True, timebase_vote=True)
    assert d.etsi_timebase_vote and not TetraDecoder(auto_decrypt=False, mode="etsi", mac=True).etsi_timebase_vote
