"""tests/_etsi_traffic_model.py and the traffic read-out's Python surface on the CPU: the built traffic
bursts mean to the oracle's lower MAC what tests/test_gpu_etsi_traffic.py assumes, the model does what
the rule says on hand-made rows, codec_frame equals the reference's recorded frames word for word."""
import os

import numpy as np
import pytest

import etsi as E
import _etsi_traffic_model as T
import _lmac_rows as R

N, P, SB = R.NDB_N, R.NDB_P, R.SB
HERE = os.path.dirname(os.path.abspath(__file__))


def _row(rng, cell, items, lead=6, tail=8):
    """Bursts (kind, t4 or None: an ordinary coded burst) with gaps: (bits, starts)."""
    scr = E.scramble_seq(cell, 432)
    parts, starts, at = [rng.integers(0, 2, lead).astype(np.uint8)], [], lead
    for kind, t4 in items:
        b = E.make_burst(kind, rng, scr)[0] if t4 is None else T.traffic_burst(kind, t4, scr, rng)[0]
        g = int(rng.integers(0, 5))
        parts += [b, rng.integers(0, 2, g).astype(np.uint8)]
        starts.append(at)
        at += 510 + g
    parts.append(rng.integers(0, 2, tail + ((at + tail) & 1)).astype(np.uint8))
    return np.concatenate(parts), starts


# ------------------------------------------------------------------------------ the built bursts

@pytest.mark.parametrize("seed", range(6))
def test_traffic_bursts_on_the_oracle_lower_mac(seed):
    """Conditions the inputs were chosen for (fixed seeds), not results: the full slot is found as kind 0
    and fails its SCH/F CRC, the stolen + half slot as kind 1 and decodes (good, bad); descrambling the
    soft bits returns t4."""
    rng = np.random.default_rng(3100 + seed)
    cell = R.random_cell(rng)
    scr = E.scramble_seq(cell, 432)
    t4f, t4h = rng.integers(0, 2, 432).astype(np.uint8), rng.integers(0, 2, 216).astype(np.uint8)
    bits, starts = _row(rng, cell, [(N, t4f), (SB, None), (P, t4h), (N, None)])
    hard, soft = R.hard_of(bits), R.soft_of(bits, 127)
    got = E.Receiver().lower_mac(soft, hard, cell)
    assert [(s, k) for s, k, _ in got] == list(zip(starts, (N, SB, P, N)))
    assert [(k, bool(ok)) for k, _, ok in got[0][2]] == [(0, False)]
    assert [(k, bool(ok)) for k, _, ok in got[2][2]] == [(1, True), (1, False)]
    assert [bool(ok) for _, _, ok in got[1][2]] == [True, True] and [bool(ok) for _, _, ok in got[3][2]] == [True]
    bursts, blocks, _ = R.flatten(got)
    o = dict(nburst=np.array([4], np.int32), bursts=np.zeros((1, 8, 2), np.int32), nblock=np.array([len(blocks)], np.int32),
             blocks=np.zeros((1, 16, 4), np.int32))
    o["bursts"][0, :4], o["blocks"][0, :len(blocks)] = bursts, blocks
    tq, tch = T.traffic(soft[None, :], 0, 1, [cell], o["nburst"], o["bursts"], o["nblock"], o["blocks"])
    assert tq[0, :4].tolist() == [[T.FULL, 432, 432 * 127, 0], [T.NONE, 0, 0, 0], [T.HALF, 216, 216 * 127, 0],
                                  [T.CONTROL, 0, 0, 0]]
    assert np.array_equal(T.signs(tch[0, 0]), t4f) and np.array_equal(T.signs(tch[0, 2, :216]), t4h)
    assert (tch[0, 2, 216:] == T.POISON8).all() and (tch[0, 1] == T.POISON8).all() and (tq[0, 4:] == T.POISON).all()
    # the same slots by hand: field bits ^ sequence
    assert np.array_equal(np.concatenate([bits[starts[0] + 14:starts[0] + 230], bits[starts[0] + 282:starts[0] + 498]]) ^ scr,
                          t4f)


# ------------------------------------------------------------------------------ the model on hand-made rows

def _one(kind, blocks, soft=None, start=4, slots=None, keep=None, cell=0x1234567, nburst=1, stride=300):
    soft = np.full((1, 2 * stride), 50, np.int8) if soft is None else soft
    bu = np.zeros((1, 8, 2), np.int32)
    bu[0, 0] = [start, kind]
    bk = np.zeros((1, 16, 4), np.int32)
    if blocks:
        bk[0, :len(blocks)] = blocks
    return T.traffic(soft, 0, 1, [cell], np.array([nburst], np.int32), bu, np.array([len(blocks)], np.int32), bk,
                     slots, keep)


def test_every_class_is_reached():
    fn18, kept0 = np.zeros((1, 8, 4), np.int32), np.ones((1, 8), np.int32)
    fn18[0, 0, T.SLOT_FN] = 18
    kept0[0, 0] = 0
    want = [
        ((0, [(0, 0, 0, 0)]), {}, T.FULL),
        ((0, [(0, 1, 0, 0)]), {}, T.CONTROL),
        ((0, [(0, 1, 1, 0), (1, 1, 0, 0), (0, 1, 0, 1)]), {}, T.FULL),   # another burst, another kind, no such index
        ((1, [(1, 1, 0, 0), (1, 1, 0, 1)]), {}, T.CONTROL),
        ((1, [(1, 1, 0, 0), (1, 0, 0, 1)]), {}, T.HALF),
        ((1, [(1, 0, 0, 0), (1, 1, 0, 1)]), {}, T.LOST),
        ((1, []), {}, T.LOST),
        ((2, [(2, 1, 0, 0), (1, 1, 0, 1)]), {}, T.NONE),
        ((0, [(0, 0, 0, 0)]), dict(slots=fn18), T.CONTROL),
        ((2, []), dict(slots=fn18), T.NONE),                      # rule c before rule d
        ((0, [(0, 0, 0, 0)]), dict(slots=fn18, keep=kept0), T.NONE),   # rule b before rule d
        ((1, [(1, 1, 0, 0)]), dict(slots=np.zeros((1, 8, 4), np.int32), keep=np.ones((1, 8), np.int32)), T.HALF),
    ]
    seen = set()
    for (kind, blocks), kw, cls in want:
        tq, tch = _one(kind, blocks, **kw)
        assert tq[0, 0, T.CLASS] == cls, (kind, blocks, kw)
        n = {T.FULL: 432, T.HALF: 216}.get(cls, 0)
        assert tq[0, 0, T.NBITS] == n and (tch[0, 0, n:] == T.POISON8).all() and (tq[0, 1:] == T.POISON).all()
        seen.add(cls)
    assert seen == {T.NONE, T.CONTROL, T.FULL, T.HALF, T.LOST}
    # invalid bursts: a kind outside 0..2, a start before the row, an end one bit past it; the last start inside
    for kind, start, ok in ((3, 4, False), (-1, 4, False), (0, -1, False), (0, 91, False), (0, 90, True)):
        tq, tch = _one(kind, [], start=start)
        assert (tq[0, 0].tolist() == [-1] * 4) == (not ok) and ok == (tch[0, 0, 0] != T.POISON8), (kind, start)
    # the counts clamp: nothing past MAXB, and a negative count writes nothing
    tq, _ = _one(0, [], nburst=99)
    assert (tq[0] != T.POISON).all()
    tq, _ = _one(0, [], nburst=-2)
    assert (tq == T.POISON).all()


def test_soft_classes_descramble_as_the_rule_says():
    rng = np.random.default_rng(77)
    cell = R.random_cell(rng)
    scr = E.scramble_seq(cell, 432)
    assert 100 < scr.sum() < 332
    off = T.field_offsets(T.FULL)
    assert off[0] == 14 and off[215] == 229 and off[216] == 282 and off[431] == 497
    for name in ("m128", "zero", "tern", "uniform"):
        soft = rng.integers(-128, 128, (1, 600)).astype(np.int8)
        field = R.soft_class(name, rng.integers(0, 2, 432), rng)
        if name == "m128":
            field[np.flatnonzero(scr == 0)[:4]] = -128   # under q = 0 and q = 1 both
            field[np.flatnonzero(scr == 1)[:4]] = -128
        soft[0, 4 + off] = field
        tq, tch = _one(0, [], soft=soft, cell=cell)
        f = field.astype(np.int64)
        want = np.where(scr == 1, np.where(f == -128, 127, -f), f)
        assert np.array_equal(tch[0, 0].astype(np.int64), want)
        assert tq[0, 0].tolist() == [T.FULL, 432, int(np.abs(want).sum()), int((want == 0).sum())]
    # -128 stays -128 where q = 0 and counts 128; it becomes 127 where q = 1
    soft = np.full((1, 600), -128, np.int8)
    tq, tch = _one(0, [], soft=soft, cell=cell)
    assert np.array_equal(tch[0, 0], np.where(scr == 1, 127, -128).astype(np.int8))
    assert tq[0, 0, T.WSUM] == int(128 * (scr == 0).sum() + 127 * (scr == 1).sum())
    # a half slot reads the second field with the sequence from its start
    soft = rng.integers(-127, 128, (1, 600)).astype(np.int8)
    tq, tch = _one(1, [(1, 1, 0, 0)], soft=soft, cell=cell)
    s = soft[0, 4 + 282:4 + 498].astype(np.int64)
    assert np.array_equal(tch[0, 0, :216].astype(np.int64), np.where(scr[:216] == 1, -s, s))


def test_groups_take_their_groups_cell():
    rng = np.random.default_rng(5)
    cells = [R.random_cell(rng), R.random_cell(rng)]
    soft = rng.integers(-127, 128, (4, 600)).astype(np.int8)
    soft[soft == 0] = 1   # a zero has no sign to flip
    bu = np.zeros((4, 8, 2), np.int32)
    tq, tch = T.traffic(soft, 0, 2, cells, np.ones(4, np.int32), bu, np.zeros(4, np.int32), np.zeros((4, 16, 4), np.int32))
    for c in range(4):
        scr = E.scramble_seq(cells[c // 2], 432)
        assert np.array_equal(T.signs(tch[c, 0]), (soft[c, T.field_offsets(T.FULL)] < 0) ^ scr)


# ------------------------------------------------------------------------------ codec_frame

def _fixture():
    return np.load(os.path.join(HERE, "golden", "g6_voice.npz"))


def _soft_of_symbols(sym, pos):
    """The fixture's symbols as the chain's soft values: bits MSB first, symbols pos // 3 + (0..107,
    119..226), soft = bit ? -127 : +127."""
    s = np.asarray(sym, np.int64)[pos // 3 + np.r_[0:108, 119:227]]
    bits = np.stack([(s >> 1) & 1, s & 1], axis=1).reshape(-1)
    return np.where(bits == 1, -127, 127).astype(np.int8)


def test_codec_frame_equals_the_reference_frames():
    from tetraear.core.etsi import codec_frame
    z = _fixture()
    pos, none, words = z["position"], z["none"], z["words"]
    assert len(pos) >= 14 and none.sum() >= 2 and (~none).sum() >= 12
    for i in range(len(pos)):
        sym = z[f"sym_{i}"]
        if none[i]:   # no position, or a slot past the stream's end
            assert pos[i] < 0 or pos[i] // 3 + 255 > len(sym)
            continue
        assert 300 <= len(sym) <= 600 and pos[i] // 3 + 255 <= len(sym)
        got = codec_frame(_soft_of_symbols(sym, int(pos[i])))
        assert isinstance(got, bytes) and len(got) == 1380
        assert np.array_equal(np.frombuffer(got, "<i2"), words[i]), i
    w = words[0]
    assert w[0] == 0x6B21 and set(np.abs(w[np.r_[1:115, 116:230, 231:345, 346:436]]).tolist()) == {127}
    assert not w[np.r_[115, 230, 345, 436:690]].any()


def test_codec_frame_options_and_errors():
    from tetraear.core.etsi import codec_frame
    rng = np.random.default_rng(1)
    soft = rng.integers(-128, 128, 432).astype(np.int8)
    soft[:2] = [-128, 127]
    ref = np.frombuffer(codec_frame(soft), "<i2")
    inv = np.frombuffer(codec_frame(soft, polarity="inverted"), "<i2")
    assert ref[1] == 127 and ref[2] == -127 and inv[1] == -127 and inv[2] == 127
    body = np.r_[1:115, 116:230, 231:345, 346:436]
    assert np.array_equal(ref[body], np.clip(-soft.astype(np.int64), -127, 127))
    assert np.array_equal(inv[body], np.clip(soft.astype(np.int64), -127, 127)) and inv[0] == ref[0] == 0x6B21
    mk = np.frombuffer(codec_frame(soft, block_markers=True), "<i2")
    assert [int(mk[115 * i]) for i in range(1, 6)] == [0x6B21 + i for i in range(1, 6)]
    rest = np.setdiff1d(np.arange(690), 115 * np.arange(1, 6))
    assert np.array_equal(mk[rest], ref[rest]) and not ref[115 * np.arange(1, 6)].any()
    for bad in (soft[:216], soft[:431], np.zeros((2, 216), np.int8), np.zeros(0, np.int8)):
        with pytest.raises(ValueError):
            codec_frame(bad)
    with pytest.raises(ValueError):
        codec_frame(soft, polarity="up")


# ------------------------------------------------------------------------------ the frame helpers

def test_traffic_streams_and_slot_usage():
    from tetraear.core.etsi import slot_usage, traffic_streams
    fr = [dict(position=p, tn=tn, usage=u) for p, tn, u in
          ((0, 1, "sync"), (510, 2, "traffic"), (1020, 3, "control"), (1530, 4, "lost"), (2040, 1, "control"),
           (2550, 2, "traffic"), (3060, 3, "stolen"), (3570, 4, None), (4080, 2, "control"), (4590, 3, "traffic"))]
    st = traffic_streams(fr)
    assert {k: [f["position"] for f in v] for k, v in st.items()} == {2: [510, 2550], 3: [4590]}
    assert st[2][0] is fr[1]
    assert slot_usage(fr) == {1: {"sync": 1, "control": 1}, 2: {"traffic": 2, "control": 1},
                              3: {"control": 1, "stolen": 1, "traffic": 1}, 4: {"lost": 1, None: 1}}
    # without a timebase (no tn key, or tn None) everything is under None
    bare = [dict(position=0, usage="traffic"), dict(position=510, usage="traffic", tn=None), dict(position=1020, usage="sync")]
    assert [f["position"] for f in traffic_streams(bare)[None]] == [0, 510] and list(traffic_streams(bare)) == [None]
    assert slot_usage(bare) == {None: {"traffic": 2, "sync": 1}}
    assert traffic_streams([]) == {} and slot_usage([]) == {}


def test_frames_gain_the_keys_only_with_traffic():
    """build_frames on hand-made records: without the traffic records the frames have today's key
    set; with them every frame gains usage and traffic, None for a channel without a cell."""
    from tetraear import _hip
    from tetraear.core.etsi import EtsiLowerMac, LowerMac, Traffic, build_frames, traffic_keys
    nb, nk = np.array([3, 1], np.int32), np.array([3, 1], np.int32)
    bursts = np.zeros((2, 8, 2), np.int32)
    bursts[0, :3] = [(10, 0), (520, 2), (1030, 1)]
    bursts[1, 0] = (4, 0)
    blocks = np.zeros((2, 16, 4), np.int32)
    blocks[0, :3] = [(0, 0, 0, 0), (2, 1, 1, 0), (1, 1, 2, 0)]
    t1 = np.zeros((2, 16, 268), np.uint8)
    lm = LowerMac(nb, bursts, nk, blocks, t1)
    plain = build_frames(lm)
    assert all(set(f) == {"position", "burst", "burst_kind", "timeslot", "blocks", "crc_ok"} for fr in plain for f in fr)
    tq = np.full((2, 8, 4), -1, np.int32)
    tq[0, :3] = [(_hip.TCH_FULL, 432, 999, 2), (_hip.TCH_NONE, 0, 0, 0), (_hip.TCH_HALF, 216, 500, 1)]
    tq[1, 0] = (_hip.TCH_FULL, 432, 7, 0)
    tch = np.arange(2 * 8 * 432).reshape(2, 8, 432).astype(np.int8)
    got = build_frames(lm, tr=Traffic(tq, tch, np.array([True, False])))
    assert [{k: v for k, v in f.items() if k not in ("usage", "traffic", "blocks")} for fr in got for f in fr] == \
        [{k: v for k, v in f.items() if k != "blocks"} for fr in plain for f in fr]
    assert [f["usage"] for f in got[0]] == ["traffic", "sync", "stolen"] and got[1][0]["usage"] is None
    assert got[1][0]["traffic"] is None and got[0][1]["traffic"] is None
    a, h = got[0][0]["traffic"], got[0][2]["traffic"]
    assert (a["bits"], a["soft_sum"], a["erased"]) == (432, 999, 2) and np.array_equal(a["soft"], tch[0, 0])
    assert (h["bits"], h["soft_sum"], h["erased"]) == (216, 500, 1) and np.array_equal(h["soft"], tch[0, 2, :216])
    assert a["soft"].dtype == np.int8 and a["soft"].base is None   # a copy: the frame owns it
    for cls, kind, usage in ((_hip.TCH_CONTROL, 0, "control"), (_hip.TCH_LOST, 1, "lost"), (_hip.TCH_NONE, 0, None),
                             (-1, 0, None)):
        assert traffic_keys([cls, 0, 0, 0] if cls >= 0 else [-1] * 4, tch[0, 0], kind) == {"usage": usage, "traffic": None}
    assert not EtsiLowerMac().traffic and EtsiLowerMac(traffic=True).traffic
    from tetraear.core import TetraDecoder
    assert not TetraDecoder(auto_decrypt=False, mode="etsi").etsi_traffic
    assert TetraDecoder(auto_decrypt=False, mode="etsi", traffic=True).etsi_traffic
