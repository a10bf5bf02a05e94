"""build_frames (tetraear/core/etsi.py) on hand-made records that carry every stage's bundle at once, four rows
in G = 2 groups: which frame, block and PDU each record lands on.  No GPU."""
import numpy as np
import pytest

from tetraear import _hip
from tetraear.core.etsi import LinkQuality, Llc, LowerMac, Mac, Sdu, Traffic, build_frames, chain_options

C, G, MAXD = 4, 2, 2
TIMEBASE_KEYS = {"tn", "fn", "mn", "slot_flags"}


def records():
    lm = LowerMac.zeros(C)
    lm.nb[:], lm.nk[:] = (2, 1, 1, 2), (3, 1, 2, 3)
    lm.bursts[0, :2] = [(10, 0), (520, 1)]
    lm.bursts[1, 0] = (4, 0)
    lm.bursts[2, 0] = (30, 2)
    lm.bursts[3, :2] = [(8, 0), (518, 1)]
    # (block kind, crc ok, burst, index in the burst)
    lm.blocks[0, :3] = [(0, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 1)]
    lm.blocks[1, 0] = (0, 1, 0, 0)
    lm.blocks[2, :2] = [(2, 1, 0, 0), (1, 1, 0, 1)]
    lm.blocks[3, :3] = [(0, 0, 0, 0), (1, 1, 1, 0), (1, 1, 1, 1)]
    lm.t1[:] = np.arange(C * _hip.ETSI_MAXJ * 268).reshape(lm.t1.shape) % 2
    mac = Mac.zeros(C)
    mac.slots[0, :2] = [(0, 0, 0, 0), (2, 5, 7, 4)]
    mac.slots[3, :2] = [(1, 18, 60, 0), (2, 18, 60, 1)]
    mac.npdu[0, :3], mac.npdu[3, 1], mac.npdu[2, 1] = (2, 1, 0), 1, 1
    mac.pdus[..., _hip.PDU_KIND] = _hip.PDU_RESOURCE
    mac.pdus[..., _hip.PDU_SSI] = np.arange(C * _hip.ETSI_MAXJ * _hip.ETSI_MAXPDU).reshape(mac.pdus.shape[:3])
    lq = LinkQuality(np.arange(C * _hip.ETSI_MAXB * 4, dtype=np.int32).reshape(C, _hip.ETSI_MAXB, 4),
                     1000 + np.arange(C * _hip.ETSI_MAXJ * 4, dtype=np.int32).reshape(C, _hip.ETSI_MAXJ, 4))
    tq = np.full((C, _hip.ETSI_MAXB, 4), -1, np.int32)
    tq[:, :2, _hip.TQ_CLASS], tq[:, :2, _hip.TQ_NBITS] = _hip.TCH_FULL, 432
    tr = Traffic(tq, np.ones((C, _hip.ETSI_MAXB, 432), np.int8), np.array([True, True, False, False]))
    sdu = np.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.SDU_FIELDS), np.int32)
    sdu[0, 0, 0, [_hip.SDU_NBITS, _hip.SDU_BYTE]] = (16, 0)
    sdu[0, 0, 1, [_hip.SDU_NBITS, _hip.SDU_BYTE]] = (8, 5)
    sdu[3, 1, 0, [_hip.SDU_NBITS, _hip.SDU_BYTE]] = (12, 9)
    rows = (np.arange(C * _hip.ETSI_MAXJ * _hip.SDU_ROW) % 251).astype(np.uint8).reshape(C, _hip.ETSI_MAXJ, _hip.SDU_ROW)
    done = np.zeros((C // G, MAXD, _hip.DONE_FIELDS), np.int32)
    where = [_hip.DONE_ROW, _hip.DONE_BURST, _hip.DONE_BLOCK, _hip.DONE_NBITS, _hip.DONE_PDU]
    done[0, 0, where] = (0, 1, 2, 24, 0)    # group 0: row 0, burst 1, its second block
    done[1, 0, where] = (3, 1, 1, 16, 0)    # group 1: its second row, burst 1, the burst's first block
    done[1, 1, where] = (2, 0, 1, 8, 1)     # group 1: its first row, the SB's second block
    done_data = (7 + np.arange(C // G * MAXD * _hip.SDU_MAXBYTES) % 241).astype(np.uint8).reshape(C // G, MAXD, -1)
    sd = Sdu(sdu, rows, np.array([1, 5], np.int32), done, done_data)   # group 1 completed more than maxd returns
    llc = np.zeros(sdu.shape[:3] + (_hip.LLC_FIELDS,), np.int32)
    llc[..., _hip.LLC_NBITS], llc[..., _hip.LLC_HEAD], llc[..., [_hip.LLC_NR, _hip.LLC_NS]] = 8, -1, -1
    llc_done = np.zeros((C // G, MAXD, _hip.LLC_FIELDS), np.int32)
    llc_done[..., _hip.LLC_NBITS], llc_done[..., _hip.LLC_HEAD], llc_done[..., _hip.LLC_TYPE] = 16, -1, [[1, 2], [3, 4]]
    tl_done = (3 + np.arange(C // G * MAXD * _hip.SDU_MAXBYTES) % 239).astype(np.uint8).reshape(done_data.shape)
    ll = Llc(llc, (rows.astype(np.int32) + 100).astype(np.uint8), llc_done, tl_done)
    return lm, mac, lq, tr, sd, ll


def test_every_record_lands_on_its_frame():
    lm, mac, lq, tr, sd, ll = records()
    out = build_frames(lm, mac, lq, tr, sd, ll, G)
    assert [len(fr) for fr in out] == [2, 1, 1, 2]
    assert [[len(f["blocks"]) for f in fr] for fr in out] == [[1, 2], [1], [2], [1, 2]]
    # sdus: on the row, burst and block DONE_ROW / DONE_BURST / DONE_BLOCK point to, and no more than maxd a group
    got = {(r, b): f["sdus"] for r, fr in enumerate(out) for b, f in enumerate(fr) if "sdus" in f}
    assert sorted(got) == [(0, 1), (2, 0), (3, 1)] and all(len(v) == 1 for v in got.values())
    assert [(got[k][0]["block"], got[k][0]["pdu"], got[k][0]["nbits"]) for k in sorted(got)] == \
        [(1, 0, 24), (1, 1, 8), (0, 0, 16)]
    assert got[(0, 1)][0]["data"] == bytes(sd.done_data[0, 0, :3]) and got[(3, 1)][0]["data"] == bytes(sd.done_data[1, 0, :2])
    assert got[(2, 0)][0]["data"] == bytes(sd.done_data[1, 1, :1])
    # ... each with the LLC record and TL-SDU of its own done slot
    assert [(got[k][0]["llc"]["type"], got[k][0]["llc"]["tl_sdu"]) for k in sorted(got)] == \
        [(1, bytes(ll.tl_done[0, 0, :2])), (4, bytes(ll.tl_done[1, 1, :2])), (3, bytes(ll.tl_done[1, 0, :2]))]
    # a PDU's SDU from the block's sdu_data row, its llc from the tl row at the PDU's SDU_BYTE
    p0, p1 = out[0][0]["blocks"][0]["pdus"]
    assert (p0["sdu"], p1["sdu"]) == (bytes(sd.sdu_data[0, 0, 0:2]), bytes(sd.sdu_data[0, 0, 5:6]))
    assert (p0["llc"]["tl_sdu"], p1["llc"]["tl_sdu"]) == (bytes(ll.tl[0, 0, 0:1]), bytes(ll.tl[0, 0, 5:6]))
    q = out[3][1]["blocks"][0]["pdus"][0]
    assert q["sdu"] == bytes(sd.sdu_data[3, 1, 9:11]) and q["llc"]["tl_sdu"] == bytes(ll.tl[3, 1, 9:10])
    assert (p0["ssi"], p1["ssi"], q["ssi"]) == tuple(int(mac.pdus[i][_hip.PDU_SSI]) for i in ((0, 0, 0), (0, 0, 1), (3, 1, 0)))
    assert [b["npdu"] for fr in out for f in fr for b in f["blocks"]] == [2, 1, 0, 0, 0, 1, 0, 1, 0]
    # the timebase of the burst's own slots record, None while tn is 0
    assert [(f["tn"], f["fn"], f["mn"], f["slot_flags"]) for f in out[0] + out[3]] == \
        [(None, None, None, 0), (2, 5, 7, 4), (1, 18, 60, 0), (2, 18, 60, 1)]
    # link quality: the burst's bq record, the block's kq record
    assert out[3][1]["training_errors"] == int(lq.bq[3, 1, _hip.BQ_TERR])
    assert out[3][1]["blocks"][1]["channel_errors"] == int(lq.kq[3, 2, _hip.LQ_NERR])
    # traffic: has_cell False yields usage None
    assert [[f["usage"] for f in fr] for fr in out] == [["traffic", "traffic"], ["traffic"], [None], [None, None]]
    assert out[2][0]["traffic"] is None and out[0][0]["traffic"]["bits"] == 432


def test_slots_not_reported_leaves_the_timebase_keys_out():
    lm, mac, lq, tr, sd, ll = records()
    full = build_frames(lm, mac, lq, tr, sd, ll, G)
    walk = build_frames(lm, mac._replace(slots_reported=False), lq, tr, sd, ll, G)
    for a, b in zip((f for fr in full for f in fr), (f for fr in walk for f in fr)):
        assert set(a) - set(b) == TIMEBASE_KEYS and not TIMEBASE_KEYS & set(b)
        assert all("pdus" in blk and "npdu" in blk for blk in b["blocks"])
        assert repr({k: v for k, v in a.items() if k not in TIMEBASE_KEYS}) == repr(b)
    bare = build_frames(lm)
    assert all(set(f) == {"position", "burst", "burst_kind", "timeslot", "blocks", "crc_ok"} for fr in bare for f in fr)
    assert not any("pdus" in blk for fr in bare for f in fr for blk in f["blocks"])


def test_option_rules_name_the_timebase_variant():
    assert chain_options().timebase is None and chain_options(mac=True).timebase == "mac"
    assert chain_options(mac=True, timebase="vote").timebase == "vote"
    assert [chain_options(mac=m, timebase=t, grouped=True).timebase for m, t in
            ((False, False), (True, False), (False, True), (True, True), (False, "vote"))] == \
        [None, "walk", "groups", "groups", "vote"]
    for kw in (dict(sdu=True), dict(mac=True, llc=True), dict(timebase="vote"), dict(timebase="yes"),
               dict(mac=True, timebase="vote", tdma_cap=0), dict(vote_cap=0),
               dict(mac=True, sdu=True, grouped=True), dict(timebase=True, sdu=True, grouped=True),
               dict(mac=True, timebase=True, llc=True, grouped=True), dict(timebase="vote", tdma_cap=-1, grouped=True)):
        with pytest.raises(ValueError):
            chain_options(**kw)
    assert chain_options(mac=True, timebase=True, sdu=True, llc=True, grouped=True).llc
