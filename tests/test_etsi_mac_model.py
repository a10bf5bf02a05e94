"""tests/_etsi_mac_model.py on the CPU: the builders and the walk agree (fields in, bits out, fields
back), the SYNC offsets are those the lower MAC already relies on, the offsets are those of the
type-1 bits the oracle's lower MAC emits, and the timebase rules hold at their edges.  What
tests/test_gpu_etsi_mac.py compares k_etsi_mac against is checked here first.  Integers only.
"""
import numpy as np
import pytest

import etsi as E
import _lmac_rows as R
import _etsi_mac_model as M


def _rng(seed=0):
    return np.random.default_rng(seed)


def test_constants_match_the_binding():
    from tetraear import _hip
    assert (M.MAXB, M.MAXJ, M.MAXPDU, M.NF) == (_hip.ETSI_MAXB, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.PDU_FIELDS)
    assert (M.TDMA_SLOTS, M.TDMA_TOL, M.TDMA_EXPIRE) == (_hip.TDMA_SLOTS, _hip.TDMA_TOL, _hip.TDMA_EXPIRE)
    assert M.TDMA_DTYPE == _hip.ETSI_TDMA and _hip.ETSI_TDMA.itemsize == 24
    assert M.TDMA_SLOTS == 60 * 18 * 4
    assert (M.RESOURCE, M.NULL, M.SYNC) == (_hip.PDU_RESOURCE, _hip.PDU_NULL, _hip.PDU_SYNC)


# ------------------------------------------------------------------------------ builder -> walk

@pytest.mark.parametrize("addr_type", range(1, 8))
def test_resource_every_address_type(addr_type):
    rng = _rng(addr_type)
    has_ssi, auxn = M.ADDRESS[addr_type]
    for kind in (0, 1):
        ssi, aux = int(rng.integers(0, 1 << 24)), int(rng.integers(0, 1 << max(auxn, 1)))
        f = dict(fill=int(rng.integers(0, 2)), grant=int(rng.integers(0, 2)), enc=int(rng.integers(0, 4)),
                 random_access=int(rng.integers(0, 2)))
        blk = M.block(rng, kind, [M.resource(rng, 9, addr_type, ssi, aux, **f), M.null_pdu()])
        recs = M.walk(blk, kind)
        hdr = 16 + 24 * has_ssi + auxn
        assert recs[0] == [M.RESOURCE, 0, 72, 0, f["fill"], f["enc"], 9, addr_type, ssi if has_ssi else -1,
                           aux if auxn else -1, hdr, f["grant"] | f["random_access"] << 1, 0, 0, 0, 0]
        assert len(recs) == 2 and recs[1][:4] == [M.NULL, 72, 16, 0]


def test_every_kind():
    rng = _rng(1)
    blk = M.block(rng, 0, [M.mac_end(rng, 5, fill=1, grant=1), M.resource(rng, 8, 1, ssi=0xABCDEF),
                          M.mac_frag(rng, 50, fill=1)])
    recs = M.walk(blk, 0)
    assert [r[0] for r in recs] == [M.END, M.RESOURCE, M.FRAG]
    assert recs[0] == [M.END, 0, 40, 0, 1, 0, 5, 0, -1, -1, 11, 1, 0, 0, 0, 0]
    assert recs[1][:4] == [M.RESOURCE, 40, 64, 0] and recs[1][8] == 0xABCDEF
    assert recs[2] == [M.FRAG, 104, 268 - 104, 0, 1, 0, 0, 0, -1, -1, 4, 0, 0, 0, 0, 0]
    for sub, want in ((1, M.ACCESS_DEFINE), (2, M.BROADCAST), (3, M.BROADCAST)):
        recs = M.walk(M.block(rng, 1, [M.broadcast(rng, sub, 124)]), 1)
        assert recs == [[want, 0, 124, 0] + [0] * 12]
    recs = M.walk(M.block(rng, 1, [M.mac_end(rng, 3), M.supplementary(rng, 100)]), 1)
    assert [r[:4] for r in recs] == [[M.END, 0, 24, 0], [M.SUPPL, 24, 100, 0]] and recs[1][4:] == [0] * 12
    assert M.walk(M.block(rng, 0, [M.null_pdu(fill=1, grant=1, enc=2, random_access=1, length=5)]), 0) == \
        [[M.NULL, 0, 16, 0, 1, 2, 5, 0, -1, -1, 16, 3, 0, 0, 0, 0]]


def test_length_indication():
    rng = _rng(2)

    def first(kind, pdu):
        return M.walk(M.block(rng, kind, [pdu]), kind)

    # L = 1: malformed; L = 2 with an address: the header runs past the PDU end
    assert first(0, M.resource(rng, 1, 1, nbits=40))[0][:4] == [M.RESOURCE, 0, 268, 1]
    r = first(0, M.resource(rng, 2, 1))
    assert len(r) == 1 and r[0][:4] == [M.RESOURCE, 0, 16, 1] and r[0][8] == -1 and r[0][10] == 40
    r = first(0, M.resource(rng, 4, 5, ssi=5, aux=3))   # 32 bits, the header needs 50
    assert len(r) == 1 and r[0][2:4] == [32, 1] and (r[0][8], r[0][9]) == (-1, -1)
    # L = 2 on a MAC-END is a whole PDU of 16 bits and the walk goes on
    r = first(0, M.mac_end(rng, 2))
    assert r[0][:4] == [M.END, 0, 16, 0] and len(r) >= 2 and r[1][1] == 16
    # L = 34: cut at 268 on SCH/F (272 - 268 < 8), malformed on SCH/HD
    r = first(0, M.resource(rng, 34, 1, ssi=77))
    assert r == [[M.RESOURCE, 0, 268, 0, 0, 0, 34, 1, 77, -1, 40, 0, 0, 0, 0, 0]]
    r = first(1, M.resource(rng, 34, 1, ssi=77))
    assert len(r) == 1 and r[0][:4] == [M.RESOURCE, 0, 124, 1] and r[0][8] == 77
    # a second PDU whose 8 L runs 4 bits past the block end is cut; 12 bits past is malformed
    r = M.walk(M.block(rng, 0, [M.mac_end(rng, 4), M.resource(rng, 30, 1)]), 0)   # 32 + 240 = 272
    assert [x[:4] for x in r] == [[M.END, 0, 32, 0], [M.RESOURCE, 32, 236, 0]]
    r = M.walk(M.block(rng, 0, [M.mac_end(rng, 5), M.resource(rng, 30, 1)]), 0)   # 40 + 240 = 280
    assert [x[:4] for x in r] == [[M.END, 0, 40, 0], [M.RESOURCE, 40, 228, 1]]
    for L, bad in ((0, 1), (35, 1), (61, 1), (62, 0), (63, 0)):
        r = first(0, M.resource(rng, L, 3, ssi=9, nbits=100))
        assert r == [[M.RESOURCE, 0, 268, bad, 0, 0, L, 3, 9, -1, 40, 0, 0, 0, 0, 0]], (L, r)
        r = first(1, M.mac_end(rng, L, nbits=60))
        assert r == [[M.END, 0, 124, bad, 0, 0, L, 0, -1, -1, 11, 0, 0, 0, 0, 0]], (L, r)


def test_short_pdus_up_to_the_block_end():
    """As many short PDUs as a block holds: sixteen 16-bit ones on SCH/F (268 // 16; a seventeenth
    has 12 bits left and is not counted), fifteen and a null PDU, seven on SCH/HD."""
    rng = _rng(3)
    r = M.walk(M.block(rng, 0, [M.mac_end(rng, 2) for _ in range(17)]), 0)
    assert len(r) == 16 and [x[1] for x in r] == list(range(0, 256, 16)) and all(x[0] == M.END for x in r)
    r = M.walk(M.block(rng, 0, [M.mac_end(rng, 2) for _ in range(15)] + [M.null_pdu()]), 0)
    assert len(r) == 16 and r[-1][:4] == [M.NULL, 240, 16, 0]
    r = M.walk(M.block(rng, 0, [M.mac_end(rng, 2) for _ in range(5)] + [M.null_pdu()] +
                       [M.mac_end(rng, 2) for _ in range(5)]), 0)
    assert len(r) == 6   # nothing follows a null PDU
    r = M.walk(M.block(rng, 1, [M.mac_end(rng, 2) for _ in range(9)]), 1)
    assert len(r) == 7 and r[-1][1] == 96


def test_sysinfo_round_trip_and_truncation():
    rng = _rng(4)
    for _ in range(20):
        f = M.random_fields(rng, M.SYSINFO_LAYOUT)
        for kind in (0, 1):
            r = M.walk(M.block(rng, kind, [M.sysinfo(f)]), kind)
            assert len(r) == 1 and r[0][:4] == [M.SYSINFO, 0, 124, 0]
            assert r[0][4:12] == [f[k] for k in ("main_carrier", "band", "offset", "duplex_spacing",
                                                 "reverse_operation", "num_cscch", "ms_txpwr_max_cell",
                                                 "rxlev_access_min")]
            assert r[0][12] == f["access_parameter"] | f["radio_downlink_timeout"] << 4 | f["optional_field_flag"] << 8
            assert r[0][13] == f["hyperframe_cck_flag"] << 16 | f["hyperframe_or_cck"]
            assert r[0][14:] == [f["location_area"], f["subscriber_class"] | f["bs_service_details"] << 16]
    # after an associated PDU: fits on SCH/F at 144 (144 + 124 = 268), not at 152; never on SCH/HD past 0
    f = M.random_fields(rng, M.SYSINFO_LAYOUT)
    r = M.walk(M.block(rng, 0, [M.mac_end(rng, 18), M.sysinfo(f)]), 0)
    assert r[1][:5] == [M.SYSINFO, 144, 124, 0, f["main_carrier"]]
    r = M.walk(M.block(rng, 0, [M.mac_end(rng, 19), M.sysinfo(f)]), 0)
    assert r[1] == [M.SYSINFO, 152, 116, 1] + [0] * 12
    r = M.walk(M.block(rng, 1, [M.mac_end(rng, 2), M.sysinfo(f)]), 1)
    assert r[1] == [M.SYSINFO, 16, 108, 1] + [0] * 12


def test_sync_round_trip_and_cell_init():
    """The model's colour code, MCC and MNC give bsch_cell_init's scrambling init on random blocks:
    the offsets the lower MAC already descrambles by."""
    rng = _rng(5)
    for _ in range(200):
        t = rng.integers(0, 2, 60).astype(np.uint8)
        rec, f = M.parse_sync(t.tolist())
        assert E.scramble_init(f["mcc"], f["mnc"], f["colour_code"]) == E.bsch_cell_init(t)
        assert (rec[5], rec[12], rec[13]) == (f["colour_code"], f["mcc"], f["mnc"])
        assert np.array_equal(M.block(rng, 2, [M.sync(f)]), t)   # every one of the 60 bits is a field's
    f = M.sync_for_slot(rng, 4319)
    assert (f["tn"], f["fn"], f["mn"]) == (3, 18, 60) and M.slot_of(f) == 4319
    rec = M.walk(M.block(rng, 2, [M.sync(f)]), 2)[0]
    assert rec[:4] == [M.SYNC, 0, 60, 0] and rec[6:9] == [3, 18, 60]
    assert rec[11] == f["dtx"] | f["frame18_extension"] << 1 | f["late_entry"] << 2
    for over in (dict(fn=0), dict(fn=19), dict(mn=0), dict(mn=61)):
        assert M.walk(M.block(rng, 2, [M.sync(M.sync_for_slot(rng, 100, **over))]), 2)[0][3] == 1


def test_walk_reads_nothing_past_the_block():
    """Random blocks of every kind, with the bytes past n1 poisoned, walk without touching them and
    tile the block: every record starts where the one before ended."""
    rng = _rng(6)
    for _ in range(300):
        kind = int(rng.integers(0, 3))
        t = np.full(268, 0x7e, np.uint8)
        t[:M.N1[kind]] = rng.integers(0, 256, M.N1[kind])
        recs = M.walk(t, kind)
        assert 1 <= len(recs) <= 16
        for a, b in zip(recs, recs[1:]):
            assert a[3] == 0 and b[1] == a[1] + 8 * a[6]
        assert recs[-1][1] + recs[-1][2] <= M.N1[kind]


def test_offsets_are_those_of_the_lower_macs_type1_bits():
    """Bursts built from the builders' payloads and decoded by the oracle's lower MAC hand the built
    fields back."""
    rng = _rng(7)
    init, cell = R.cell_fields(rng)
    fs, fi = M.sync_for_slot(rng, 1234, cell), M.random_fields(rng, M.SYSINFO_LAYOUT)
    pays = [[M.block(rng, 2, [M.sync(fs)]), M.block(rng, 1, [M.sysinfo(fi)])],
            [M.block(rng, 0, [M.resource(rng, 10, 6, ssi=0x123456, aux=33, enc=1), M.null_pdu()])],
            [M.block(rng, 1, [M.mac_frag(rng, 124)]), M.block(rng, 1, [M.mac_end(rng, 7, fill=1)])]]
    bits, planted, jobs = R.place_bursts(rng, [(5, R.SB, init, [p.copy() for p in pays[0]]),
                                               (0, R.NDB_N, init, [p.copy() for p in pays[1]]),
                                               (0, R.NDB_P, init, [p.copy() for p in pays[2]])])
    dec = E.Receiver().lower_mac(R.soft_of(bits), R.hard_of(bits), init)
    assert [(s, k) for s, k, _ in dec] == planted
    got = [[M.walk(t1, k) for k, t1, ok in blocks if ok] for _, _, blocks in dec]
    assert got[0][0][0][6:9] == [fs["tn"], fs["fn"], fs["mn"]] and got[0][0][0][12:14] == [cell[0], cell[1]]
    assert got[0][1][0][:5] == [M.SYSINFO, 0, 124, 0, fi["main_carrier"]] and got[0][1][0][14] == fi["location_area"]
    assert got[1][0][0][:12] == [M.RESOURCE, 0, 80, 0, 0, 1, 10, 6, 0x123456, 33, 46, 0]
    assert got[1][0][1][:3] == [M.NULL, 80, 16]
    assert got[2][0][0][0] == M.FRAG and got[2][1][0][:5] == [M.END, 0, 56, 0, 1]


# ------------------------------------------------------------------------------ the timebase

def _one(t, start, own=None, kind=0, nsym=1):
    return t.chunk(nsym, [(start, kind)], [own])[0]


def test_timebase_unlocked_then_locked_then_wraps():
    t = M.Tdma()
    assert _one(t, 100) == [0, 0, 0, 0] and not t.locked
    assert _one(t, 610, own=4318, kind=2) == [3, 18, 60, 1]
    assert _one(t, 1120) == [4, 18, 60, 0]          # slot 4319
    assert _one(t, 1630) == [1, 1, 1, 0]            # wraps to 0
    assert _one(t, 1630 + 1020) == [3, 1, 1, 0]     # one missed burst: k = 2
    assert t.state() == (0, 2650, 2, 1)


def test_timebase_tolerance_and_reanchoring():
    for r in (4, -4):
        t = M.Tdma(0, 1000, 10, 1)
        assert _one(t, 1510 + r) == [4, 3, 1, 0] and t.anchor_bit == 1510 + r   # taken, re-anchored
    for r in (5, -5):
        t = M.Tdma(0, 1000, 10, 1)
        assert _one(t, 1510 + r) == [0, 0, 0, 0] and t.state() == (0, 1000, 10, 1)   # refused, anchor kept
        assert _one(t, 2020) == [1, 4, 1, 0]    # the next on-grid burst: k = 2 from the kept anchor


def test_timebase_expiry():
    t = M.Tdma(0, 1000, 10, 1)
    assert _one(t, 1000 + 71 * 510) == [(10 + 71) % 4 + 1, (10 + 71) // 4 % 18 + 1, 2, 0]
    t = M.Tdma(0, 1000, 10, 1)
    assert _one(t, 1000 + 72 * 510) == [0, 0, 0, 0] and not t.locked
    assert _one(t, 1000 + 73 * 510) == [0, 0, 0, 0]
    t = M.Tdma(0, 1000, 10, 1)
    assert _one(t, 999) == [0, 0, 0, 0] and not t.locked    # before the anchor: d < 0


def test_timebase_own_sync_wins_and_flags():
    t = M.Tdma(0, 1000, 10, 1)
    assert _one(t, 1510, own=11, kind=2) == [4, 3, 1, 1]         # agrees
    assert _one(t, 2020, own=500, kind=2) == [1, 18, 7, 3]       # contradicts: wins, bit 1
    assert _one(t, 2530) == [2, 18, 7, 0]
    assert _one(t, 2530 + 515, own=7, kind=2) == [4, 2, 1, 3]    # off the grid: rule 2 gave none
    t = M.Tdma(0, 1000, 10, 1)
    assert _one(t, 1000 + 80 * 510, own=3, kind=2) == [4, 1, 1, 3] and t.locked   # expired, then its own SYNC
    t = M.Tdma()
    assert _one(t, 0, own=3, kind=2) == [4, 1, 1, 1]             # not locked before: no bit 1


def test_timebase_large_bit0_negative_start_and_carry():
    t = M.Tdma(bit0=1 << 40)
    assert t.chunk(1001, [(-300, 2), (210, 0)], [8, None]) == [[1, 3, 1, 1], [2, 3, 1, 0]]
    assert t.state() == ((1 << 40) + 2000, (1 << 40) + 210, 9, 1)
    assert t.chunk(0, [], []) == [] and t.bit0 == (1 << 40) + 2000
    assert t.chunk(256, [(-2000 + 210 + 510 * 3, 1)], [None]) == [[1, 4, 1, 0]]


def test_run_takes_the_sync_of_the_bursts_own_block():
    """run(): an SB's slot comes from block q of the sync kernel's numbering, only when that block is
    a CRC-good BSCH with a valid SYNC; entries past the counts are not read."""
    rng = _rng(8)
    bursts = np.full((1, 8, 2), 99, np.int32)
    blocks = np.full((1, 16, 4), 99, np.int32)
    type1 = np.full((1, 16, 268), 0x7e, np.uint8)
    bursts[0, :3] = [(0, 0), (510, 2), (1020, 2)]
    blocks[0, :5, :2] = [(0, 1), (2, 1), (1, 0), (2, 0), (1, 1)]
    type1[0, 0] = M.block(rng, 0, [M.null_pdu()])
    type1[0, 1, :60] = M.block(rng, 2, [M.sync(M.sync_for_slot(rng, 41))])
    type1[0, 3, :60] = M.block(rng, 2, [M.sync(M.sync_for_slot(rng, 99))])   # CRC-bad: no anchor
    type1[0, 4, :124] = M.block(rng, 1, [M.supplementary(rng, 124)])
    t = [M.Tdma()]
    npdu, recs, rows = M.run([1531], [3], bursts, [5], blocks, type1, t)
    assert npdu[0].tolist() == [1, 1, 0, 0, 1] + [0] * 11 and sorted(recs) == [(0, 0), (0, 1), (0, 4)]
    assert rows == {(0, 0): [0, 0, 0, 0], (0, 1): [2, 11, 1, 1], (0, 2): [3, 11, 1, 0]}
    assert t[0].state() == (3060, 1020, 42, 1)


def test_lower_mac_with_mac_constructs_without_a_gpu():
    from tetraear.core.etsi import EtsiLowerMac, pdu_dict
    lm = EtsiLowerMac(mac=True)
    assert lm.mac and lm._tdma is None and not EtsiLowerMac().mac
    from tetraear.core.decoder import TetraDecoder
    assert TetraDecoder(auto_decrypt=False, mode="etsi", mac=True).etsi_mac
    rng = _rng(9)
    f = M.random_fields(rng, M.SYSINFO_LAYOUT)
    d = pdu_dict(M.walk(M.block(rng, 1, [M.sysinfo(f)]), 1)[0])
    # ("offset" is the record's bit offset in the dict: SYSINFO's own offset field is carrier_offset)
    assert all(d[{"offset": "carrier_offset"}.get(k, k)] == v for k, v in f.items() if k != "optional_field_value")
    assert (d["kind"], d["offset"], d["nbits"], d["ok"]) == ("SYSINFO", 0, 124, True)
    assert d["downlink_hz"] == f["band"] * 100e6 + f["main_carrier"] * 25e3 + {0: 0, 1: 6250, 2: -6250, 3: 12500}[f["offset"]]
    fs = M.sync_for_slot(rng, 77)
    d = pdu_dict(M.walk(M.block(rng, 2, [M.sync(fs)]), 2)[0])
    assert all(d[k] == v for k, v in fs.items() if k != "reserved") and d["kind"] == "SYNC" and d["ok"]
