"""tetra_etsi_sdu's CPU model against typed-out vectors, an independent writer and fragmenter, and every
rule of the fragment walk at its edge; then the checks of the new surfaces that need no GPU."""
import os
import re

import numpy as np
import pytest

import _etsi_mac_model as M
import _etsi_sdu_cases as K
import _etsi_sdu_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(*parts):
    return [int(ch) for ch in "".join(parts).replace(" ", "")]


def first_record(block_bits, kind, q=0):
    """The model's Part A record and SDU bits of PDU q of a block typed out as bits."""
    recs = M.walk(np.array(block_bits, np.uint8), kind)
    return S.sdu_of(list(block_bits), recs[q])


# ------------------------------------------------------------------------------ 1. literal vectors
# Each: the block's leading bits typed out (zeros follow), block kind, PDU index, and the expected STATUS,
# OFFSET, NBITS, ROLE, ELEMS, POWER_GRANT, CHAN and bytes, worked by hand from the layout tables.
NULL = "0000000 000010 000"
VECTORS = {
    # MAC-RESOURCE, L = 7, address type 1 (SSI 0xABCDEF), the three element flags 0, 13 SDU bits, a null PDU
    "resource, ssi, no elements": (
        bits("00 0 0 00 0 000111 001", "1010 1011 1100 1101 1110 1111", "0 0 0", "1011001110001", NULL), 0, 0,
        (0, 43, 13, 0, 0, 0, 0), bytes([0xB3, 0x88])),
    # L = 13; power control 5; slot granting 0xA5; channel allocation: type 1, timeslots 1000, up/downlink 3,
    # CLCH 1, cell change 0, carrier 250, extended (band 4, offset 1, duplex 2, reverse 1), monitoring
    # pattern 0, frame-18 pattern 2; 12 SDU bits
    "resource, all three elements": (
        bits("00 0 0 00 0 001101 001", "0000 0000 0000 0000 0000 0001", "1 0101", "1 10100101",
             "1 01 1000 11 1 0 000011111010 1 0100 01 010 1 00 10", "111100001010", NULL), 0, 0,
        (0, 92, 12, 0, 15, 0x0115A505, 0x00FA098E), bytes([0xF0, 0xA0])),
    # fill flag set, L = 5, address type 2 (event label 0x2AA): SDU 1101, then the fill bits 1000000
    "resource with fill": (
        bits("00 1 0 00 0 000101 010", "1010101010", "0 0 0", "1101", "1000000", NULL), 0, 0,
        (0, 29, 4, 0, 0, 0, 0), bytes([0xD0])),
    # MAC-END, L = 3, slot granting 0x33, no channel allocation, 3 SDU bits
    "end with a grant": (
        bits("01 1 0 0 000011", "1 00110011", "0", "101", NULL), 0, 0,
        (0, 21, 3, 3, 2, 0x3300, 0), bytes([0xA0])),
    # MAC-FRAG in SCH/HD: the 120 bits behind its four
    "frag in SCH/HD": (
        bits("01 0 0", "0001001000110100010101100111100010011010", "1011110011011110111100000000111100011110",
             "0010110100111100010010110101101001101001"), 1, 0,
        (0, 4, 120, 2, 0, 0, 0), bytes.fromhex("123456789ABCDEF00F1E2D3C4B5A69")),
    # MAC-RESOURCE with L = 34 in SCH/F: 272 bits cut at 268, so the SDU is bits 43..267
    "L = 34 cut at bit 268": (
        bits("00 0 0 00 0 100010 001", "0000 0000 0000 0000 0000 0010", "0 0 0",
             "101010101010101010101010101010101010101010101", "010101010101010101010101010101010101010101010",
             "101010101010101010101010101010101010101010101", "010101010101010101010101010101010101010101010",
             "101010101010101010101010101010101010101010101"), 0, 0,
        (0, 43, 225, 0, 0, 0, 0), bytes([0xAA] * 28 + [0x80])),
    # the second PDU of a block: a whole MAC-RESOURCE (L = 4, event label) behind a MAC-END of two octets
    "second PDU of a block": (
        bits("01 1 0 0 000010", "0 0", "110", "00 0 0 00 0 000100 010", "0000000001", "0 0 0", "101", NULL), 0, 1,
        (0, 45, 3, 0, 0, 0, 0), bytes([0xA0])),
    # encrypted (ENC 2): nothing interpreted, bits 40..55 exported untouched
    "encrypted": (
        bits("00 1 0 10 0 000111 001", "0000 0000 0000 0000 0000 0011", "1111000011110000", NULL), 0, 0,
        (3, 40, 16, 0, 0, 0, 0), bytes([0xF0, 0xF0])),
}


@pytest.mark.parametrize("name", list(VECTORS))
def test_literal_vector(name):
    lead, kind, q, want, data = VECTORS[name]
    block = lead + [0] * (M.N1[kind] - len(lead))
    rec, sdu = first_record(block, kind, q)
    got = (rec[S.STATUS], rec[S.OFFSET], rec[S.NBITS], rec[S.ROLE], rec[S.ELEMS], rec[S.POWER_GRANT], rec[S.CHAN])
    assert got == want
    assert S.pack(sdu) == data


# ------------------------------------------------------------------------------ 2. round trip

def some_ca(rng, ext, mon):
    return dict(allocation_type=int(rng.integers(4)), timeslot_assigned=int(rng.integers(16)),
                updownlink_assigned=int(rng.integers(1, 4)), clch_permission=int(rng.integers(2)),
                cell_change=int(rng.integers(2)), carrier=int(rng.integers(4096)),
                extended=dict(band=int(rng.integers(16)), offset=int(rng.integers(4)), duplex_spacing=int(rng.integers(8)),
                              reverse_operation=int(rng.integers(2))) if ext else None,
                monitoring_pattern=mon, frame18_monitoring=int(rng.integers(4)))


def check_elements(rec, pc, sg, ca):
    assert rec[S.ELEMS] == (pc is not None) | (sg is not None) << 1 | (ca is not None) << 2 | \
        (ca is not None and ca["extended"] is not None) << 3
    pg = (pc or 0) | (sg or 0) << 8
    chan = 0
    if ca is not None:
        e = ca["extended"]
        if e is not None:
            pg |= (e["band"] << 6 | e["offset"] << 4 | e["duplex_spacing"] << 1 | e["reverse_operation"]) << 16
        chan = (ca["allocation_type"] << 8 | ca["timeslot_assigned"] << 4 | ca["updownlink_assigned"] << 2 |
                ca["clch_permission"] << 1 | ca["cell_change"] | ca["carrier"] << 16 | ca["monitoring_pattern"] << 28)
        if ca["monitoring_pattern"] == 0:
            chan |= ca["frame18_monitoring"] << 10
    assert rec[S.POWER_GRANT] == pg and rec[S.CHAN] == chan


@pytest.mark.parametrize("addr_type", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("fill", [0, 1])
def test_round_trip_resource(addr_type, fill):
    rng = np.random.default_rng(100 + 2 * addr_type + fill)
    has_ssi, auxn = M.ADDRESS[addr_type]
    seen = set()
    for combo in range(8):
        for length in list(range(2, 35)) + [62, 63]:
            pc = int(rng.integers(16)) if combo & 1 else None
            sg = int(rng.integers(256)) if combo & 2 else None
            ca = some_ca(rng, ext=bool(rng.integers(2)), mon=int(rng.integers(4))) if combo & 4 else None
            el = S.elements(M.RESOURCE, pc, sg, ca)
            head = 16 + 24 * has_ssi + auxn + len(el)
            nbits = min(8 * length, 268) if length <= 34 else 268
            room = nbits - head - fill
            if room < 0:
                continue
            n = room if not fill else 0 if rng.random() < 0.2 else int(rng.integers(0, room + 1))
            sdu = K.payload(rng, n)
            ssi, aux = int(rng.integers(1 << 24)), int(rng.integers(1 << auxn)) if auxn else 0
            pdu = S.resource_pdu(length, addr_type, sdu, head + n + fill if fill else nbits, ssi=ssi, aux=aux, fill=fill,
                                 elems=el)
            pdu += [0] * (nbits - len(pdu))   # the fill bits' zeros up to the PDU end
            block = pdu + M.null_pdu() + [0] * 268
            rec, got = first_record(block[:268], 0)
            assert rec[S.STATUS] == S.OK and got == sdu, (combo, length)
            assert rec[S.OFFSET] == head and rec[S.NBITS] == n
            assert rec[S.ROLE] == (S.FIRST if length == 63 else S.WHOLE)
            check_elements(rec, pc, sg, ca)
            seen.add((combo, n == 0))
    assert {c for c, _ in seen} == set(range(8)) and (not fill or any(z for _, z in seen))


def test_zero_bit_sdu_without_fill():
    """Event label (26 header bits), the three flags, an extended channel allocation of 35 bits: 64 = 8 L."""
    rng = np.random.default_rng(5)
    ca = some_ca(rng, ext=True, mon=2)
    pdu = S.resource_pdu(8, 2, [], 64, aux=0x155, elems=S.elements(M.RESOURCE, None, None, ca))
    rec, got = first_record((pdu + M.null_pdu() + [0] * 268)[:268], 0)
    assert (rec[S.STATUS], rec[S.OFFSET], rec[S.NBITS], got) == (S.OK, 64, 0, [])
    check_elements(rec, None, None, ca)


@pytest.mark.parametrize("fill", [0, 1])
def test_round_trip_end_and_frag(fill):
    rng = np.random.default_rng(7 + fill)
    for kind in (0, 1):
        n1 = M.N1[kind]
        for combo in range(4):
            for length in [L for L in list(range(2, 35)) + [62, 63] if L > 34 or 8 * L - n1 < 8]:
                sg = int(rng.integers(256)) if combo & 1 else None
                ca = some_ca(rng, ext=bool(rng.integers(2)), mon=int(rng.integers(4))) if combo & 2 else None
                el = S.elements(M.END, None, sg, ca)
                nbits = min(8 * length, n1) if length <= 34 else n1
                room = nbits - 11 - len(el) - fill
                if room < 0:
                    continue
                n = int(rng.integers(0, room + 1)) if fill else room
                sdu = K.payload(rng, n)
                pdu = S.end_pdu(length, sdu, 11 + len(el) + n + fill if fill else nbits, fill=fill, elems=el)
                pdu += [0] * (nbits - len(pdu))
                rec, got = first_record((pdu + M.null_pdu() + [0] * n1)[:n1], kind)
                assert rec[S.STATUS] == S.OK and got == sdu and rec[S.ROLE] == S.LAST
                assert rec[S.OFFSET] == 11 + len(el)
                check_elements(rec, None, sg, ca)
        for n in (0, 1, 57, n1 - 4 - fill):
            sdu = K.payload(rng, n)
            pdu = S.frag_pdu(sdu, 4 + n + fill if fill else n1, fill=fill) if fill or n == n1 - 4 else None
            if pdu is None:
                continue
            rec, got = first_record(pdu + [0] * (n1 - len(pdu)), kind)
            assert rec[S.STATUS] == S.OK and got == sdu and rec[S.ROLE] == S.MIDDLE and rec[S.OFFSET] == 4


def test_statuses():
    rng = np.random.default_rng(3)
    z = [0] * 268
    # malformed: the fill flag over nothing but zeros
    pdu = S.resource_pdu(6, 1, [], 43, fill=0) + [0] * 5
    pdu[2] = 1
    rec, sdu = first_record((pdu + M.null_pdu() + z)[:268], 0)
    assert (rec[S.STATUS], rec[S.NBITS], sdu) == (S.MALFORMED, 0, [])
    # malformed: slot granting runs past the PDU end (L = 6: 48 bits, 43 + 1 + 8 > 48)
    pdu = S.resource_pdu(6, 1, [1, 0, 1, 0, 1, 0], 48, elems=[0, 1])
    rec, _ = first_record((pdu + M.null_pdu() + z)[:268], 0)
    assert (rec[S.STATUS], rec[S.ELEMS]) == (S.MALFORMED, 0)
    # malformed: the channel allocation stops inside its carrier number; the ten bits before are kept
    el = S.elements(M.RESOURCE, 9, None, some_ca(rng, False, 1))
    pdu = S.resource_pdu(8, 1, [], 64, elems=el[:64 - 40])
    rec, _ = first_record((pdu + M.null_pdu() + z)[:268], 0)
    assert (rec[S.STATUS], rec[S.ELEMS], rec[S.POWER_GRANT]) == (S.MALFORMED, 5, 9)
    # unsupported: up/downlink assigned 0
    ca = some_ca(rng, False, 1)
    ca["updownlink_assigned"] = 0
    pdu = S.resource_pdu(10, 1, K.payload(rng, 80 - 43 - 10), 80, elems=S.elements(M.RESOURCE, None, None, ca))
    rec, sdu = first_record((pdu + M.null_pdu() + z)[:268], 0)
    assert (rec[S.STATUS], rec[S.ELEMS], rec[S.NBITS], sdu) == (S.UNSUPPORTED, 4, 0, [])
    assert rec[S.CHAN] & 0x3FF == (ca["allocation_type"] << 8 | ca["timeslot_assigned"] << 4 |
                                  ca["clch_permission"] << 1 | ca["cell_change"])
    # encrypted, every mode: the bits behind the address, fill bits and all
    for enc in (1, 2, 3):
        body = K.payload(rng, 30)
        pdu = S.resource_pdu(9, 1, body, 72, enc=enc, fill=1, elems=[])
        rec, sdu = first_record((pdu + M.null_pdu() + z)[:268], 0)
        assert (rec[S.STATUS], rec[S.OFFSET], rec[S.NBITS]) == (S.ENCRYPTED, 40, 32) and sdu == pdu[40:72]
    # none: a null PDU, a SYSINFO, a PDU the header walk found malformed (L = 1), a SYNC
    assert first_record((M.null_pdu() + z)[:268], 0)[0][S.STATUS] == S.NONE
    assert first_record((M.sysinfo({}) + z)[:268], 0)[0][S.STATUS] == S.NONE
    rec, _ = first_record((M.mac_end(rng, 1) + z)[:268], 0)
    assert (rec[S.STATUS], rec[S.ROLE]) == (S.NONE, S.LAST)
    assert first_record(M.sync(M.sync_for_slot(rng, 5)), 2)[0][S.STATUS] == S.NONE


def test_bytes_of_a_block_are_packed_in_pdu_order():
    rng = np.random.default_rng(4)
    a, b, c = K.payload(rng, 13), K.payload(rng, 0), K.payload(rng, 21)
    pdus = [S.resource_pdu(7, 1, a, 56), S.resource_pdu(4, 2, b, 32, fill=1), S.resource_pdu(8, 1, c, 64)]
    arrays = S.build_rows(rng, [[(0, 0, [pdus + [M.null_pdu()]])]])
    recs = S.part_a(arrays[2], arrays[3], arrays[4], arrays[5], arrays[6])[(0, 0)]
    assert [r[S.BYTE] for r, _ in recs] == [0, 2, 2, 5]
    assert [bits for _, bits in recs[:3]] == [a, b, c] and recs[3][0][S.STATUS] == S.NONE


# ------------------------------------------------------------------------------ 3. chains

@pytest.mark.parametrize("nfrag", range(2, 9))
def test_chain_comes_back_byte_for_byte(nfrag):
    rng = np.random.default_rng(nfrag)
    for step in (4, 8, 12):   # slots between fragments: 1..6 calls of 8 slots
        sdu = K.payload(rng, K.sdu_len(rng, nfrag))
        sc = K.Scenario("chain", K.chain_bursts(rng, sdu, nfrag, int(rng.integers(0, 2000)), step * K.SLOT))
        done, counts, fr = K.run_model(sc, rng)
        assert 1 <= len(counts) <= 13 and sum(counts) == 1
        f, data = done[0]
        assert data == S.pack(sdu) and f[S.D_NBITS] == len(sdu)
        assert (f[S.D_SSI], f[S.D_NFRAG], f[S.D_FED], f[S.D_SPAN], f[S.D_GAPS]) == \
            (0x123456, nfrag, nfrag, step * (nfrag - 1), (step // 4 - 1) * (nfrag - 1))
        assert (fr.dropped, fr.orphans) == (0, 0) and not any(c.active for c in fr.chains)


def test_chain_over_mixed_blocks():
    rng = np.random.default_rng(11)
    kinds = [1, 0, 1, 0]
    lo, hi = S.capacity(kinds)
    sdu = K.payload(rng, (lo + hi) // 2)
    pdus = S.fragment(sdu, kinds)
    filler = [M.null_pdu()]
    bursts = []
    for i, (k, pd) in enumerate(zip(kinds, pdus)):
        content = [pd] if i < 3 else [pd, M.null_pdu()]
        bursts.append(K.ndb(500 + 2040 * i, content) if k == 0 else K.ndp(500 + 2040 * i, content, filler))
    done, _, fr = K.run_model(K.Scenario("mixed", bursts), rng)
    assert [d for _, d in done] == [S.pack(sdu)] and fr.orphans == 0


# ------------------------------------------------------------------------------ 4. every rule at its edge

EDGE_NAMES = [sc.name for sc, _ in K.edge_cases(np.random.default_rng(0))]


@pytest.mark.parametrize("i", range(len(EDGE_NAMES)), ids=EDGE_NAMES)
def test_part_b_edge(i):
    sc, exp = K.edge_cases(np.random.default_rng(50))[i]
    done, counts, fr = K.run_model(sc, np.random.default_rng(51))
    assert [d for _, d in done] == [S.pack(b) for b in exp["done"]]
    assert [f[S.D_NBITS] for f, _ in done] == [len(b) for b in exp["done"]]
    assert (fr.dropped, fr.orphans) == (exp["dropped"], exp["orphans"])
    if "gaps" in exp:
        assert [f[S.D_GAPS] for f, _ in done] == exp["gaps"]
    if "counts" in exp:
        assert counts == exp["counts"]
    if "active" in exp:
        assert sum(c.active for c in fr.chains) == exp["active"]
    assert fr.bit0 == sc.bit0 + sc.ncalls * sc.chunk


def test_edge_details():
    cases = {sc.name: (sc, exp) for sc, exp in K.edge_cases(np.random.default_rng(50))}
    done, _, _ = K.run_model(cases["SCH/HD block 1 starts, block 2 ends"][0], np.random.default_rng(1))
    f = done[0][0]
    assert (f[S.D_BLOCK], f[S.D_PDU], f[S.D_SPAN], f[S.D_FED], f[S.D_NFRAG]) == (1, 0, 0, 1, 2)
    done, _, _ = K.run_model(cases["[END of A][start of B]"][0], np.random.default_rng(1))
    assert [(f[S.D_PDU], f[S.D_SSI]) for f, _ in done] == [(0, 0x123456), (0, 77)]
    done, _, _ = K.run_model(cases["GAPS over a CRC-bad burst"][0], np.random.default_rng(1))
    assert (done[0][0][S.D_SPAN], done[0][0][S.D_FED]) == (12, 3)


# ------------------------------------------------------------------------------ 5. groups

def test_groups_feed_each_burst_once():
    rng = np.random.default_rng(21)
    for sc, sdu in K.group_cases(rng):
        done, _, fr = K.run_model(sc, rng)
        assert [d for _, d in done] == [S.pack(sdu)], sc.name
        assert (fr.dropped, fr.orphans) == (0, 0)
        # without keep the second copy of a fragment feeds again: the chain is not the SDU any more
        sc.use_keep = False
        done2, _, fr2 = K.run_model(sc, rng)
        assert [d for _, d in done2] != [S.pack(sdu)] or fr2.orphans + fr2.dropped > 0, sc.name


def test_one_row_groups_equal_the_streaming_form():
    rng = np.random.default_rng(22)
    nfrag = 5
    sdu = K.payload(rng, K.sdu_len(rng, nfrag))
    sc = K.Scenario("stream", K.chain_bursts(rng, sdu, nfrag, 700))
    a, b = S.Frag(), S.Frag()
    for call in sc.calls(rng):
        arrays = call["arrays"]
        ra = S.run([a], 1, 0, 12345, 72, 4, call["nsym"], *arrays)   # streaming: the advance comes from nsym
        keep = np.ones((1, S.MAXB), np.int32)
        rb = S.run([b], 1, 0, 2 * (int(call["nsym"][0]) - 1), 72, 4, call["nsym"], *arrays, keep=keep)
        assert ra[2] == rb[2] and ra[1].tolist() == rb[1].tolist()
        assert a.to_array().tobytes() == b.to_array().tobytes()
    assert a.bit0 == sc.ncalls * sc.chunk


# ------------------------------------------------------------------------------ 6. no-GPU checks of the surfaces

def test_header_declares_the_entry_point_and_hip_carries_its_constants():
    from tetraear import _hip
    h = open(os.path.join(ROOT, "include", "tetra_hip.h")).read()
    assert re.search(r"\bint tetra_etsi_sdu\(tetra_ctx \*ctx", h)
    assert "#define TETRA_ABI_VERSION 2" in h

    def define(name):
        return int(re.search(rf"#define {name} (\d+)", h).group(1))

    assert (define("TETRA_SDU_ROW"), define("TETRA_SDU_MAXBYTES"), define("TETRA_FRAG_CHAINS")) == \
        (_hip.SDU_ROW, _hip.SDU_MAXBYTES, _hip.FRAG_CHAINS) == (S.SDU_ROW, S.SDU_MAXBYTES, S.FRAG_CHAINS)
    assert re.search(r"TETRA_SDU_FIELDS = (\d+)", h).group(1) == str(_hip.SDU_FIELDS) == str(S.SDU_FIELDS)
    assert re.search(r"TETRA_DONE_FIELDS = (\d+)", h).group(1) == str(_hip.DONE_FIELDS) == str(S.DONE_FIELDS)
    sdu_enum = re.search(r"enum \{\s*TETRA_SDU_STATUS = 0,([^}]*)\}", h).group(1)
    assert [s.strip() for s in sdu_enum.split(",")][:7] == [
        "TETRA_SDU_OFFSET", "TETRA_SDU_NBITS", "TETRA_SDU_BYTE", "TETRA_SDU_ROLE", "TETRA_SDU_ELEMS",
        "TETRA_SDU_POWER_GRANT", "TETRA_SDU_CHAN"]
    assert (_hip.SDU_STATUS, _hip.SDU_OFFSET, _hip.SDU_NBITS, _hip.SDU_BYTE, _hip.SDU_ROLE, _hip.SDU_ELEMS,
            _hip.SDU_POWER_GRANT, _hip.SDU_CHAN) == tuple(range(8))
    assert _hip.ETSI_FRAG == S.FRAG_DTYPE and _hip.ETSI_FRAG.itemsize == 16 + 4 * (48 + 512)
    assert (_hip.DONE_ROW, _hip.DONE_GAPS) == (S.D_ROW, S.D_GAPS)


def test_sdu_needs_mac():
    from tetraear.core.etsi import EtsiLowerMac
    with pytest.raises(ValueError):
        EtsiLowerMac(sdu=True)
    with pytest.raises(ValueError):
        EtsiLowerMac(mcc=1, mnc=2, colour_code=3, sdu=True, mac=False)
    assert EtsiLowerMac(mac=True, sdu=True).sdu is True and EtsiLowerMac().sdu is False


def test_messages_orders_whole_and_joined_sdus():
    from tetraear.core import etsi
    whole = {"kind": "RESOURCE", "ok": True, "sdu": b"\x12\x30", "sdu_bits": 12, "sdu_status": 0, "role": 0,
             "ssi": 5, "address_type": 1, "aux": None, "encryption_mode": 0}
    part = dict(whole, role=1, sdu=b"\xff", sdu_bits=8)
    empty = dict(whole, sdu=b"", sdu_bits=0)
    joined = {"ssi": 9, "address_type": 1, "aux": None, "enc": 0, "nbits": 20, "data": b"\x01\x02\x30", "fragments": 3,
              "span_slots": 8, "gaps": 0}
    frames = [{"position": 0, "blocks": [{"crc_ok": True, "pdus": [part, whole]}]},
              {"position": 510, "blocks": [{"crc_ok": True, "pdus": [empty]}], "sdus": [joined]},
              {"position": 1020, "blocks": [{"crc_ok": False}]}]
    got = etsi.messages(frames)
    assert [(m["data"], m["nbits"], m["ssi"], m["fragments"]) for m in got] == \
        [(b"\x12\x30", 12, 5, 1), (b"\x01\x02\x30", 20, 9, 3)]
    assert got[0]["gaps"] == 0 and got[0]["position"] == 0 and got[1]["position"] == 510


def test_etsi_frames_builds_mac_pdus_from_the_device_records():
    from tetraear.core.decoder import TetraDecoder

    class Recorder(TetraDecoder):
        def upper_mac(self, frame, burst, mac_pdu=None):
            self.calls.append(mac_pdu)
            return frame

    def pdu(kind, role, sdu, nbits, **kw):
        d = {"kind": kind, "offset": 0, "nbits": 268, "ok": True, "fill": 0, "header_bits": 40, "sdu": sdu,
             "sdu_bits": nbits, "sdu_status": 0, "role": role}
        d.update(kw)
        return d

    def frame(pos, pdus, **kw):
        f = {"position": pos, "burst": "NDB (n)", "burst_kind": 0, "timeslot": 0, "crc_ok": True,
             "blocks": [{"channel": "SCH/F", "crc_ok": True, "bits": np.zeros(268, np.uint8), "block": 0,
                         "npdu": len(pdus), "pdus": pdus}]}
        f.update(kw)
        return f

    raw = [frame(0, [pdu("RESOURCE", 0, b"\xAB\xC0", 12, length=7, encryption_mode=0, address_type=1, ssi=77, aux=None)]),
           frame(510, [pdu("RESOURCE", 1, b"\x11", 8, length=63, encryption_mode=0, address_type=1, ssi=88, aux=None)]),
           frame(2550, [pdu("END", 3, b"\x22", 8, length=5)],
                 sdus=[{"ssi": 88, "address_type": 1, "aux": None, "enc": 0, "nbits": 16, "data": b"\x11\x22",
                        "fragments": 2, "span_slots": 4, "gaps": 0}]),
           frame(3060, [pdu("RESOURCE", 0, b"\x99\x99", 16, length=8, encryption_mode=2, address_type=1, ssi=66, aux=None,
                            sdu_status=3)]),
           frame(3570, [pdu("NULL", 0, b"", 0, length=2, encryption_mode=0, address_type=0, ssi=None, aux=None,
                            sdu_status=1)])]
    d = Recorder(mode="etsi", mac=True, sdu=True)
    d.calls = []
    d._etsi_rx()   # the lower MAC object whose colour code the frames quote
    out = d._etsi_frames(raw)
    assert len(out) == 5 and len(d.calls) == 5
    whole, first, end, enc, null = d.calls
    assert (whole.pdu_type.name, whole.address, whole.length, whole.data, whole.reassembled_data, whole.encrypted) == \
        ("MAC_RESOURCE", 77, 7, b"\xAB\xC0", b"\xAB\xC0", False)
    assert (first.pdu_type.name, first.address, first.data, first.reassembled_data) == ("MAC_RESOURCE", 88, b"\x11", b"")
    assert (end.pdu_type.name, end.data, end.reassembled_data) == ("MAC_END", b"\x22", b"\x11\x22")
    assert (enc.encrypted, enc.data, enc.reassembled_data, enc.address) == (True, b"\x99\x99", b"", 66)
    assert null is None
    assert out[0]["mac_pdus"][0]["sdu_bits"] == 12 and out[0]["mac_pdus"][0]["role"] == 0
    assert out[2]["mac_pdus"][0]["role"] == 3 and out[2]["sdus"][0]["data"] == b"\x11\x22"
