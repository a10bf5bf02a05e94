"""The host side of tetra_etsi_llc without a GPU: the header's declaration and constants against
tetraear/_hip.py and the model, llc_keys on the model's records, and messages / link_messages on frames
written by hand.  All of these fail without the feature."""
import os
import re

import numpy as np
import pytest

import _etsi_mac_model as M
import _etsi_sdu_model as S
import _etsi_llc_model as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point_and_hip_carries_its_constants():
    from tetraear import _hip
    h = open(os.path.join(ROOT, "include", "tetra_hip.h")).read()
    assert re.search(r"\bint tetra_etsi_llc\(tetra_ctx \*ctx, size_t C, size_t G,", h)
    assert "#define TETRA_ABI_VERSION 2" in h
    assert re.search(r"TETRA_LLC_FIELDS = (\d+)", h).group(1) == str(_hip.LLC_FIELDS) == str(L.LLC_FIELDS)
    fields = re.search(r"enum \{\s*TETRA_LLC_STATUS = 0,([^}]*)\}", h).group(1)
    names = [s.strip() for s in fields.split(",")][:9]
    assert names == ["TETRA_LLC_TYPE", "TETRA_LLC_NR", "TETRA_LLC_NS", "TETRA_LLC_OFFSET", "TETRA_LLC_NBITS",
                     "TETRA_LLC_HEAD", "TETRA_LLC_FCS", "TETRA_LLC_FCS_RX", "TETRA_LLC_FCS_CALC"]
    assert [getattr(_hip, n[6:]) for n in names] == list(range(1, 10)) == \
        [L.TYPE, L.NR, L.NS, L.OFFSET, L.NBITS, L.HEAD, L.FCS, L.FCS_RX, L.FCS_CALC]
    assert re.search(r"enum \{ TETRA_LLC_OK = 0, TETRA_LLC_NONE, TETRA_LLC_MALFORMED, TETRA_LLC_ENCRYPTED, "
                     r"TETRA_LLC_UNSUPPORTED \}", h)
    assert (_hip.LLC_OK, _hip.LLC_NONE, _hip.LLC_MALFORMED, _hip.LLC_ENCRYPTED, _hip.LLC_UNSUPPORTED) == \
        (L.OK, L.NONE, L.MALFORMED, L.ENCRYPTED, L.UNSUPPORTED)
    assert re.search(r"enum \{ TETRA_FCS_NONE = 0, TETRA_FCS_GOOD, TETRA_FCS_BAD \}", h)
    assert (_hip.FCS_NONE, _hip.FCS_GOOD, _hip.FCS_BAD) == (L.FCS_NONE, L.FCS_GOOD, L.FCS_BAD)
    for said in ("0x04C11DB7", "0xFC891918", "0xC704DD7B", "NOT pinned"):
        assert said in h, said


def test_lower_mac_and_decoder_take_the_keyword():
    from tetraear.core.decoder import TetraDecoder
    from tetraear.core.etsi import EtsiLowerMac
    from tetraear.signal.wideband import WidebandStream
    for kw in (dict(llc=True), dict(mac=True, llc=True), dict(sdu=True, llc=True)):
        with pytest.raises(ValueError):
            EtsiLowerMac(**kw)
    assert EtsiLowerMac(mac=True, sdu=True, llc=True).llc is True and EtsiLowerMac(mac=True, sdu=True).llc is False
    assert TetraDecoder(auto_decrypt=False, mode="etsi", mac=True, sdu=True, llc=True).etsi_llc is True
    assert TetraDecoder(auto_decrypt=False, mode="etsi").etsi_llc is False
    with pytest.raises(ValueError):
        WidebandStream(np.zeros(800, np.uint32), mac=True, timebase=True, llc=True)


def keys_of(bits):
    from tetraear.core.etsi import llc_keys
    rec, tl = L.read_pdu(bits)
    return llc_keys(np.array(L.signed(rec), np.int32), np.frombuffer(S.pack(tl) + bytes(4), np.uint8))


def test_llc_keys_names_the_protocol_and_the_pdu():
    body = [1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1]
    sds = keys_of(L.llc_pdu(6, M.bits_of(2, 3) + M.bits_of(15, 5) + body))
    assert sds == {"status": 0, "type": 6, "name": "BL-UDATA+FCS", "nr": None, "ns": None, "fcs": True,
                   "fcs_rx": sds["fcs_calc"], "fcs_calc": sds["fcs_calc"], "tl_sdu": S.pack(M.bits_of(2, 3) + M.bits_of(15, 5) + body),
                   "tl_sdu_bits": 19, "protocol": 2, "protocol_name": "CMCE", "pdu_type": 15, "pdu_name": "D-SDS-DATA"}
    assert sds["fcs_calc"] == L.fcs(M.bits_of(6, 4) + M.bits_of(2, 3) + M.bits_of(15, 5) + body) > 0
    for t, name in enumerate(("D-ALERT", "D-CALL-PROCEEDING", "D-CONNECT", "D-CONNECT-ACKNOWLEDGE", "D-DISCONNECT",
                              "D-INFO", "D-RELEASE", "D-SETUP", "D-STATUS", "D-TX-CEASED", "D-TX-CONTINUE", "D-TX-GRANTED",
                              "D-TX-WAIT", "D-TX-INTERRUPT", "D-CALL-RESTORE", "D-SDS-DATA", "D-FACILITY")):
        assert keys_of(L.llc_pdu(2, M.bits_of(2, 3) + M.bits_of(t, 5)))["pdu_name"] == name
    assert keys_of(L.llc_pdu(2, M.bits_of(2, 3) + M.bits_of(17, 5)))["pdu_name"] is None
    # the type field: 5 bits for CMCE, 4 for MM and SNDCP, 3 for MLE; None when HEAD holds fewer
    for pd, name, width in ((1, "MM", 4), (2, "CMCE", 5), (4, "SNDCP", 4), (5, "MLE", 3)):
        for n in range(0, 6):
            k = keys_of(L.llc_pdu(1, M.bits_of(pd, 3) + [1] * n, ns=0))
            assert (k["protocol"], k["protocol_name"]) == (pd, name) and k["ns"] == 0 and k["fcs"] is None
            assert k["pdu_type"] == ((1 << width) - 1 if n >= width else None), (pd, n)
    for pd, name in ((0, "RESERVED"), (3, "RESERVED"), (6, "MANAGEMENT"), (7, "RESERVED")):
        k = keys_of(L.llc_pdu(0, M.bits_of(pd, 3) + [1] * 8, nr=1, ns=0))
        assert (k["protocol_name"], k["pdu_type"], k["nr"], k["ns"], k["name"]) == (name, None, 1, 0, "BL-ADATA")
    short = keys_of(L.llc_pdu(3, [1, 0], nr=1))
    assert (short["protocol"], short["protocol_name"], short["tl_sdu"], short["tl_sdu_bits"]) == (None, None, b"\x80", 2)
    assert keys_of(L.llc_pdu(6, [0, 1, 0, 1, 1], flip=6))["fcs"] is False


def test_llc_keys_of_records_that_are_not_ok():
    from tetraear.core.etsi import llc_keys
    row = np.arange(40, dtype=np.uint8)
    for rec, want in ((L.blank(L.NONE), (1, None, None)), (L.blank(L.MALFORMED), (2, None, None)),
                      (L.blank(L.ENCRYPTED, -1), (3, None, None)), (L.blank(L.UNSUPPORTED, 9), (4, 9, "AL-DATA/AL-FINAL"))):
        k = llc_keys(np.array(rec, np.int32), row)
        assert (k["status"], k["type"], k["name"]) == want
        assert (k["tl_sdu"], k["tl_sdu_bits"], k["fcs"], k["protocol"], k["pdu_name"], k["nr"], k["ns"]) == \
            (b"", 0, None, None, None, None, None)


def test_messages_pass_llc_through_and_link_messages_filter():
    from tetraear.core import etsi
    good = keys_of(L.llc_pdu(6, M.bits_of(2, 3) + M.bits_of(15, 5) + [1] * 16))
    bad = keys_of(L.llc_pdu(5, M.bits_of(1, 3) + [0] * 20, flip=9))
    bare = keys_of(L.llc_pdu(1, M.bits_of(5, 3) + [0] * 5))
    unsupported = keys_of(L.llc_pdu(9, [1] * 30))
    assert (good["fcs"], bad["fcs"], bare["fcs"], unsupported["status"]) == (True, False, None, 4)
    whole = {"kind": "RESOURCE", "ok": True, "sdu": b"\x12\x30", "sdu_bits": 12, "sdu_status": 0, "role": 0,
             "ssi": 5, "address_type": 1, "aux": None, "encryption_mode": 0}
    joined = {"ssi": 9, "address_type": 1, "aux": None, "enc": 0, "nbits": 20, "data": b"\x01\x02\x30", "fragments": 3,
              "span_slots": 8, "gaps": 0}
    frames = [{"position": 0, "blocks": [{"crc_ok": True, "pdus": [dict(whole, llc=good), dict(whole, ssi=6, llc=unsupported)]}]},
              {"position": 510, "blocks": [{"crc_ok": True, "pdus": [dict(whole, ssi=7, llc=bare)]}], "sdus": [dict(joined, llc=bad)]},
              {"position": 1020, "blocks": [{"crc_ok": True, "pdus": [dict(whole, ssi=8)]}]}]
    msgs = etsi.messages(frames)
    assert [m["ssi"] for m in msgs] == [5, 6, 7, 9, 8]
    assert [m.get("llc") for m in msgs] == [good, unsupported, bare, bad, None]
    link = etsi.link_messages(frames)
    assert [(m["ssi"], m["fcs"], m["protocol_name"], m["pdu_name"]) for m in link] == \
        [(5, True, "CMCE", "D-SDS-DATA"), (7, None, "MLE", None)]
    assert link[0]["tl_sdu"] == good["tl_sdu"] and link[0]["tl_sdu_bits"] == 24 and link[0]["llc"] == good
    assert link[0]["data"] == b"\x12\x30" and link[0]["position"] == 0
    both = etsi.link_messages(frames, drop_bad_fcs=False)
    assert [(m["ssi"], m["fcs"]) for m in both] == [(5, True), (7, None), (9, False)]
    assert both[2]["protocol_name"] == "MM" and both[2]["fragments"] == 3
