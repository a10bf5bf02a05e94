"""ETSI lower MAC on the GPU: burst sync, descrambling, deinterleaving, RCPC Viterbi, CRC-16.

The reference slices bursts at a fixed offset and checks a "simplified" CRC on raw bits
(/root/reference/tetraear/core/decoder.py:835-888, protocol.py:292-329); it never channel-decodes.
This module decodes what the north star asks for (EN 300 392-2 §8.2, §9.4.4):
  normal continuous downlink burst, training sequence n -> one SCH/F block (432 -> 268 bits)
                                    training sequence p -> two SCH/HD blocks (216 -> 124 bits)
  synchronisation burst -> BSCH (120 -> 60 bits, colour code 0) + SCH/HD on block 2
The work runs in tetra_lmac_etsi (k_lmac_etsi); this module packages results as frame dicts.
With ``mac=True`` tetra_etsi_mac (k_etsi_mac) follows it on the device: the TDMA timeslot / frame /
multiframe of every burst and the MAC PDU headers of every CRC-good block (EN 300 392-2 §21.4).
With ``link_quality=True`` tetra_etsi_link_quality (k_etsi_quality) follows it too: per burst the known
bits that came out wrong and the soft bits' strength, per CRC-good block the channel bits the decoder
corrected.
With ``traffic=True`` tetra_etsi_traffic (k_etsi_traffic) follows them: every burst gets a ``usage``, and
a slot the control decoders could not read comes out as descrambled type-4 soft bits, which
``codec_frame`` lays out as the speech codec's input frame.
With ``sdu=True`` (and ``mac=True``) tetra_etsi_sdu (k_sdu_walk, k_sdu_join) follows the MAC call: every PDU
gets its TM-SDU, and a carrier's fragments are joined across bursts and calls; ``messages`` lists the
finished TM-SDUs for an upper MAC.
With ``llc=True`` (and ``sdu=True``) tetra_etsi_llc (k_llc_whole, k_llc_done) follows: every TM-SDU is read as an
LLC PDU -- type, sequence bits, the frame check sequence, the TL-SDU byte-aligned -- and ``link_messages``
lists the messages whose LLC PDU reads well.
"""
import numpy as np

from tetraear import _hip

BLOCK_NAMES = {0: "SCH/F", 1: "SCH/HD", 2: "BSCH"}
BURST_NAMES = {0: "NDB (n)", 1: "NDB (p)", 2: "SB"}
KIND_N1 = {0: 268, 1: 124, 2: 60}
KIND_K = {0: 432, 1: 216, 2: 120}   # coded (type-5) bits


def scrambling_init(mcc, mnc, colour_code):
    """EN 300 392-2 §8.2.5.2: 30-bit extended colour code with two leading ones."""
    return ((((mcc & 0x3FF) << 20) | ((mnc & 0x3FFF) << 6) | (colour_code & 0x3F)) << 2) | 3


def cell_of(init):
    """(MCC, MNC, colour code) of a scrambling init."""
    ecc = int(init) >> 2
    return (ecc >> 20) & 0x3FF, (ecc >> 6) & 0x3FFF, ecc & 0x3F


PDU_NAMES = ("RESOURCE", "FRAG", "END", "SYSINFO", "ACCESS-DEFINE", "BROADCAST", "SUPPLEMENTARY", "SYNC", "NULL")
SYSINFO_OFFSET_HZ = {0: 0, 1: 6250, 2: -6250, 3: 12500}


def pdu_dict(rec):
    """One tetra_etsi_mac PDU record (16 int32, include/tetra_hip.h) as a dict with named fields."""
    r = [int(v) for v in rec]
    d = {"kind": PDU_NAMES[r[_hip.PDU_KIND]], "offset": r[_hip.PDU_OFFSET], "nbits": r[_hip.PDU_NBITS],
         "ok": r[_hip.PDU_STATUS] == 0}
    k = r[_hip.PDU_KIND]
    if k in (_hip.PDU_RESOURCE, _hip.PDU_FRAG, _hip.PDU_END, _hip.PDU_NULL):
        d.update(fill=r[_hip.PDU_FILL], header_bits=r[_hip.PDU_HDR_BITS])
        if k != _hip.PDU_FRAG:
            d.update(length=r[_hip.PDU_LENGTH], grant=r[_hip.PDU_FLAGS] & 1)
        if k in (_hip.PDU_RESOURCE, _hip.PDU_NULL):
            d.update(encryption_mode=r[_hip.PDU_ENC], address_type=r[_hip.PDU_ADDR_TYPE],
                     random_access=(r[_hip.PDU_FLAGS] >> 1) & 1,
                     ssi=None if r[_hip.PDU_SSI] < 0 else r[_hip.PDU_SSI],
                     aux=None if r[_hip.PDU_AUX] < 0 else r[_hip.PDU_AUX])
    elif k == _hip.PDU_SYNC:
        d.update(system_code=r[4], colour_code=r[5], tn=r[6], fn=r[7], mn=r[8], sharing_mode=r[9],
                 ts_reserved_frames=r[10], dtx=r[11] & 1, frame18_extension=(r[11] >> 1) & 1,
                 late_entry=(r[11] >> 2) & 1, mcc=r[12], mnc=r[13], neighbour_cell_broadcast=r[14],
                 cell_service_level=r[15])
    elif k == _hip.PDU_SYSINFO and d["ok"]:
        d.update(main_carrier=r[4], band=r[5], carrier_offset=r[6], duplex_spacing=r[7], reverse_operation=r[8],
                 num_cscch=r[9], ms_txpwr_max_cell=r[10], rxlev_access_min=r[11], access_parameter=r[12] & 15,
                 radio_downlink_timeout=(r[12] >> 4) & 15, optional_field_flag=(r[12] >> 8) & 3,
                 hyperframe_cck_flag=(r[13] >> 16) & 1, hyperframe_or_cck=r[13] & 0xFFFF, location_area=r[14],
                 subscriber_class=r[15] & 0xFFFF, bs_service_details=(r[15] >> 16) & 0xFFF,
                 downlink_hz=r[5] * 100e6 + r[4] * 25e3 + SYSINFO_OFFSET_HZ[r[6]])
    return d


UNKNOWN_CELL = scrambling_init(0, 0, 0)   # colour code 0: what a receiver descrambles with before the BSCH


def acquired_channels(nblock, blocks):
    """[C] bool: the channel's call decoded a CRC-good BSCH block (block kind 2), i.e. the cell
    k_cell_acquire keeps came from a SYNC PDU of this call."""
    nblock = np.asarray(nblock)
    blocks = np.asarray(blocks)
    live = np.arange(blocks.shape[1])[None, :] < nblock[:, None]
    return np.any(live & (blocks[:, :, 0] == 2) & (blocks[:, :, 1] != 0), axis=1)


def run_link_quality(c, soft, hard, origin, G, cells, nb, bursts, nk, blocks, t1):
    """tetra_etsi_link_quality on host arrays: (bq [C, MAXB, 4], kq [C, MAXJ, 4]), -1 where not written."""
    C, stride = hard.shape
    cells = np.ascontiguousarray(cells, np.uint32)
    bq = np.full((C, _hip.ETSI_MAXB, _hip.LQ_FIELDS), -1, np.int32)
    kq = np.full((C, _hip.ETSI_MAXJ, _hip.LQ_FIELDS), -1, np.int32)
    c.check(c.lib.tetra_etsi_link_quality(c.handle, _hip.ptr(soft), _hip.ptr(hard), C, stride, origin, G,
                                          _hip.ptr(cells), _hip.ptr(nb), _hip.ptr(bursts), _hip.ptr(nk),
                                          _hip.ptr(blocks), _hip.ptr(t1), _hip.ptr(bq), _hip.ptr(kq)),
            "tetra_etsi_link_quality")
    return bq, kq


def burst_quality(rec):
    """One burst record of tetra_etsi_link_quality as the keys a frame gains (None: not scored)."""
    r = [int(v) if v >= 0 else None for v in rec]
    return {"training_errors": r[_hip.BQ_TERR], "edge_errors": r[_hip.BQ_HERR], "soft_sum": r[_hip.BQ_WSUM],
            "saturated": r[_hip.BQ_NSAT]}


def block_quality(rec, kind):
    """One block record as the keys a block gains; channel_errors and ber are None for a CRC-bad block."""
    r = [int(v) for v in rec]
    scored = r[_hip.LQ_NERR] >= 0
    n = KIND_K[kind] - r[_hip.LQ_NZERO]
    return {"channel_errors": r[_hip.LQ_NERR] if scored else None, "channel_bits": KIND_K[kind],
            "soft_errors": r[_hip.LQ_WERR] if scored else None, "soft_sum": r[_hip.LQ_WSUM] if scored else None,
            "erased": r[_hip.LQ_NZERO] if scored else None,
            "ber": r[_hip.LQ_NERR] / n if scored and n > 0 else None}


def carrier_quality(frames):
    """Per-carrier totals of link_quality frames (one list of frames per carrier, as decode_batch or
    the wideband receiver returns them): [dict(blocks, blocks_ok, channel_errors, channel_bits, ber)],
    channel_bits counting the CRC-good blocks' bits that were not erased and ber = channel_errors /
    channel_bits (None when no block decoded).  A scanner ranks carriers by blocks_ok and ber."""
    out = []
    for fr in frames:
        blks = [b for f in fr for b in f["blocks"]]
        good = [b for b in blks if b.get("channel_errors") is not None]
        err = sum(b["channel_errors"] for b in good)
        bits = sum(b["channel_bits"] - b["erased"] for b in good)
        out.append({"blocks": len(blks), "blocks_ok": len(good), "channel_errors": err, "channel_bits": bits,
                    "ber": err / bits if bits else None})
    return out


USAGE_NAMES = {_hip.TCH_CONTROL: "control", _hip.TCH_FULL: "traffic", _hip.TCH_HALF: "stolen", _hip.TCH_LOST: "lost"}
CODEC_WORDS, CODEC_HEADER = 690, 0x6B21
# the 432 values of a codec frame lie at these words (word 0 the header, every other word 0)
CODEC_RUNS = ((1, 114), (116, 114), (231, 114), (346, 90))


def run_traffic(c, soft, origin, G, cells, nb, bursts, nk, blocks, slots=None, keep=None):
    """tetra_etsi_traffic on host arrays (soft [C, 2 stride]): (tq [C, MAXB, 4], -1 where not written,
    tch [C, MAXB, 432])."""
    C, stride = soft.shape[0], soft.shape[1] // 2
    cells = np.ascontiguousarray(cells, np.uint32)
    tq = np.full((C, _hip.ETSI_MAXB, _hip.TQ_FIELDS), -1, np.int32)
    tch = np.zeros((C, _hip.ETSI_MAXB, _hip.TCH_BITS), np.int8)
    c.check(c.lib.tetra_etsi_traffic(c.handle, _hip.ptr(soft), C, stride, origin, G, _hip.ptr(cells), _hip.ptr(nb),
                                     _hip.ptr(bursts), _hip.ptr(nk), _hip.ptr(blocks), _hip.ptr(slots), _hip.ptr(keep),
                                     _hip.ptr(tq), _hip.ptr(tch)), "tetra_etsi_traffic")
    return tq, tch


def traffic_keys(rec, tch, burst_kind, has_cell=True):
    """One burst record of tetra_etsi_traffic and its soft row as the keys a frame gains: ``usage``
    ("sync", "control", "traffic", "stolen" -- a half slot behind a stolen, decoded half -- "lost", or
    None: an invalid burst, a copy not kept, or a channel without a cell) and ``traffic`` (None, or
    dict(bits, soft int8 [bits], soft_sum, erased))."""
    r = [int(v) for v in rec]
    cls = r[_hip.TQ_CLASS]
    if not has_cell or cls < 0:
        return {"usage": None, "traffic": None}
    if cls == _hip.TCH_NONE:   # a synchronisation burst, or (with keep) the copy not chosen
        return {"usage": "sync" if burst_kind == 2 else None, "traffic": None}
    out = {"usage": USAGE_NAMES[cls], "traffic": None}
    if cls in (_hip.TCH_FULL, _hip.TCH_HALF):
        n = r[_hip.TQ_NBITS]
        out["traffic"] = {"bits": n, "soft": np.array(tch[:n], np.int8), "soft_sum": r[_hip.TQ_WSUM],
                          "erased": r[_hip.TQ_NZERO]}
    return out


def codec_frame(soft, polarity="reference", block_markers=False):
    """The speech codec's input frame of one full traffic slot: 1380 bytes, 690 little-endian int16
    words -- word 0 = 0x6B21, the 432 values at words 1..114, 116..229, 231..344 and 346..435, every
    other word 0 -- as the reference's writer lays them out (ui/modern.py:2369-2417; pinned word for
    word by tests/golden/g6_voice.npz).  ``soft``: the 432 type-4 soft values of a "traffic" frame
    (frame["traffic"]["soft"]; positive means bit 0).  ``polarity="reference"`` writes clamp(-soft, -127,
    127), bit 1 positive as the reference's writer has it; ``"inverted"`` writes clamp(soft, -127, 127).
    ``block_markers=True`` also writes 0x6B21 + i at words 115 i, i = 1..5.  The inverted polarity and
    the markers are written from memory of the ETSI codec's own file writer: no fixture pins them.
    216 values (a half slot) raise ValueError: the reference defines no half-slot frame."""
    s = np.asarray(soft)
    if s.ndim != 1 or len(s) != _hip.TCH_BITS:
        raise ValueError(f"codec_frame takes the {_hip.TCH_BITS} soft values of a full slot, not {s.shape}")
    if polarity not in ("reference", "inverted"):
        raise ValueError(f"polarity {polarity!r}: 'reference' or 'inverted'")
    v = s.astype(np.int32)
    v = np.clip(-v if polarity == "reference" else v, -127, 127)
    w = np.zeros(CODEC_WORDS, "<i2")
    w[0] = CODEC_HEADER
    at = 0
    for first, n in CODEC_RUNS:
        w[first:first + n] = v[at:at + n]
        at += n
    if block_markers:
        for i in range(1, 6):
            w[115 * i] = CODEC_HEADER + i
    return w.tobytes()


def traffic_streams(frames):
    """One carrier's frames -> {tn: [frame, ...]} of its "traffic" frames in time order (the order
    given); tn is None for frames without a timebase."""
    out = {}
    for f in frames:
        if f.get("usage") == "traffic":
            out.setdefault(f.get("tn"), []).append(f)
    return out


def slot_usage(frames):
    """One carrier's frames -> {tn: {usage: count}} (tn None without a timebase): the read-out a
    scanner ranks carriers by."""
    out = {}
    for f in frames:
        d = out.setdefault(f.get("tn"), {})
        d[f.get("usage")] = d.get(f.get("usage"), 0) + 1
    return out


SDU_MAXD = 16   # done records a row (or a wideband carrier's group) can return from one call


def run_sdu(c, nsym, G, row_bits, advance, nb, bursts, nk, blocks, t1, npdu, pdus, keep, frag, maxd=SDU_MAXD,
            gap_slots=_hip.TDMA_EXPIRE):
    """tetra_etsi_sdu on host arrays, frag [C / G] (_hip.ETSI_FRAG) updated in place: (sdu [C, MAXJ, MAXPDU,
    8], sdu_data [C, MAXJ, 40], ndone [C / G], done [C / G, maxd, 13], done_data [C / G, maxd, 512])."""
    C = len(nb)
    sdu = np.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.SDU_FIELDS), np.int32)
    sdu_data = np.zeros((C, _hip.ETSI_MAXJ, _hip.SDU_ROW), np.uint8)
    ndone = np.zeros(C // G, np.int32)
    done = np.zeros((C // G, maxd, _hip.DONE_FIELDS), np.int32)
    done_data = np.zeros((C // G, maxd, _hip.SDU_MAXBYTES), np.uint8)
    c.check(c.lib.tetra_etsi_sdu(c.handle, _hip.ptr(nsym), C, G, row_bits, advance, gap_slots, _hip.ptr(nb),
                                 _hip.ptr(bursts), _hip.ptr(nk), _hip.ptr(blocks), _hip.ptr(t1), _hip.ptr(npdu),
                                 _hip.ptr(pdus), _hip.ptr(keep), _hip.ptr(sdu), _hip.ptr(sdu_data), _hip.ptr(frag), maxd,
                                 _hip.ptr(ndone), _hip.ptr(done), _hip.ptr(done_data)), "tetra_etsi_sdu")
    return sdu, sdu_data, ndone, done, done_data


def sdu_keys(rec, row):
    """One tetra_etsi_sdu record and its block's sdu_data row as the keys a pdu dict gains: ``sdu`` (the
    TM-SDU's bytes, MSB first, zero-padded; empty unless sdu_status is 0 or 3), ``sdu_bits``,
    ``sdu_status`` (0 ok, 1 none, 2 malformed, 3 encrypted, 4 unsupported), ``role`` (0 whole, 1 first, 2
    middle, 3 last fragment) and, where present, ``power_control``, ``slot_granting`` and
    ``channel_allocation`` (a dict of the raw fields)."""
    r = [int(v) for v in rec]
    n, at = r[_hip.SDU_NBITS], r[_hip.SDU_BYTE]
    d = {"sdu": bytes(row[at:at + (n + 7) // 8]), "sdu_bits": n, "sdu_status": r[_hip.SDU_STATUS],
         "role": r[_hip.SDU_ROLE]}
    el, pg, ch = r[_hip.SDU_ELEMS], r[_hip.SDU_POWER_GRANT], r[_hip.SDU_CHAN]
    if el & 1:
        d["power_control"] = pg & 15
    if el & 2:
        d["slot_granting"] = (pg >> 8) & 255
    if el & 4:
        ca = {"allocation_type": (ch >> 8) & 3, "timeslot_assigned": (ch >> 4) & 15, "updownlink_assigned": (ch >> 2) & 3,
              "clch_permission": (ch >> 1) & 1, "cell_change": ch & 1}
        if r[_hip.SDU_STATUS] != _hip.SDU_UNSUPPORTED:   # the augmented form stops after these
            ca.update(carrier=(ch >> 16) & 0xFFF, monitoring_pattern=(ch >> 28) & 3)
            if ca["monitoring_pattern"] == 0:
                ca["frame18_monitoring"] = (ch >> 10) & 3
            if el & 8:
                x = (pg >> 16) & 0x3FF
                ca["extended"] = {"band": x >> 6, "offset": (x >> 4) & 3, "duplex_spacing": (x >> 1) & 7,
                                  "reverse_operation": x & 1}
        d["channel_allocation"] = ca
    return d


def done_dict(rec, data, block):
    """One done record of tetra_etsi_sdu and its bytes as an entry of a frame's ``sdus``; ``block`` (the
    block's index in its burst) and ``pdu`` say where the MAC-END sat."""
    r = [int(v) for v in rec]
    n = r[_hip.DONE_NBITS]
    return {"ssi": None if r[_hip.DONE_SSI] < 0 else r[_hip.DONE_SSI], "address_type": r[_hip.DONE_ADDR_TYPE],
            "aux": None if r[_hip.DONE_AUX] < 0 else r[_hip.DONE_AUX], "enc": r[_hip.DONE_ENC], "nbits": n,
            "data": bytes(data[:(n + 7) // 8]), "fragments": r[_hip.DONE_NFRAG], "span_slots": r[_hip.DONE_SPAN],
            "gaps": r[_hip.DONE_GAPS], "block": block, "pdu": r[_hip.DONE_PDU]}


def run_llc(c, G, nk, blocks, npdu, pdus, sd):
    """tetra_etsi_llc on host arrays behind run_sdu, sd = what run_sdu returned: (llc [C, MAXJ, MAXPDU, 10],
    tl [C, MAXJ, 40], llc_done [C / G, maxd, 10], tl_done [C / G, maxd, 512])."""
    sdu, sdu_data, ndone, done, done_data = sd
    C, maxd = len(nk), done.shape[1]
    llc = np.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.LLC_FIELDS), np.int32)
    tl = np.zeros((C, _hip.ETSI_MAXJ, _hip.SDU_ROW), np.uint8)
    llc_done = np.zeros((C // G, maxd, _hip.LLC_FIELDS), np.int32)
    tl_done = np.zeros((C // G, maxd, _hip.SDU_MAXBYTES), np.uint8)
    c.check(c.lib.tetra_etsi_llc(c.handle, C, G, _hip.ptr(nk), _hip.ptr(blocks), _hip.ptr(npdu), _hip.ptr(pdus),
                                 _hip.ptr(sdu), _hip.ptr(sdu_data), maxd, _hip.ptr(ndone), _hip.ptr(done),
                                 _hip.ptr(done_data), _hip.ptr(llc), _hip.ptr(tl), _hip.ptr(llc_done), _hip.ptr(tl_done)),
            "tetra_etsi_llc")
    return llc, tl, llc_done, tl_done


# Host-side names, transcribed from EN 300 392-2 (clause 21 the LLC PDU types, clause 18 the MLE protocol
# discriminator, clause 14 the CMCE downlink PDU types) and NOT pinned against a conformance vector: the
# device records carry the raw TYPE and HEAD, so a correction is a change to these tables.
LLC_NAMES = ("BL-ADATA", "BL-DATA", "BL-UDATA", "BL-ACK", "BL-ADATA+FCS", "BL-DATA+FCS", "BL-UDATA+FCS", "BL-ACK+FCS",
             "AL-SETUP", "AL-DATA/AL-FINAL", "AL-UDATA/AL-UFINAL", "AL-ACK/AL-RNR", "AL-RECONNECT", "SUPPLEMENTARY",
             "L2-SIGNALLING", "AL-DISC")
MLE_PROTOCOLS = {1: "MM", 2: "CMCE", 4: "SNDCP", 5: "MLE", 6: "MANAGEMENT"}   # the rest reserved
PDU_TYPE_BITS = {1: 4, 2: 5, 4: 4, 5: 3}   # the PDU type field behind the discriminator
CMCE_DOWNLINK = ("D-ALERT", "D-CALL-PROCEEDING", "D-CONNECT", "D-CONNECT-ACKNOWLEDGE", "D-DISCONNECT", "D-INFO",
                 "D-RELEASE", "D-SETUP", "D-STATUS", "D-TX-CEASED", "D-TX-CONTINUE", "D-TX-GRANTED", "D-TX-WAIT",
                 "D-TX-INTERRUPT", "D-CALL-RESTORE", "D-SDS-DATA", "D-FACILITY")


def llc_keys(rec, row):
    """One tetra_etsi_llc record and the bytes from its TL-SDU's first byte on (tl at the SDU's BYTE, or the
    tl_done row) as the dict a pdu, or an entry of ``sdus``, gains under ``llc``: ``status`` (0 ok, 1 none,
    2 malformed, 3 encrypted, 4 unsupported), ``type`` and ``name`` (None where not read), ``nr`` / ``ns``
    (None where the type has none), ``fcs`` (None: the type has none; True good, False bad), ``fcs_rx``,
    ``fcs_calc``, ``tl_sdu`` (bytes, MSB first, zero-padded), ``tl_sdu_bits``, ``protocol`` (the MLE protocol
    discriminator, None with fewer than 3 bits) and ``protocol_name``, ``pdu_type`` (None when the TL-SDU's
    first eight bits hold fewer bits than the protocol's type field, or the protocol has no table) and
    ``pdu_name`` (the CMCE downlink names; else None)."""
    r = [int(v) for v in rec]
    status, t, head = r[_hip.LLC_STATUS], r[_hip.LLC_TYPE], r[_hip.LLC_HEAD]
    read = status in (_hip.LLC_OK, _hip.LLC_UNSUPPORTED)
    n = r[_hip.LLC_NBITS] if status == _hip.LLC_OK else 0
    d = {"status": status, "type": t if read else None, "name": LLC_NAMES[t] if read else None,
         "nr": None if r[_hip.LLC_NR] < 0 else r[_hip.LLC_NR], "ns": None if r[_hip.LLC_NS] < 0 else r[_hip.LLC_NS],
         "fcs": {_hip.FCS_GOOD: True, _hip.FCS_BAD: False}.get(r[_hip.LLC_FCS]),
         "fcs_rx": r[_hip.LLC_FCS_RX] & 0xFFFFFFFF, "fcs_calc": r[_hip.LLC_FCS_CALC] & 0xFFFFFFFF,
         "tl_sdu": bytes(row[:(n + 7) // 8]), "tl_sdu_bits": n, "protocol": None, "protocol_name": None,
         "pdu_type": None, "pdu_name": None}
    if status == _hip.LLC_OK and head >= 0:
        pd = head >> 5
        d["protocol"], d["protocol_name"] = pd, MLE_PROTOCOLS.get(pd, "RESERVED")
        w = PDU_TYPE_BITS.get(pd)
        if w is not None and n >= 3 + w:
            d["pdu_type"] = (head >> (5 - w)) & ((1 << w) - 1)
            if pd == 2 and d["pdu_type"] < len(CMCE_DOWNLINK):
                d["pdu_name"] = CMCE_DOWNLINK[d["pdu_type"]]
    return d


def messages(frames):
    """One carrier's frames (sdu=True) -> its finished TM-SDUs in time order, what a caller hands to an
    upper MAC: of every frame the whole ones -- a MAC-RESOURCE that is no fragment, with a TM-SDU of at
    least one bit, sdu_status 0 or 3 (encrypted: ``enc`` != 0, the bits untouched) -- in block and PDU order,
    then the ones a MAC-END of the frame completed (``sdus``).  Each is a dict(ssi, address_type, aux, enc,
    nbits, data, fragments, span_slots, gaps, position[, tn, fn, mn]); a whole one has fragments 1, gaps 0.
    With llc=True each carries its ``llc`` dict (llc_keys) as well."""
    out = []
    for f in frames:
        where = {k: f[k] for k in ("position", "tn", "fn", "mn") if k in f}
        for b in f["blocks"]:
            for p in b.get("pdus", ()) if b["crc_ok"] else ():
                if p["kind"] == "RESOURCE" and p.get("role") == _hip.ROLE_WHOLE and p["sdu_bits"] > 0 and \
                        p["sdu_status"] in (_hip.SDU_OK, _hip.SDU_ENCRYPTED):
                    out.append(dict(ssi=p["ssi"], address_type=p["address_type"], aux=p["aux"],
                                    enc=p["encryption_mode"], nbits=p["sdu_bits"], data=p["sdu"], fragments=1,
                                    span_slots=0, gaps=0, **where))
                    if "llc" in p:
                        out[-1]["llc"] = p["llc"]
        for m in f.get("sdus", ()):
            out.append(dict(m, **where))
    return out


def link_messages(frames, drop_bad_fcs=True):
    """One carrier's frames (llc=True) -> the messages of ``messages(frames)`` whose LLC PDU reads ok (status
    0), each with ``tl_sdu``, ``tl_sdu_bits``, ``protocol_name``, ``pdu_name`` and ``fcs`` beside its ``llc``
    dict: what an MLE router consumes.  A message whose FCS is bad (``fcs`` False) is left out unless
    drop_bad_fcs is False; one without an FCS (``fcs`` None) is kept: nothing vouches for it."""
    out = []
    for m in messages(frames):
        ll = m.get("llc")
        if ll is None or ll["status"] != _hip.LLC_OK or (drop_bad_fcs and ll["fcs"] is False):
            continue
        out.append(dict(m, **{k: ll[k] for k in ("tl_sdu", "tl_sdu_bits", "protocol_name", "pdu_name", "fcs")}))
    return out


class EtsiLowerMac:
    """Lower MAC of the ETSI chain.  With a cell (mcc, mnc, colour_code) every channel is
    descrambled with it.  Without one the receiver acquires the cell itself: each chunk's BSCH
    blocks are decoded first with colour code 0, and the SYNC PDU of the last CRC-good one gives the
    channel's MCC / MNC / colour code (tetra_lmac_etsi_acquire).  The acquired cell persists across
    calls per channel -- the state the reference parser keeps from a SYSINFO broadcast
    (/root/reference/tetraear/core/protocol.py:479-485) -- and is exposed as ``cells`` /
    ``mcc`` / ``mnc`` / ``colour_code``.

    ``mac=True``: tetra_etsi_mac runs after the lower MAC.  Every frame gains ``tn`` / ``fn`` / ``mn``
    (None while the channel has no timebase) and ``slot_flags``, every block ``pdus`` (dicts of the
    first TETRA_ETSI_MAXPDU MAC PDU headers, pdu_dict) and ``npdu``.  The timebase is carried from
    chunk to chunk by decode_stream / decode (reset_stream() drops it) and is fresh for every
    decode_batch.  Without it the frames are unchanged.

    ``link_quality=True``: tetra_etsi_link_quality runs after the lower MAC on the rows it read.  Every
    frame gains ``training_errors`` / ``edge_errors`` (training-sequence and head / tail bits that came
    out wrong), ``soft_sum`` (sum of |soft| over the burst's 510 bits) and ``saturated`` (soft bits at
    full scale); every block ``channel_errors`` (coded bits the decoder corrected, None when the CRC
    failed), ``channel_bits``, ``soft_errors`` (sum of |soft| over the corrected bits), ``soft_sum``,
    ``erased`` (soft bits at 0) and ``ber`` = channel_errors / (channel_bits - erased).  decode_stream
    then alternates two sets of rows, so the rows a call read are intact for the quality pass.
    Everything else in the frames is unchanged.

    ``vote=True`` (acquisition mode only): the cell is chosen by the vote of tetra_lmac_etsi_vote_groups /
    _stream_vote instead of by the last CRC-good BSCH -- every CRC-good BSCH weighs in with the
    correlation of its soft bits with its re-encoded codeword, and the cell kept so far defends with
    ``cell_score`` [C] (int32, kept next to ``cell_state``; reset_stream() clears it), bounded by
    ``vote_cap``.  One false CRC pass or a neighbour cell's burst then no longer replaces an established
    cell.  With one cell per channel the frames are those of ``vote=False``.

    ``timebase_vote=True`` (with ``mac=True``): the timebase comes from tetra_etsi_mac_vote_groups (G = 1,
    row_bits = 0, advance = 2 max(nsym - 1, 0)) instead of tetra_etsi_mac: a SYNC moves the channel's slot
    grid only if its soft-bit weight outvotes the score the grid has gathered, kept in ``tdma_score`` [C]
    beside the timebases (reset_stream() clears both) and bounded by ``tdma_cap``; ``slot_flags`` bit 2
    marks a burst whose own SYNC was outvoted.  tetra_etsi_link_quality runs first for the weights (the
    streaming origin for streaming rows; its keys reach the frames only with ``link_quality=True``).  The
    one difference from tetra_etsi_mac on a stream without contradictions: a burst behind the anchor does
    not drop the lock (tetra_etsi_mac_groups' rule 1).

    ``traffic=True``: tetra_etsi_traffic runs after the lower MAC (and after the MAC call when
    ``mac=True``, whose slots it is given: frame 18 never carries traffic) on the rows it read.  Every
    frame gains ``usage`` and ``traffic`` (traffic_keys): a normal burst whose blocks the control decoders
    could not read comes out as its 432 (216 behind a stolen half) descrambled type-4 soft bits, positive
    meaning bit 0 -- what the speech codec's channel decoder consumes (codec_frame).  Without the AACH
    such a slot is a candidate: a control burst lost to noise looks the same, and ``soft_sum`` and the
    timebase are what a caller gates on.  In acquisition mode a channel without a cell yet reports
    ``usage`` None.  decode_stream alternates two sets of rows as with ``link_quality=True``.  Everything
    else in the frames is unchanged.

    ``sdu=True`` (with ``mac=True``): tetra_etsi_sdu runs after the MAC call.  Every pdu dict gains ``sdu``,
    ``sdu_bits``, ``sdu_status``, ``role`` and the optional elements it carries (sdu_keys); a frame whose
    burst held a MAC-END that completed a chain of fragments gains ``sdus``, a list of dict(ssi,
    address_type, aux, enc, nbits, data, fragments, span_slots, gaps).  The fragment state is carried like
    the timebase: per channel by decode_stream / decode, cleared by reset_stream(), fresh for every
    decode_batch; ``frag_stats`` counts the chains dropped unfinished and the fragments that found no
    chain.  ``messages(frames)`` lists a carrier's finished TM-SDUs.  Everything else is unchanged.

    ``llc=True`` (with ``mac=True, sdu=True``): tetra_etsi_llc runs after the SDU call.  Every pdu dict and
    every entry of ``sdus`` gains ``llc`` (llc_keys): the LLC type, sequence bits, the FCS verdict and the
    TL-SDU; ``link_messages(frames)`` lists the messages that read well.  Everything else is unchanged."""

    def __init__(self, mcc=None, mnc=None, colour_code=None, mac=False, link_quality=False, vote=False,
                 vote_cap=_hip.TETRA_ETSI_VOTE_CAP_DEFAULT, timebase_vote=False,
                 tdma_cap=_hip.TETRA_TDMA_VOTE_CAP_DEFAULT, traffic=False, sdu=False, llc=False):
        self.mac = bool(mac)
        self.sdu = bool(sdu)
        if self.sdu and not self.mac:
            raise ValueError("sdu=True reads the PDU records of mac=True")
        self.llc = bool(llc)
        if self.llc and not self.sdu:
            raise ValueError("llc=True reads the TM-SDUs of mac=True, sdu=True")
        self.traffic = bool(traffic)
        self.link_quality = bool(link_quality)
        self.timebase_vote, self.tdma_cap = bool(timebase_vote), int(tdma_cap)
        if self.timebase_vote and not self.mac:
            raise ValueError("timebase_vote=True chooses the timebase of mac=True")
        if self.timebase_vote and self.tdma_cap <= 0:
            raise ValueError(f"tdma_cap ({tdma_cap}) must be positive")
        self.tdma_votes = None   # [C, 4] int32: the last call's ballots (cast, agreed, outvoted, won)
        self.acquire = mcc is None and mnc is None and colour_code is None
        self.vote, self.vote_cap = bool(vote), int(vote_cap)
        if self.vote and not self.acquire:
            raise ValueError("vote=True chooses among acquired cells: it takes no mcc / mnc / colour_code")
        if self.vote and self.vote_cap <= 0:
            raise ValueError(f"vote_cap ({vote_cap}) must be positive")
        self.cell_score = None   # [C] int32: the score each channel's cell has gathered (vote=True)
        self.cell = None if self.acquire else scrambling_init(mcc or 0, mnc or 0, colour_code or 0)
        self.cell_state = None   # [C] scrambling inits of the acquired cells (acquisition mode)
        # [C] bool: a CRC-good BSCH has been decoded on the channel.  Kept apart from cell_state,
        # because an all-zero cell (MCC = MNC = CC = 0) has the init of UNKNOWN_CELL.
        self.acquired = None
        self.reset_stream()

    def reset_stream(self):
        """decode_stream / decode start a new capture: no carried dibits."""
        self._rows = None   # (soft rows [C, 2 stride], hard rows [C, stride], lead [C]): the carried tails
        self._alt = None    # link_quality: the other (soft rows, hard rows), which the next tails go to
        self._tdma = None   # [C] tetra_etsi_tdma: the carried timebases (mac=True)
        self.tdma_score = None   # [C] int32: the score each timebase has gathered (timebase_vote=True)
        self.cell_score = None   # vote=True: the cells start without incumbency (cell_state is kept)
        self._frag = None   # [C] tetra_etsi_frag: the carried fragment chains (sdu=True)
        self._frag_last = None   # the state the last call left (decode_batch's is not carried)
        self._lost = None   # [C] completions beyond SDU_MAXD a call, which no frame carries

    @property
    def frag_stats(self):
        """sdu=True: dict(dropped [C], orphans [C]) -- chains freed unfinished (expired, superseded,
        evicted, overflowed) and middle / last fragments that found no chain -- since the stream began
        (decode_batch: of that call); ``lost`` [C] counts the messages completed beyond the SDU_MAXD a call can
        return per channel, which reach no frame; None before the first call."""
        if self._frag_last is None:
            return None
        return {"dropped": self._frag_last["dropped"].copy(), "orphans": self._frag_last["orphans"].copy(),
                "lost": self._lost.copy()}

    def _run_sdu(self, c, nsym, nb, bursts, nk, blocks, t1, mac, frag):
        """tetra_etsi_sdu in its streaming form on the MAC call's records (sdu=True; else None)."""
        if not self.sdu:
            return None
        if frag is None or self._lost is None or len(self._lost) != len(nb):
            self._lost = np.zeros(len(nb), np.int64)
        if frag is None:
            frag = np.zeros(len(nb), _hip.ETSI_FRAG)
        self._frag_last = frag
        sd = run_sdu(c, nsym, 1, 0, 0, nb, bursts, nk, blocks, t1, mac[1], mac[2], None, frag)
        self._lost += np.maximum(sd[2] - SDU_MAXD, 0)
        if self.llc:   # the LLC records ride behind the SDU call's five arrays
            sd += run_llc(c, 1, nk, blocks, mac[1], mac[2], sd)
        return sd

    @property
    def cells(self):
        """Per channel (MCC, MNC, colour code) acquired so far, None where no BSCH decoded yet."""
        if self.cell_state is None:
            return []
        return [cell_of(v) if a else None for v, a in zip(self.cell_state, self.acquired)]

    @property
    def mcc(self):
        c = self.cells[0] if self.cells else None
        return None if c is None else c[0]

    @property
    def mnc(self):
        c = self.cells[0] if self.cells else None
        return None if c is None else c[1]

    @property
    def colour_code(self):
        c = self.cells[0] if self.cells else None
        return None if c is None else c[2]

    def decode_batch(self, soft, hard, nsym, cells=None):
        """soft [C, 2*smax] int8, hard [C, smax] uint8, nsym [C] -> per channel a list of frames.
        ``cells`` ([C] scrambling inits) overrides the receiver's cell for this call."""
        soft = np.ascontiguousarray(soft, np.int8)
        hard = np.ascontiguousarray(hard, np.uint8)
        nsym = np.ascontiguousarray(nsym, np.int32)
        C, smax = hard.shape
        nb = np.zeros(C, np.int32)
        bursts = np.zeros((C, _hip.ETSI_MAXB, 2), np.int32)
        nk = np.zeros(C, np.int32)
        blocks = np.zeros((C, _hip.ETSI_MAXJ, 4), np.int32)
        t1 = np.zeros((C, _hip.ETSI_MAXJ, 268), np.uint8)
        c = _hip.ctx()
        if self.acquire and cells is None:
            if self.cell_state is None or len(self.cell_state) != C:
                self.cell_state = np.full(C, UNKNOWN_CELL, np.uint32)
                self.acquired = np.zeros(C, bool)
            if self.acquired is None or len(self.acquired) != C:   # cell_state handed in from outside
                self.acquired = np.zeros(C, bool)
            if self.vote:
                ngood, agree = np.zeros(C, np.int32), np.zeros(C, np.int32)
                c.check(c.lib.tetra_lmac_etsi_vote_groups(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C,
                                                          smax, 1, self.vote_cap, _hip.ptr(self.cell_state),
                                                          _hip.ptr(self._score(C)), _hip.ptr(ngood), _hip.ptr(agree),
                                                          _hip.ptr(nb), _hip.ptr(bursts), _hip.ptr(nk), _hip.ptr(blocks),
                                                          _hip.ptr(t1)), "tetra_lmac_etsi_vote_groups")
            else:
                c.check(c.lib.tetra_lmac_etsi_acquire(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, smax,
                                                      _hip.ptr(self.cell_state), _hip.ptr(nb), _hip.ptr(bursts),
                                                      _hip.ptr(nk), _hip.ptr(blocks), _hip.ptr(t1)),
                        "tetra_lmac_etsi_acquire")
            self.acquired |= acquired_channels(nk, blocks)
            used = self.cell_state
        else:
            cells = np.full(C, self.cell if self.cell is not None else UNKNOWN_CELL, np.uint32) if cells is None \
                else np.ascontiguousarray(cells, np.uint32)
            c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(cells), C), "tetra_etsi_set_cells")
            c.check(c.lib.tetra_lmac_etsi(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, smax,
                                          _hip.ptr(nb), _hip.ptr(bursts), _hip.ptr(nk), _hip.ptr(blocks), _hip.ptr(t1)),
                    "tetra_lmac_etsi")
            used = cells
        lq = self._run_quality(c, soft, hard, 0, used, nb, bursts, nk, blocks, t1)
        mac = self._run_mac(c, C, nsym, nb, bursts, nk, blocks, t1, None, lq)
        tr = self._run_traffic(c, soft, 0, used, nb, bursts, nk, blocks, mac, used is self.cell_state)
        sd = self._run_sdu(c, nsym, nb, bursts, nk, blocks, t1, mac, None)
        return self._frames(C, nb, bursts, nk, blocks, t1, mac, lq if self.link_quality else None, tr, sd)

    def _score(self, C):
        """cell_score for C channels (vote=True): zeros when new or of another length."""
        if self.cell_score is None or len(self.cell_score) != C:
            self.cell_score = np.zeros(C, np.int32)
        return self.cell_score

    def _run_quality(self, c, soft, hard, origin, cells, nb, bursts, nk, blocks, t1):
        """tetra_etsi_link_quality on the rows the lower-MAC call read (link_quality=True or
        timebase_vote=True; else None): (bq, kq).  cells [C]: the inits the rows were descrambled with."""
        if not (self.link_quality or self.timebase_vote):
            return None
        return run_link_quality(c, soft, hard, origin, 1, cells, nb, bursts, nk, blocks, t1)

    def _run_traffic(self, c, soft, origin, cells, nb, bursts, nk, blocks, mac, acquiring):
        """tetra_etsi_traffic on the rows the lower-MAC call read (traffic=True; else None): (tq, tch,
        has_cell [C]).  mac: None or the MAC call's (slots, npdu, pdus); acquiring: the cells are the
        acquisition state, so a channel has one only once a BSCH decoded."""
        if not self.traffic:
            return None
        tq, tch = run_traffic(c, soft, origin, 1, cells, nb, bursts, nk, blocks, None if mac is None else mac[0])
        return tq, tch, self.acquired.copy() if acquiring else np.ones(len(nb), bool)

    def _run_mac(self, c, C, nsym, nb, bursts, nk, blocks, t1, tdma, lq=None, score=None):
        """tetra_etsi_mac on the lower MAC's outputs (mac=True; else None): (slots, npdu, pdus).
        tdma None: a new stream per channel.  timebase_vote=True: tetra_etsi_mac_vote_groups with the
        call's link-quality records lq and the scores score [C] (None: zeros) instead."""
        if not self.mac:
            return None
        if tdma is None:
            tdma = np.zeros(C, _hip.ETSI_TDMA)
        slots = np.zeros((C, _hip.ETSI_MAXB, _hip.SLOT_FIELDS), np.int32)
        npdu = np.zeros((C, _hip.ETSI_MAXJ), np.int32)
        pdus = np.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.PDU_FIELDS), np.int32)
        if self.timebase_vote:
            score = np.zeros(C, np.int32) if score is None else score
            self.tdma_votes = np.zeros((C, _hip.TV_FIELDS), np.int32)
            keep = np.zeros((C, _hip.ETSI_MAXB), np.int32)   # one row a group: a row's bursts are a slot apart
            for n in np.unique(nsym):   # advance is one value a call: the channels of one chunk length together
                idx = np.flatnonzero(nsym == n)
                every = len(idx) == C
                a = [v if every else np.ascontiguousarray(v[idx])
                     for v in (nsym, nb, bursts, nk, blocks, t1, lq[0], lq[1], tdma, score, keep, slots, npdu, pdus,
                               self.tdma_votes)]
                c.check(c.lib.tetra_etsi_mac_vote_groups(c.handle, _hip.ptr(a[0]), len(idx), 1, 0, 32,
                                                         2 * max(int(n) - 1, 0), self.tdma_cap,
                                                         *[_hip.ptr(v) for v in a[1:]]), "tetra_etsi_mac_vote_groups")
                if not every:
                    for dst, src in zip((tdma, score, slots, npdu, pdus, self.tdma_votes),
                                        (a[8], a[9], a[11], a[12], a[13], a[14])):
                        dst[idx] = src
            return slots, npdu, pdus
        c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(nsym), C, _hip.ptr(nb), _hip.ptr(bursts), _hip.ptr(nk),
                                     _hip.ptr(blocks), _hip.ptr(t1), _hip.ptr(tdma), _hip.ptr(slots), _hip.ptr(npdu),
                                     _hip.ptr(pdus)), "tetra_etsi_mac")
        return slots, npdu, pdus

    def _run_stream(self, c, C, nb, bursts, nk, blocks, t1, cells, stream):
        """tetra_lmac_etsi_stream over stream = (soft rows, hard rows, nsym, stride, lead[, next soft
        rows, next hard rows]), with the receiver's cell handling (acquisition state or configured
        cells) as decode_batch's.  Returns the inits the rows were descrambled with."""
        if self.acquire and cells is None:
            if self.cell_state is None or len(self.cell_state) != C:
                self.cell_state = np.full(C, UNKNOWN_CELL, np.uint32)
                self.acquired = np.zeros(C, bool)
            if self.acquired is None or len(self.acquired) != C:   # cell_state handed in from outside
                self.acquired = np.zeros(C, bool)
            ci = _hip.ptr(self.cell_state)
        else:
            cells = np.full(C, self.cell if self.cell is not None else UNKNOWN_CELL, np.uint32) if cells is None \
                else np.ascontiguousarray(cells, np.uint32)
            c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(cells), C), "tetra_etsi_set_cells")
            ci = None
        srow, hrow, ns, stride, lead = stream[:5]
        nsrow, nhrow = stream[5:] if len(stream) > 5 else (srow, hrow)
        if self.vote and ci is not None:
            c.check(c.lib.tetra_lmac_etsi_stream_vote(c.handle, _hip.ptr(srow), _hip.ptr(hrow), _hip.ptr(ns), C, stride,
                                                      _hip.ptr(lead), _hip.ptr(nsrow), _hip.ptr(nhrow), self.vote_cap,
                                                      ci, _hip.ptr(self._score(C)), None, _hip.ptr(nb),
                                                      _hip.ptr(bursts), _hip.ptr(nk), _hip.ptr(blocks), _hip.ptr(t1)),
                    "tetra_lmac_etsi_stream_vote")
        else:
            c.check(c.lib.tetra_lmac_etsi_stream(c.handle, _hip.ptr(srow), _hip.ptr(hrow), _hip.ptr(ns), C, stride,
                                                 _hip.ptr(lead), _hip.ptr(nsrow), _hip.ptr(nhrow), ci, _hip.ptr(nb),
                                                 _hip.ptr(bursts), _hip.ptr(nk), _hip.ptr(blocks), _hip.ptr(t1)),
                    "tetra_lmac_etsi_stream")
        if ci is not None:
            self.acquired |= acquired_channels(nk, blocks)
            return self.cell_state
        return cells

    def decode_stream(self, soft, hard, nsym, cells=None):
        """decode_batch for consecutive chunks of C continuous streams (EtsiStream.demod rows):
        each channel's dibits the previous call left unconsumed -- from the first bit its burst scan
        did not examine -- go in front of this chunk's, and the scan resumes there
        (tetra_lmac_etsi_stream), so a burst across the seam is decoded whole.  Positions are
        relative to this chunk's first dibit (negative: the burst began in the carried tail)."""
        soft = np.ascontiguousarray(soft, np.int8)
        hard = np.ascontiguousarray(hard, np.uint8)
        nsym = np.ascontiguousarray(nsym, np.int32)
        C, smax = hard.shape
        R = _hip.ETSI_RESERVE
        if self._rows is None or self._rows[1].shape[0] != C or self._rows[1].shape[1] < R + smax:
            stride = R + max(smax, self._rows[1].shape[1] - R if self._rows is not None and
                             self._rows[1].shape[0] == C else 0)
            srow, hrow = np.zeros((C, 2 * stride), np.int8), np.zeros((C, stride), np.uint8)
            lead = np.full(C, 2 * R, np.int32)
            if self._rows is not None and self._rows[1].shape[0] == C:   # keep the carried tails
                srow[:, :2 * R], hrow[:, :R] = self._rows[0][:, :2 * R], self._rows[1][:, :R]
                lead = self._rows[2]
            self._rows = (srow, hrow, lead)
            self._alt = None
        srow, hrow, lead = self._rows
        stride = hrow.shape[1]
        # the quality and traffic passes read the rows after the call
        intact = self.link_quality or self.timebase_vote or self.traffic
        if intact and self._alt is None:
            self._alt = (np.zeros_like(srow), np.zeros_like(hrow))
        hrow[:, R:R + smax] = hard
        srow[:, 2 * R:2 * R + 2 * smax] = soft
        nb = np.zeros(C, np.int32)
        bursts = np.zeros((C, _hip.ETSI_MAXB, 2), np.int32)
        nk = np.zeros(C, np.int32)
        blocks = np.zeros((C, _hip.ETSI_MAXJ, 4), np.int32)
        t1 = np.zeros((C, _hip.ETSI_MAXJ, 268), np.uint8)
        # link_quality: the tails go to the other rows, these stay as the call read them
        nxt = self._alt if intact else ()
        used = self._run_stream(_hip.ctx(), C, nb, bursts, nk, blocks, t1, cells,
                                (srow, hrow, nsym, stride, lead) + tuple(nxt))
        lq = self._run_quality(_hip.ctx(), srow, hrow, 2 * R, used, nb, bursts, nk, blocks, t1)
        if intact:
            self._rows, self._alt = (nxt[0], nxt[1], lead), (srow, hrow)
        if self.mac and (self._tdma is None or len(self._tdma) != C):
            self._tdma = np.zeros(C, _hip.ETSI_TDMA)
            self.tdma_score = None
        if self.timebase_vote and self.tdma_score is None:
            self.tdma_score = np.zeros(C, np.int32)
        mac = self._run_mac(_hip.ctx(), C, nsym, nb, bursts, nk, blocks, t1, self._tdma, lq, self.tdma_score)
        tr = self._run_traffic(_hip.ctx(), srow, 2 * R, used, nb, bursts, nk, blocks, mac, used is self.cell_state)
        if self.sdu and (self._frag is None or len(self._frag) != C):
            self._frag = np.zeros(C, _hip.ETSI_FRAG)
        sd = self._run_sdu(_hip.ctx(), nsym, nb, bursts, nk, blocks, t1, mac, self._frag)
        return self._frames(C, nb, bursts, nk, blocks, t1, mac, lq if self.link_quality else None, tr, sd)

    @staticmethod
    def _frames(C, nb, bursts, nk, blocks, t1, mac=None, lq=None, tr=None, sd=None, G=1):
        """mac: None, or tetra_etsi_mac's (slots, npdu, pdus) for the same call; lq: None, or
        tetra_etsi_link_quality's (bq, kq); tr: None, or tetra_etsi_traffic's (tq, tch, has_cell [C]); sd:
        None, or tetra_etsi_sdu's (sdu, sdu_data, ndone, done, done_data) over groups of G rows, with
        tetra_etsi_llc's (llc, tl, llc_done, tl_done) behind them when llc=True."""
        out = []
        for ch in range(C):
            frames = []
            for b in range(int(nb[ch])):
                start, kind = int(bursts[ch, b, 0]), int(bursts[ch, b, 1])
                blks = []
                for j in range(int(nk[ch])):
                    if blocks[ch, j, 2] != b:
                        continue
                    k = int(blocks[ch, j, 0])
                    blks.append({"channel": BLOCK_NAMES[k], "crc_ok": bool(blocks[ch, j, 1]),
                                 "bits": t1[ch, j, :KIND_N1[k]].copy(), "block": int(blocks[ch, j, 3])})
                    if mac is not None:
                        n = int(mac[1][ch, j])
                        blks[-1].update(npdu=n, pdus=[pdu_dict(r) for r in mac[2][ch, j, :min(n, _hip.ETSI_MAXPDU)]])
                        if sd is not None:
                            for q, p in enumerate(blks[-1]["pdus"]):
                                p.update(sdu_keys(sd[0][ch, j, q], sd[1][ch, j]))
                                if len(sd) > 5:
                                    p["llc"] = llc_keys(sd[5][ch, j, q], sd[6][ch, j, int(sd[0][ch, j, q, _hip.SDU_BYTE]):])
                    if lq is not None:
                        blks[-1].update(block_quality(lq[1][ch, j], k))
                frames.append({"position": start, "burst": BURST_NAMES[kind], "burst_kind": kind,
                               "timeslot": (start // 510) % 4, "blocks": blks,
                               "crc_ok": all(x["crc_ok"] for x in blks)})
                if mac is not None:
                    tn, fn, mn, fl = (int(v) for v in mac[0][ch, b])
                    known = tn != 0
                    frames[-1].update(tn=tn if known else None, fn=fn if known else None, mn=mn if known else None,
                                      slot_flags=fl)
                if lq is not None:
                    frames[-1].update(burst_quality(lq[0][ch, b]))
                if tr is not None:
                    frames[-1].update(traffic_keys(tr[0][ch, b], tr[1][ch, b], kind, bool(tr[2][ch])))
            out.append(frames)
        if sd is not None:   # a finished chain goes to the frame of the burst that held its MAC-END
            for g in range(C // G):
                for i in range(min(int(sd[2][g]), sd[3].shape[1])):
                    row, b = int(sd[3][g, i, _hip.DONE_ROW]), int(sd[3][g, i, _hip.DONE_BURST])
                    blk = int(blocks[row, int(sd[3][g, i, _hip.DONE_BLOCK]), 3])
                    out[row][b].setdefault("sdus", []).append(done_dict(sd[3][g, i], sd[4][g, i], blk))
                    if len(sd) > 5:
                        out[row][b]["sdus"][-1]["llc"] = llc_keys(sd[7][g, i], sd[8][g, i])
        return out

    def decode(self, symbols, soft_bits=None, stream=True):
        """One chunk of hard dibit symbols (process() output in etsi mode carries soft_bits).
        ``stream`` (default): the chunk continues the stream of the previous calls (decode_stream;
        TetraDecoder(mode='etsi').decode behind SignalProcessor(mode='etsi').process, as the
        reference's capture loop calls them chunk after chunk); reset_stream() starts a new one.
        ``stream=False``: the chunk on its own (decode_batch)."""
        h = np.asarray(symbols, np.uint8)
        sb = soft_bits if soft_bits is not None else getattr(symbols, "soft_bits", None)
        if sb is None:   # hard decisions only: +-64 soft values
            bits = np.stack([(h >> 1) & 1, h & 1], axis=1).reshape(-1)
            sb = np.where(bits == 0, 64, -64).astype(np.int8)
        n = len(h)
        smax = n + 2
        hard = np.zeros((1, smax), np.uint8)
        hard[0, :n] = h
        soft = np.zeros((1, 2 * smax), np.int8)
        soft[0, :2 * n] = np.asarray(sb, np.int8)[:2 * n]
        if stream:
            return self.decode_stream(soft, hard, np.array([n + 1], np.int32))[0]
        return self.decode_batch(soft, hard, np.array([n + 1], np.int32))[0]
