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
With ``follow=True`` (and ``sdu=True``) tetra_etsi_assign (k_assign_scan, k_assign_events, k_assign_follow)
follows: the channel allocations the control channel announces are listed with the carrier they name, and
every burst says whether its carrier and timeslot were assigned, to whom and since when (``assigned`` /
``assignment`` / ``allocations``; ``assigned_streams`` lists a carrier's assigned traffic frames).
"""
import dataclasses
from collections import namedtuple

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


# What each stage of the chain leaves, as host arrays over C rows in G-row groups (one group a carrier).


class LowerMac(namedtuple("LowerMac", "nb bursts nk blocks t1")):
    """tetra_lmac_etsi*: nb [C], bursts [C, MAXB, 2], nk [C], blocks [C, MAXJ, 4], t1 [C, MAXJ, 268]."""
    __slots__ = ()

    @classmethod
    def zeros(cls, C):
        """The outputs a lower-MAC call over C rows fills."""
        return cls(np.zeros(C, np.int32), np.zeros((C, _hip.ETSI_MAXB, 2), np.int32), np.zeros(C, np.int32),
                   np.zeros((C, _hip.ETSI_MAXJ, 4), np.int32), np.zeros((C, _hip.ETSI_MAXJ, 268), np.uint8))

    def ptrs(self):
        return tuple(_hip.ptr(v) for v in self)


class Mac(namedtuple("Mac", "slots npdu pdus keep slots_reported", defaults=(None, True))):
    """tetra_etsi_mac*: slots [C, MAXB, 4], npdu [C, MAXJ], pdus [C, MAXJ, MAXPDU, 16]; keep [C, MAXB] int32 from
    the grouped forms (the copy of each burst kept); slots_reported False: the PDU walk alone ran, a fresh
    timebase per row, and the frames get no tn / fn / mn / slot_flags."""
    __slots__ = ()

    @classmethod
    def zeros(cls, C, keep=False):
        return cls(np.zeros((C, _hip.ETSI_MAXB, _hip.SLOT_FIELDS), np.int32), np.zeros((C, _hip.ETSI_MAXJ), np.int32),
                   np.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.PDU_FIELDS), np.int32),
                   np.zeros((C, _hip.ETSI_MAXB), np.int32) if keep else None)


# tetra_etsi_link_quality: bq [C, MAXB, 4], kq [C, MAXJ, 4], -1 where not written
LinkQuality = namedtuple("LinkQuality", "bq kq")
# tetra_etsi_traffic: tq [C, MAXB, 4], -1 where not written, tch [C, MAXB, 432]; has_cell [C] bool: the row was
# descrambled with a known cell
Traffic = namedtuple("Traffic", "tq tch has_cell")
# tetra_etsi_sdu: sdu [C, MAXJ, MAXPDU, 8], sdu_data [C, MAXJ, 40], ndone [C / G], done [C / G, maxd, 13], done_data
# [C / G, maxd, 512]
Sdu = namedtuple("Sdu", "sdu sdu_data ndone done done_data")
# tetra_etsi_llc: llc [C, MAXJ, MAXPDU, 10], tl [C, MAXJ, 40], llc_done [C / G, maxd, 10], tl_done [C / G, maxd, 512]
Llc = namedtuple("Llc", "llc tl llc_done tl_done")


def run_link_quality(c, soft, hard, origin, G, cells, lm):
    """tetra_etsi_link_quality on host arrays, lm the LowerMac of the rows: LinkQuality."""
    C, stride = hard.shape
    cells = np.ascontiguousarray(cells, np.uint32)
    lq = LinkQuality(np.full((C, _hip.ETSI_MAXB, _hip.LQ_FIELDS), -1, np.int32),
                     np.full((C, _hip.ETSI_MAXJ, _hip.LQ_FIELDS), -1, np.int32))
    c.check(c.lib.tetra_etsi_link_quality(c.handle, _hip.ptr(soft), _hip.ptr(hard), C, stride, origin, G,
                                          _hip.ptr(cells), *lm.ptrs(), _hip.ptr(lq.bq), _hip.ptr(lq.kq)),
            "tetra_etsi_link_quality")
    return lq


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


def run_traffic(c, soft, origin, G, cells, lm, has_cell, mac=None):
    """tetra_etsi_traffic on host arrays (soft [C, 2 stride]): Traffic.  mac: None, or the Mac whose reported
    slots (frame 18 never carries traffic) and keep it is given."""
    C, stride = soft.shape[0], soft.shape[1] // 2
    cells = np.ascontiguousarray(cells, np.uint32)
    tr = Traffic(np.full((C, _hip.ETSI_MAXB, _hip.TQ_FIELDS), -1, np.int32),
                 np.zeros((C, _hip.ETSI_MAXB, _hip.TCH_BITS), np.int8), has_cell)
    timed = mac is not None and mac.slots_reported
    c.check(c.lib.tetra_etsi_traffic(c.handle, _hip.ptr(soft), C, stride, origin, G, _hip.ptr(cells), _hip.ptr(lm.nb),
                                     _hip.ptr(lm.bursts), _hip.ptr(lm.nk), _hip.ptr(lm.blocks),
                                     _hip.ptr(mac.slots if timed else None), _hip.ptr(mac.keep if timed else None),
                                     _hip.ptr(tr.tq), _hip.ptr(tr.tch)), "tetra_etsi_traffic")
    return tr


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


def run_sdu(c, nsym, G, row_bits, advance, lm, mac, keep, frag, maxd=SDU_MAXD, gap_slots=_hip.TDMA_EXPIRE):
    """tetra_etsi_sdu on host arrays behind the Mac's PDU records, frag [C / G] (_hip.ETSI_FRAG) updated in
    place: Sdu.  keep: the bursts that feed the chains ([C, MAXB] int32), or None with nsym (the streaming form)."""
    C = len(lm.nb)
    sd = Sdu(np.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.SDU_FIELDS), np.int32),
             np.zeros((C, _hip.ETSI_MAXJ, _hip.SDU_ROW), np.uint8), np.zeros(C // G, np.int32),
             np.zeros((C // G, maxd, _hip.DONE_FIELDS), np.int32), np.zeros((C // G, maxd, _hip.SDU_MAXBYTES), np.uint8))
    c.check(c.lib.tetra_etsi_sdu(c.handle, _hip.ptr(nsym), C, G, row_bits, advance, gap_slots, *lm.ptrs(),
                                 _hip.ptr(mac.npdu), _hip.ptr(mac.pdus), _hip.ptr(keep), _hip.ptr(sd.sdu),
                                 _hip.ptr(sd.sdu_data), _hip.ptr(frag), maxd, _hip.ptr(sd.ndone), _hip.ptr(sd.done),
                                 _hip.ptr(sd.done_data)), "tetra_etsi_sdu")
    return sd


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


def run_llc(c, G, lm, mac, sd):
    """tetra_etsi_llc on host arrays behind run_sdu's Sdu: Llc."""
    C, maxd = len(lm.nk), sd.done.shape[1]
    ll = Llc(np.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.LLC_FIELDS), np.int32),
             np.zeros((C, _hip.ETSI_MAXJ, _hip.SDU_ROW), np.uint8), np.zeros((C // G, maxd, _hip.LLC_FIELDS), np.int32),
             np.zeros((C // G, maxd, _hip.SDU_MAXBYTES), np.uint8))
    c.check(c.lib.tetra_etsi_llc(c.handle, C, G, _hip.ptr(lm.nk), _hip.ptr(lm.blocks), _hip.ptr(mac.npdu),
                                 _hip.ptr(mac.pdus), _hip.ptr(sd.sdu), _hip.ptr(sd.sdu_data), maxd, _hip.ptr(sd.ndone),
                                 _hip.ptr(sd.done), _hip.ptr(sd.done_data), *(_hip.ptr(v) for v in ll)), "tetra_etsi_llc")
    return ll


# tetra_etsi_assign: nev [C / G], ev [C / G, maxe, 16], ta [C, MAXB, 8], -1 where not written; row_key [C / G] int32 or None
Assign = namedtuple("Assign", "nev ev ta row_key")
ASSIGN_MAXE = 16   # events a row (or a wideband carrier's group) can return from one call
# The carrier numbering (include/tetra_hip.h, tetra_etsi_assign), transcribed from EN 300 392-2 and NOT pinned
# against a conformance vector: keys count 6.25 kHz, a band is 100 MHz, a carrier 25 kHz.
KEY_HZ, KEY_BAND, KEY_CARRIER = 6250, 16000, 4
KEY_OFFSET = {0: 0, 1: 1, 2: 2, 3: -1}   # a key's two low bits -> its offset from the 25 kHz raster, in keys
EXT_OFFSET = {0: 0, 1: 1, 2: -1, 3: 2}   # the extended carrier numbering's offset field -> the same


def carrier_key(hz):
    """The key of a downlink carrier frequency: hz / 6250.  ValueError unless hz is a multiple of 6250 Hz."""
    k = int(round(float(hz) / KEY_HZ))
    if k < 0 or k * KEY_HZ != float(hz):
        raise ValueError(f"a carrier frequency is a non-negative multiple of {KEY_HZ} Hz, not {hz!r}")
    return k


def key_hz(key):
    """The frequency in Hz of a key; None for an unknown (negative) key."""
    return None if key is None or int(key) < 0 else int(key) * KEY_HZ


def allocation_key(ca, own_key):
    """The key a channel_allocation dict (sdu_keys) names when the carrier with own_key sent it, -1 when it
    cannot be told: tetra_etsi_assign's TARGET, restated on the host."""
    if "carrier" not in ca:   # the augmented form stops before the carrier number
        return -1
    ext = ca.get("extended")
    if ext is not None:
        return ext["band"] * KEY_BAND + KEY_CARRIER * ca["carrier"] + EXT_OFFSET[ext["offset"]]
    if own_key is None or int(own_key) < 0:
        return -1
    off = KEY_OFFSET[int(own_key) & 3]
    return (int(own_key) - off) // KEY_BAND * KEY_BAND + KEY_CARRIER * ca["carrier"] + off


def run_assign(c, nsym, G, row_bits, advance, lm, mac, keep, sd, tq, state, row_key, shared_clock, maxe=ASSIGN_MAXE,
               hold_slots=_hip.ASSIGN_HOLD_DEFAULT, idle_max=_hip.ASSIGN_IDLE_DEFAULT):
    """tetra_etsi_assign on host arrays behind run_sdu's Sdu, state [C / G] (_hip.ETSI_ASSIGN) updated in place:
    Assign.  keep: what run_sdu was given; tq: the traffic call's records or None; row_key [C / G] int32 or None."""
    C = len(lm.nb)
    row_key = None if row_key is None else np.ascontiguousarray(row_key, np.int32)
    asg = Assign(np.zeros(C // G, np.int32), np.full((C // G, maxe, _hip.AE_FIELDS), -1, np.int32),
                 np.full((C, _hip.ETSI_MAXB, _hip.TA_FIELDS), -1, np.int32), row_key)
    c.check(c.lib.tetra_etsi_assign(c.handle, _hip.ptr(nsym), C, G, row_bits, advance, hold_slots, idle_max,
                                    int(bool(shared_clock)), _hip.ptr(lm.nb), _hip.ptr(lm.bursts), _hip.ptr(lm.nk),
                                    _hip.ptr(lm.blocks), _hip.ptr(mac.npdu), _hip.ptr(mac.pdus), _hip.ptr(keep),
                                    _hip.ptr(mac.slots), _hip.ptr(tq), _hip.ptr(sd.sdu), sd.done.shape[1], _hip.ptr(sd.ndone),
                                    _hip.ptr(sd.done), _hip.ptr(row_key), _hip.ptr(state), maxe, _hip.ptr(asg.nev),
                                    _hip.ptr(asg.ev), _hip.ptr(asg.ta)), "tetra_etsi_assign")
    return asg


def allocation_dict(rec, row_key, block):
    """One event record of tetra_etsi_assign as an entry of a frame's ``allocations``: the raw fields, ``target_hz``
    (None when the target cannot be told) and ``target_row`` (the group of this call with that key, else None);
    ``block`` (the block's index in its burst) and ``pdu`` say where the PDU sat."""
    r = [int(v) for v in rec]
    head, ext, target = r[_hip.AE_HEAD], r[_hip.AE_EXT], r[_hip.AE_TARGET]
    rows = np.flatnonzero(row_key == target) if row_key is not None and target >= 0 else ()
    d = {"kind": PDU_NAMES[r[_hip.AE_KIND]], "block": block, "pdu": r[_hip.AE_PDU],
         "allocation_type": (head >> 8) & 3, "timeslot_assigned": (head >> 4) & 15, "updownlink_assigned": (head >> 2) & 3,
         "clch_permission": (head >> 1) & 1, "cell_change": head & 1, "carrier": r[_hip.AE_CARRIER],
         "extended": None if ext < 0 else {"band": ext >> 6, "offset": (ext >> 4) & 3, "duplex_spacing": (ext >> 1) & 7,
                                           "reverse_operation": ext & 1},
         "target_hz": key_hz(target), "target_row": int(rows[0]) if len(rows) else None,
         "ssi": None if r[_hip.AE_SSI] < 0 else r[_hip.AE_SSI], "address_type": r[_hip.AE_ADDR_TYPE],
         "aux": None if r[_hip.AE_AUX] < 0 else r[_hip.AE_AUX]}
    return d


def assignment_keys(rec):
    """One ta record of tetra_etsi_assign as the keys a frame gains: ``assigned`` (True: the control channel
    assigned this carrier and timeslot and nothing ended it since; False; None: the burst was not followed -- a
    copy not kept, no timeslot yet) and ``assignment`` (None, or dict(ssi, address_type, usage_marker, from_hz,
    age_slots, allocations, idle))."""
    r = [int(v) for v in rec]
    if r[_hip.TA_STATE] != 1:
        return {"assigned": False if r[_hip.TA_STATE] == 0 else None, "assignment": None}
    at = r[_hip.TA_ADDR_TYPE]
    return {"assigned": True,
            "assignment": {"ssi": None if r[_hip.TA_SSI] < 0 else r[_hip.TA_SSI], "address_type": at,
                           "usage_marker": r[_hip.TA_AUX] if at == 6 else None, "from_hz": key_hz(r[_hip.TA_SRC_KEY]),
                           "age_slots": r[_hip.TA_AGE], "allocations": r[_hip.TA_NALLOC], "idle": r[_hip.TA_IDLE]}}


def assigned_streams(frames):
    """One carrier's frames (traffic=True, follow=True) -> {tn: [frame, ...]} of its "traffic" and "stolen" frames
    whose timeslot the control channel assigned (``assigned`` True), in the order given: traffic_streams with
    the announcement as the gate."""
    out = {}
    for f in frames:
        if f.get("usage") in ("traffic", "stolen") and f.get("assigned") is True:
            out.setdefault(f.get("tn"), []).append(f)
    return out


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


# The stages that follow the lower MAC.  timebase: None, "walk" (the PDU walk per row, slots not reported), "mac"
# (tetra_etsi_mac), "groups" (tetra_etsi_mac_groups) or "vote" (tetra_etsi_mac_vote_groups); vote_cap: the bound of the
# cell vote's scores, None without one.
ChainOptions = namedtuple("ChainOptions", "timebase link_quality traffic sdu llc tdma_cap vote_cap follow",
                          defaults=(False,))


def chain_options(mac=False, timebase=False, link_quality=False, traffic=False, sdu=False, llc=False,
                  tdma_cap=_hip.TETRA_TDMA_VOTE_CAP_DEFAULT, vote_cap=None, grouped=False, follow=False):
    """The one place the option rules live: ChainOptions, or ValueError.  timebase: False, True or "vote".
    grouped False (EtsiLowerMac: rows are channels): the timebase is that of mac=True, the vote on it needs
    mac=True.  grouped True (wideband: G chunk rows a carrier): mac=True alone is the PDU walk, timebase=True
    merges the rows and implies it, and sdu=True needs both.  vote_cap: None unless the cells are voted on.
    follow=True reads the SDU call's records and the MAC call's slots: it needs what sdu=True needs, and sdu=True."""
    if timebase not in (False, True, "vote"):
        raise ValueError(f"timebase={timebase!r}: False, True or 'vote'")
    if timebase == "vote" and not (mac or grouped):
        raise ValueError("timebase_vote=True chooses the timebase of mac=True")
    if sdu and not (mac and (timebase or not grouped)):
        raise ValueError("sdu=True reads the PDU records of mac=True" +
                         (" and the keep of timebase=True or 'vote'" if grouped else ""))
    if llc and not sdu:
        raise ValueError("llc=True reads the TM-SDUs of mac=True, sdu=True")
    if follow and not sdu:
        raise ValueError("follow=True reads the channel allocations of mac=True, sdu=True" +
                         (" on the timebase of timebase=True or 'vote'" if grouped else ""))
    if timebase == "vote" and int(tdma_cap) <= 0:
        raise ValueError(f"tdma_cap ({tdma_cap}) must be positive")
    if vote_cap is not None and int(vote_cap) <= 0:
        raise ValueError(f"vote_cap ({vote_cap}) must be positive")
    if grouped:
        variant = "vote" if timebase == "vote" else "groups" if timebase else "walk" if mac else None
    else:
        variant = None if not mac else "vote" if timebase == "vote" else "mac"
    return ChainOptions(variant, bool(link_quality), bool(traffic), bool(sdu), bool(llc), int(tdma_cap),
                        None if vote_cap is None else int(vote_cap), bool(follow))


class Geometry(namedtuple("Geometry", "G row_bits tol_bits advance", defaults=(1, 0, 32, None))):
    """How the rows of a call lie: G rows a group, row r of a group starting r row_bits after the group's first,
    copies of a burst within tol_bits of each other, and the group's stream moving on by ``advance`` bits after
    the call.  advance None: every row is a channel's own stream (G = 1), which moves on by its chunk's length."""
    __slots__ = ()


@dataclasses.dataclass
class Carried:
    """What a stream carries from call to call, one element a group, updated in place (None: a fresh stream):
    the timebases ([C / G] ETSI_TDMA), the scores they gathered (int32, timebase "vote"), the fragment chains
    (ETSI_FRAG, sdu) and the assigned timeslots (ETSI_ASSIGN, follow)."""
    tdma: np.ndarray = None
    tdma_score: np.ndarray = None
    frag: np.ndarray = None
    walked: np.ndarray = None   # [C / G], 72 kHz samples of this call's rows: the bursts up to there fed the chains before
    assign: np.ndarray = None


def run_mac(c, nsym, lm, tdma=None):
    """tetra_etsi_mac on the lower MAC's outputs, tdma [C] in/out (None: a new stream per row): Mac."""
    C = len(lm.nb)
    tdma = np.zeros(C, _hip.ETSI_TDMA) if tdma is None else tdma
    mac = Mac.zeros(C)
    c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(nsym), C, *lm.ptrs(), _hip.ptr(tdma), _hip.ptr(mac.slots),
                                 _hip.ptr(mac.npdu), _hip.ptr(mac.pdus)), "tetra_etsi_mac")
    return mac


def run_mac_groups(c, nsym, geo, advance, cap, lm, lq, tdma, score):
    """tetra_etsi_mac_groups, or with lq (the rows' LinkQuality) tetra_etsi_mac_vote_groups with the scores
    score [C / G] bounded by cap: (Mac with keep, the call's ballots [C / G, 4] or None); tdma, score in/out."""
    C = len(lm.nb)
    mac = Mac.zeros(C, keep=True)
    where = (c.handle, _hip.ptr(nsym), C, geo.G, geo.row_bits, geo.tol_bits, advance)
    outs = tuple(_hip.ptr(v) for v in (mac.keep, mac.slots, mac.npdu, mac.pdus))
    if lq is None:
        c.check(c.lib.tetra_etsi_mac_groups(*where, *lm.ptrs(), _hip.ptr(tdma), *outs), "tetra_etsi_mac_groups")
        return mac, None
    votes = np.zeros((C // geo.G, _hip.TV_FIELDS), np.int32)
    c.check(c.lib.tetra_etsi_mac_vote_groups(*where, cap, *lm.ptrs(), _hip.ptr(lq.bq), _hip.ptr(lq.kq), _hip.ptr(tdma),
                                             _hip.ptr(score), *outs, _hip.ptr(votes)), "tetra_etsi_mac_vote_groups")
    return mac, votes


def run_mac_vote_rows(c, nsym, cap, lm, lq, tdma, score):
    """tetra_etsi_mac_vote_groups over rows that are each a channel's own stream (G = 1, row_bits = 0): advance
    is one value a call, so the channels of one chunk length go together, advance = 2 max(nsym - 1, 0), and
    the in/out arrays are scattered back.  (Mac without keep: one row a group, nothing to choose; ballots [C, 4])."""
    C = len(lm.nb)
    mac, votes = Mac.zeros(C), np.zeros((C, _hip.TV_FIELDS), np.int32)
    for n in np.unique(nsym):
        idx = np.flatnonzero(nsym == n)
        if len(idx) == C:
            part, pv = run_mac_groups(c, nsym, Geometry(), 2 * max(int(n) - 1, 0), cap, lm, lq, tdma, score)
            return part._replace(keep=None), pv
        ns_i, tdma_i, score_i = (np.ascontiguousarray(v[idx]) for v in (nsym, tdma, score))
        part, pv = run_mac_groups(c, ns_i, Geometry(), 2 * max(int(n) - 1, 0), cap,
                                  LowerMac(*(np.ascontiguousarray(v[idx]) for v in lm)),
                                  LinkQuality(*(np.ascontiguousarray(v[idx]) for v in lq)), tdma_i, score_i)
        for dst, src in zip((tdma, score, mac.slots, mac.npdu, mac.pdus, votes),
                            (tdma_i, score_i, part.slots, part.npdu, part.pdus, pv)):
            dst[idx] = src
    return mac, votes


def run_chain(c, opt, geo, soft, hard, nsym, origin, cells, has_cell, lm, carried, row_key=None, shared_clock=False):
    """The chain behind a lower-MAC call, the one place its order lives: link quality -> MAC -> traffic -> SDU ->
    LLC -> assign -> frames.  soft [C, 2 stride] / hard [C, stride]: the rows the call read, intact, their first bit at
    ``origin``; nsym [C]; cells [C / G]: the inits they were descrambled with; has_cell [C] bool; lm: the call's
    LowerMac; carried: Carried, updated in place.  Returns (frames per row, Mac or None, Sdu or None, the vote's
    ballots or None).  What each stage reads: link quality runs for its keys or for the vote's weights; traffic
    is given the slots and keep of a MAC call that reports them; the SDU call feeds the bursts the grouped MAC
    call kept (less those before ``carried.walked``, in 72 kHz samples, which the previous buffer fed), or with
    rows that are streams of their own every burst of nsym; LLC reads the SDU call's records; assign (opt.follow)
    reads them too, with the keep the SDU call got, the traffic call's records when it ran, and row_key [C / G]
    (the groups' carrier keys, None: unknown) / shared_clock (the groups count one sample clock)."""
    C, G = len(lm.nb), geo.G
    lq = mac = tr = sd = ll = asg = votes = None
    if opt.link_quality or opt.timebase == "vote":
        lq = run_link_quality(c, soft, hard, origin, G, cells, lm)
    if opt.timebase == "walk":
        mac = run_mac(c, nsym, lm)._replace(slots_reported=False)
    elif opt.timebase:
        if carried.tdma is None:
            carried.tdma = np.zeros(C // G, _hip.ETSI_TDMA)
        if opt.timebase == "vote" and carried.tdma_score is None:
            carried.tdma_score = np.zeros(C // G, np.int32)
        if opt.timebase == "mac":
            mac = run_mac(c, nsym, lm, carried.tdma)
        elif opt.timebase == "vote" and geo.advance is None:   # rows that are streams of their own
            assert G == 1 and geo.row_bits == 0
            mac, votes = run_mac_vote_rows(c, nsym, opt.tdma_cap, lm, lq, carried.tdma, carried.tdma_score)
        else:   # "groups", or "vote" with the link-quality records
            assert geo.advance is not None, "the grouped MAC calls take the call's advance"
            mac, votes = run_mac_groups(c, nsym, geo, geo.advance, opt.tdma_cap, lm, lq if opt.timebase == "vote" else None,
                                        carried.tdma, carried.tdma_score)
    if opt.traffic:
        tr = run_traffic(c, soft, origin, G, cells, lm, has_cell, mac)
    if opt.sdu:
        if carried.frag is None:
            carried.frag = np.zeros(C // G, _hip.ETSI_FRAG)
        fed = mac.keep
        if fed is not None and carried.walked is not None:   # the carried tail's bursts were fed from the previous buffer
            sample = 2 * ((np.arange(C) % G)[:, None] * geo.row_bits + lm.bursts[:, :, 0])
            fed = np.ascontiguousarray(fed * (sample > np.repeat(carried.walked, G)[:, None]), np.int32)
        sd = run_sdu(c, nsym if fed is None else None, G, geo.row_bits, geo.advance or 0, lm, mac, fed, carried.frag)
        if opt.llc:
            ll = run_llc(c, G, lm, mac, sd)
        if opt.follow:
            if carried.assign is None:
                carried.assign = np.zeros(C // G, _hip.ETSI_ASSIGN)
            asg = run_assign(c, nsym if fed is None else None, G, geo.row_bits, geo.advance or 0, lm, mac, fed, sd,
                             None if tr is None else tr.tq, carried.assign, row_key, shared_clock)
    return build_frames(lm, mac, lq if opt.link_quality else None, tr, sd, ll, G, asg), mac, sd, votes


def build_frames(lm, mac=None, lq=None, tr=None, sd=None, ll=None, G=1, asg=None):
    """The frame dicts of every row from the stages' records (None: the stage did not run), sd, ll and asg over
    groups of G rows.  A Mac whose slots are not reported gives the blocks their pdus and the frames no tn / fn / mn /
    slot_flags."""
    nb, bursts, nk, blocks, t1 = lm
    out = []
    for ch in range(len(nb)):
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
                    n = int(mac.npdu[ch, j])
                    blks[-1].update(npdu=n, pdus=[pdu_dict(r) for r in mac.pdus[ch, j, :min(n, _hip.ETSI_MAXPDU)]])
                    if sd is not None:
                        for q, p in enumerate(blks[-1]["pdus"]):
                            p.update(sdu_keys(sd.sdu[ch, j, q], sd.sdu_data[ch, j]))
                            if ll is not None:
                                p["llc"] = llc_keys(ll.llc[ch, j, q], ll.tl[ch, j, int(sd.sdu[ch, j, q, _hip.SDU_BYTE]):])
                if lq is not None:
                    blks[-1].update(block_quality(lq.kq[ch, j], k))
            frames.append({"position": start, "burst": BURST_NAMES[kind], "burst_kind": kind,
                           "timeslot": (start // 510) % 4, "blocks": blks,
                           "crc_ok": all(x["crc_ok"] for x in blks)})
            if mac is not None and mac.slots_reported:
                tn, fn, mn, fl = (int(v) for v in mac.slots[ch, b])
                known = tn != 0
                frames[-1].update(tn=tn if known else None, fn=fn if known else None, mn=mn if known else None,
                                  slot_flags=fl)
            if lq is not None:
                frames[-1].update(burst_quality(lq.bq[ch, b]))
            if tr is not None:
                frames[-1].update(traffic_keys(tr.tq[ch, b], tr.tch[ch, b], kind, bool(tr.has_cell[ch])))
            if asg is not None:
                frames[-1].update(assignment_keys(asg.ta[ch, b]), allocations=None)
        out.append(frames)
    if sd is not None:   # a finished chain goes to the frame of the burst that held its MAC-END
        for g in range(len(nb) // G):
            for i in range(min(int(sd.ndone[g]), sd.done.shape[1])):
                row, b = int(sd.done[g, i, _hip.DONE_ROW]), int(sd.done[g, i, _hip.DONE_BURST])
                blk = int(blocks[row, int(sd.done[g, i, _hip.DONE_BLOCK]), 3])
                out[row][b].setdefault("sdus", []).append(done_dict(sd.done[g, i], sd.done_data[g, i], blk))
                if ll is not None:
                    out[row][b]["sdus"][-1]["llc"] = llc_keys(ll.llc_done[g, i], ll.tl_done[g, i])
    if asg is not None:   # an allocation goes to the frame of the burst it was heard in
        for g in range(len(nb) // G):
            for i in range(min(int(asg.nev[g]), asg.ev.shape[1])):
                row = int(asg.ev[g, i, _hip.AE_ROW])
                f = out[row][int(asg.ev[g, i, _hip.AE_BURST])]
                blk = int(blocks[row, int(asg.ev[g, i, _hip.AE_BLOCK]), 3])
                f["allocations"] = (f["allocations"] or []) + [allocation_dict(asg.ev[g, i], asg.row_key, blk)]
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
    TL-SDU; ``link_messages(frames)`` lists the messages that read well.  Everything else is unchanged.

    ``follow=True`` (with ``mac=True, sdu=True``): tetra_etsi_assign runs after the SDU / LLC calls.  Every frame
    gains ``assigned`` (True: the control channel assigned this carrier and timeslot, and neither the hold time
    nor decoded control signalling ended it; False; None: the burst has no timeslot yet), ``assignment`` (None,
    or dict(ssi, address_type, usage_marker, from_hz, age_slots, allocations, idle)) and ``allocations`` (None,
    or the channel allocations heard in the burst, allocation_dict, each with ``target_hz`` / ``target_row``).
    ``carrier_hz``: the channels' downlink carrier frequencies, one value or one per channel, multiples of 6250
    Hz; without it every allocation is listed and nothing is assigned.  The channels' streams count their own
    clocks, so only a carrier's allocations onto itself apply (the wideband chain joins carriers).  This follows
    announcements, it is not the AACH: a call's end is inferred (``age_slots``, ``idle`` and ``soft_sum`` are what a
    caller gates on), and the carrier numbering is transcribed from EN 300 392-2, not pinned.  The state is
    carried like the timebase; ``assign_stats`` counts the entries that expired and that were released.
    ``assigned_streams(frames)`` lists a carrier's assigned traffic.  Everything else is unchanged."""

    def __init__(self, mcc=None, mnc=None, colour_code=None, mac=False, link_quality=False, vote=False,
                 vote_cap=_hip.TETRA_ETSI_VOTE_CAP_DEFAULT, timebase_vote=False,
                 tdma_cap=_hip.TETRA_TDMA_VOTE_CAP_DEFAULT, traffic=False, sdu=False, llc=False, follow=False,
                 carrier_hz=None):
        self.opt = chain_options(mac, "vote" if timebase_vote else False, link_quality, traffic, sdu, llc, tdma_cap,
                                 vote_cap if vote else None, follow=follow)
        self.follow = self.opt.follow
        # the channels' keys: None (unknown), one int for every channel, or one per channel
        self.carrier_keys = None if carrier_hz is None else carrier_key(carrier_hz) if np.ndim(carrier_hz) == 0 else \
            np.array([carrier_key(v) for v in carrier_hz], np.int32)
        self.mac, self.sdu, self.llc, self.traffic = bool(mac), self.opt.sdu, self.opt.llc, self.opt.traffic
        self.link_quality = self.opt.link_quality
        self.timebase_vote, self.tdma_cap = bool(timebase_vote), int(tdma_cap)
        self.tdma_votes = None   # [C, 4] int32: the last call's ballots (cast, agreed, outvoted, won)
        self.acquire = mcc is None and mnc is None and colour_code is None
        self.vote, self.vote_cap = bool(vote), int(vote_cap)
        if self.vote and not self.acquire:
            raise ValueError("vote=True chooses among acquired cells: it takes no mcc / mnc / colour_code")
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
        self._assign = None   # [C] tetra_etsi_assign_state: the carried assignments (follow=True)
        self._assign_last = None   # the state the last call left (decode_batch's is not carried)

    def reset_channels(self, mask):
        """The masked channels ([C] bool) start a new chain, the others go on: their carried dibits are
        dropped (the burst scan starts at the next chunk's first dibit) and their timebase, its score, the
        cell's score, the fragment chains and the assignments are cleared.  The cell (``cell_state``,
        ``acquired``) is kept: a receiver that re-acquired its timing is still on the same carrier.  From
        the next call on a reset channel's frames are those of a new EtsiLowerMac with the same options
        that was handed the cell.  What EtsiStream(lock=True) reports in ``fresh`` goes here."""
        mask = np.asarray(mask, bool)
        if not mask.any():
            return
        R = _hip.ETSI_RESERVE
        if self._rows is not None and len(mask) == self._rows[1].shape[0]:
            srow, hrow, lead = self._rows
            srow[mask, :2 * R] = 0
            hrow[mask, :R] = 0
            lead[mask] = 2 * R
        for a in (self._tdma, self.tdma_score, self.cell_score, self._frag, self._assign, self._lost):
            if a is not None and len(a) == len(mask):
                a[mask] = np.zeros((), a.dtype)

    @property
    def assign_stats(self):
        """follow=True: dict(expired [C], released [C]) -- assignments that ended after the hold time without
        a repeat or traffic, and that ended because the slot returned to decoded control signalling -- since
        the stream began (decode_batch: of that call); None before the first call."""
        if self._assign_last is None:
            return None
        return {"expired": self._assign_last["expired"].copy(), "released": self._assign_last["released"].copy()}

    def _row_keys(self, C):
        """row_key for a call over C channels, None when no carrier frequency was given."""
        if self.carrier_keys is None:
            return None
        if np.ndim(self.carrier_keys) == 0:
            return np.full(C, self.carrier_keys, np.int32)
        if len(self.carrier_keys) != C:
            raise ValueError(f"carrier_hz names {len(self.carrier_keys)} channels, the call has {C}")
        return self.carrier_keys
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
        lm = LowerMac.zeros(C)
        c = _hip.ctx()
        used, acquiring = self._cells_for(c, C, cells)
        rows = (c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, smax)
        if acquiring and self.vote:
            ngood, agree = np.zeros(C, np.int32), np.zeros(C, np.int32)
            c.check(c.lib.tetra_lmac_etsi_vote_groups(*rows, 1, self.vote_cap, _hip.ptr(used), _hip.ptr(self._score(C)),
                                                      _hip.ptr(ngood), _hip.ptr(agree), *lm.ptrs()),
                    "tetra_lmac_etsi_vote_groups")
        elif acquiring:
            c.check(c.lib.tetra_lmac_etsi_acquire(*rows, _hip.ptr(used), *lm.ptrs()), "tetra_lmac_etsi_acquire")
        else:
            c.check(c.lib.tetra_lmac_etsi(*rows, *lm.ptrs()), "tetra_lmac_etsi")
        return self._chain(c, soft, hard, nsym, 0, used, acquiring, lm, Carried(), False)

    def _score(self, C):
        """cell_score for C channels (vote=True): zeros when new or of another length."""
        if self.cell_score is None or len(self.cell_score) != C:
            self.cell_score = np.zeros(C, np.int32)
        return self.cell_score

    def _cells_for(self, c, C, cells):
        """The cells a lower-MAC call over C channels descrambles with: (the acquisition state, made anew when
        it is missing or of another length, True) in acquisition mode without given ``cells``; else (the given
        or configured cells, set on the device, False)."""
        if self.acquire and cells is None:
            if self.cell_state is None or len(self.cell_state) != C:
                self.cell_state = np.full(C, UNKNOWN_CELL, np.uint32)
                self.acquired = np.zeros(C, bool)
            if self.acquired is None or len(self.acquired) != C:   # cell_state handed in from outside
                self.acquired = np.zeros(C, bool)
            return self.cell_state, True
        cells = np.full(C, self.cell if self.cell is not None else UNKNOWN_CELL, np.uint32) if cells is None \
            else np.ascontiguousarray(cells, np.uint32)
        c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(cells), C), "tetra_etsi_set_cells")
        return cells, False

    def _chain(self, c, soft, hard, nsym, origin, used, acquiring, lm, carried, stream):
        """run_chain behind a lower-MAC call (one row a channel) and the receiver's bookkeeping of it: the
        channels that acquired a cell, the vote's ballots, the fragment statistics."""
        C = len(lm.nb)
        if acquiring:
            self.acquired |= acquired_channels(lm.nk, lm.blocks)
        has_cell = self.acquired.copy() if acquiring else np.ones(C, bool)
        frames, _, sd, votes = run_chain(c, self.opt, Geometry(), soft, hard, nsym, origin, used, has_cell, lm, carried,
                                         self._row_keys(C) if self.follow else None)
        if self.follow:
            self._assign_last = carried.assign
        if votes is not None:
            self.tdma_votes = votes
        if sd is not None:   # (decode_batch's fragment state is not carried; its statistics are that call's)
            if not stream or self._lost is None or len(self._lost) != C:
                self._lost = np.zeros(C, np.int64)
            self._frag_last = carried.frag
            self._lost += np.maximum(sd.ndone - SDU_MAXD, 0)
        return frames

    def decode_stream(self, soft, hard, nsym, cells=None, fresh=None):
        """decode_batch for consecutive chunks of C continuous streams (EtsiStream.demod rows):
        each channel's dibits the previous call left unconsumed -- from the first bit its burst scan
        did not examine -- go in front of this chunk's, and the scan resumes there
        (tetra_lmac_etsi_stream), so a burst across the seam is decoded whole.  Positions are
        relative to this chunk's first dibit (negative: the burst began in the carried tail).
        ``fresh`` ([C] bool, EtsiStream.fresh): the channels whose rows start a new chain
        (reset_channels, applied before the call)."""
        if fresh is not None:
            self.reset_channels(fresh)
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
        # the quality and traffic passes read the rows after the call: the tails then go to the other set of
        # rows, and these stay as the call read them
        intact = self.link_quality or self.timebase_vote or self.traffic
        if intact and self._alt is None:
            self._alt = (np.zeros_like(srow), np.zeros_like(hrow))
        hrow[:, R:R + smax] = hard
        srow[:, 2 * R:2 * R + 2 * smax] = soft
        nsrow, nhrow = self._alt if intact else (srow, hrow)
        lm = LowerMac.zeros(C)
        c = _hip.ctx()
        used, acquiring = self._cells_for(c, C, cells)
        rows = (c.handle, _hip.ptr(srow), _hip.ptr(hrow), _hip.ptr(nsym), C, stride, _hip.ptr(lead), _hip.ptr(nsrow),
                _hip.ptr(nhrow))
        if acquiring and self.vote:
            c.check(c.lib.tetra_lmac_etsi_stream_vote(*rows, self.vote_cap, _hip.ptr(used), _hip.ptr(self._score(C)),
                                                      None, *lm.ptrs()), "tetra_lmac_etsi_stream_vote")
        else:
            c.check(c.lib.tetra_lmac_etsi_stream(*rows, _hip.ptr(used) if acquiring else None, *lm.ptrs()),
                    "tetra_lmac_etsi_stream")
        if intact:
            self._rows, self._alt = (nsrow, nhrow, lead), (srow, hrow)
        if self._tdma is not None and len(self._tdma) != C:
            self._tdma = self.tdma_score = None
        if self._frag is not None and len(self._frag) != C:
            self._frag = None
        if self._assign is not None and len(self._assign) != C:
            self._assign = None
        carried = Carried(self._tdma, self.tdma_score, self._frag, assign=self._assign)
        frames = self._chain(c, srow, hrow, nsym, 2 * R, used, acquiring, lm, carried, True)
        self._tdma, self.tdma_score, self._frag, self._assign = carried.tdma, carried.tdma_score, carried.frag, carried.assign
        return frames

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
            new = bool(getattr(symbols, "new_stream", False))   # the receiver re-acquired (EtsiReceiver(relock=True))
            return self.decode_stream(soft, hard, np.array([n + 1], np.int32), fresh=[True] if new else None)[0]
        return self.decode_batch(soft, hard, np.array([n + 1], np.int32))[0]
