"""CPU model of tetra_etsi_llc (TEST INFRASTRUCTURE): the LLC record of a TM-SDU, the frame check sequence
and the TL-SDU, restated from include/tetra_hip.h in plain Python on lists of bits -- the register rule one
bit a step, no table, no split -- and a writer that goes forwards from the header table (type, N(R), N(S),
TL-SDU, FCS appended) and shares nothing with the reader but the register rule.  Bit 0 is the first bit on
air, fields are MSB first.
"""
import numpy as np

import _etsi_mac_model as M
import _etsi_sdu_model as S

MAXJ, MAXPDU = S.MAXJ, S.MAXPDU
LLC_FIELDS = 10
STATUS, TYPE, NR, NS, OFFSET, NBITS, HEAD, FCS, FCS_RX, FCS_CALC = range(10)
OK, NONE, MALFORMED, ENCRYPTED, UNSUPPORTED = range(5)
FCS_NONE, FCS_GOOD, FCS_BAD = range(3)
POLY = 0x04C11DB7
RESIDUE = 0xC704DD7B   # the register after a message and its own FCS

# the sequence bits behind the type, by type & 3: BL-ADATA, BL-DATA, BL-UDATA, BL-ACK
SEQUENCE = {0: ("nr", "ns"), 1: ("ns",), 2: (), 3: ("nr",)}


# ------------------------------------------------------------------------------ the FCS

def register(bits, r=0xFFFFFFFF):
    """The register after `bits`, from r."""
    for b in bits:
        t = (r >> 31) ^ (int(b) & 1)
        r = (r << 1) & 0xFFFFFFFF
        if t:
            r ^= POLY
    return r


def fcs(bits):
    return register(bits) ^ 0xFFFFFFFF


def bits_of_bytes(data):
    return [(x >> (7 - i)) & 1 for x in data for i in range(8)]


# ------------------------------------------------------------------------------ the reader

def blank(status, type_=0):
    r = [0] * LLC_FIELDS
    r[STATUS], r[TYPE], r[NR], r[NS] = status, type_, -1, -1
    return r


def read_pdu(bits):
    """The rules both parts share, on an LLC PDU's bits: (record, TL-SDU bits)."""
    n = len(bits)
    if n < 4:
        return blank(MALFORMED), []
    t = M._get(bits, 0, 4)
    if t >= 8:
        return blank(UNSUPPORTED, t), []
    seq = SEQUENCE[t & 3]
    hdr, has_fcs = 4 + len(seq), bool(t & 4)
    if n < hdr + (32 if has_fcs else 0):
        return blank(MALFORMED), []
    r = blank(OK, t)
    for i, name in enumerate(seq):
        r[NR if name == "nr" else NS] = bits[4 + i]
    end = n - 32 if has_fcs else n
    tl = list(bits[hdr:end])
    r[OFFSET], r[NBITS] = hdr, len(tl)
    r[HEAD] = -1 if len(tl) < 3 else M._get(tl[:8] + [0] * 8, 0, 8)
    if has_fcs:
        rx, calc = M._get(bits, end, 32), fcs(bits[:end])
        r[FCS], r[FCS_RX], r[FCS_CALC] = (FCS_GOOD if rx == calc else FCS_BAD), rx, calc
    return r, tl


def read_whole(pdu, sdu, row):
    """Part A for one record: pdu the tetra_etsi_mac record, sdu the tetra_etsi_sdu record, row the block's
    sdu_data bytes.  (record, TL-SDU bits)."""
    if int(pdu[0]) != M.RESOURCE or int(sdu[S.ROLE]) != S.WHOLE:
        return blank(NONE), []
    if int(sdu[S.STATUS]) == S.ENCRYPTED or int(pdu[5]) != 0:
        return blank(ENCRYPTED, -1), []
    n, at = int(sdu[S.NBITS]), int(sdu[S.BYTE])
    if int(sdu[S.STATUS]) != S.OK or n <= 0:
        return blank(NONE), []
    if at < 0 or at + (n + 7) // 8 > S.SDU_ROW:
        return blank(MALFORMED), []
    return read_pdu(S.unpack(bytes(row[at:at + (n + 7) // 8]), n))


def read_done(rec, data):
    """Part B for one done record and its done_data row."""
    n = int(rec[S.D_NBITS])
    if int(rec[S.D_ENC]) != 0:
        return blank(ENCRYPTED, -1), []
    if n < 0 or n > 8 * S.SDU_MAXBYTES:
        return blank(MALFORMED), []
    if n == 0:
        return blank(NONE), []
    return read_pdu(S.unpack(bytes(data[:(n + 7) // 8]), n))


def signed(r):
    """The record as the int32 fields the library writes (FCS_RX / FCS_CALC hold the bit pattern)."""
    return [int(np.uint32(v & 0xFFFFFFFF).astype(np.int32)) if i in (FCS_RX, FCS_CALC) else v for i, v in enumerate(r)]


def run(G, nblock, blocks, npdu, pdus, sdu, sdu_data, maxd, ndone, done, done_data):
    """One tetra_etsi_llc call: ({(c, j, q): (record, TL-SDU bits, BYTE)}, {(g, i): (record, TL-SDU bits)})."""
    a, b = {}, {}
    for c in range(len(nblock)):
        for j in range(min(max(int(nblock[c]), 0), MAXJ)):
            kind, crc = int(blocks[c, j, 0]), int(blocks[c, j, 1])
            n = min(max(int(npdu[c, j]), 0), MAXPDU) if crc and kind in M.N1 else 0
            for q in range(n):
                rec, tl = read_whole(pdus[c, j, q], sdu[c, j, q], sdu_data[c, j])
                a[(c, j, q)] = (rec, tl, int(sdu[c, j, q, S.BYTE]))
    for g in range(len(nblock) // G):
        for i in range(min(max(int(ndone[g]), 0), maxd)):
            b[(g, i)] = read_done(done[g, i], done_data[g, i])
    return a, b


def expected_arrays(a, b, llc, tl, llc_done, tl_done):
    """Write what the library writes into copies of the caller's (sentinel-filled) output arrays; the done
    arrays may be None (maxd == 0)."""
    llc, tl = llc.copy(), tl.copy()
    llc_done, tl_done = (None, None) if llc_done is None else (llc_done.copy(), tl_done.copy())
    for (c, j, q), (rec, bits, at) in a.items():
        llc[c, j, q] = signed(rec)
        if rec[STATUS] == OK:
            d = S.pack(bits)
            tl[c, j, at:at + len(d)] = np.frombuffer(d, np.uint8)
    for (g, i), (rec, bits) in b.items():
        llc_done[g, i] = signed(rec)
        if rec[STATUS] == OK:
            d = S.pack(bits)
            tl_done[g, i, :len(d)] = np.frombuffer(d, np.uint8)
    return llc, tl, llc_done, tl_done


# ------------------------------------------------------------------------------ the writer

HEADER_BITS = {0: 6, 1: 5, 2: 4, 3: 5}


def llc_pdu(type_, tl_bits=(), nr=0, ns=0, flip=None):
    """An LLC PDU's bits: the 4-bit type, the sequence bits the type carries (BL-ADATA N(R) N(S), BL-DATA
    N(S), BL-ACK N(R)), the TL-SDU, and for types 4..7 the FCS of everything before it, MSB first.  Types
    8..15 get the TL-SDU bits behind the type as they are.  flip: a bit index of the finished PDU to invert."""
    b = M.bits_of(type_, 4)
    if type_ < 8:
        form = type_ & 3
        b += [nr, ns] if form == 0 else [ns] if form == 1 else [nr] if form == 3 else []
        assert len(b) == HEADER_BITS[form]
    b += [int(v) for v in tl_bits]
    if type_ < 8 and type_ & 4:
        b += M.bits_of(fcs(b), 32)
    if flip is not None:
        b[flip] ^= 1
    return b


def capacity(type_, nbits):
    """The longest TL-SDU whose LLC PDU of this type fits nbits bits."""
    return nbits - HEADER_BITS[type_ & 3] - (32 if type_ & 4 else 0)
