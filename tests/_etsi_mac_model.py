"""CPU model of tetra_etsi_mac (TEST INFRASTRUCTURE): builders, the PDU walk and the TDMA timebase.

The builders are written forwards from the layout tables of DESIGN.md §5.16 (fields in, PDU bits
out); the walk and the timebase restate include/tetra_hip.h's description in plain Python, table
driven, so that they share no code and no shape with k_etsi_mac.  Bit 0 is the first type-1 bit of
the block, fields are MSB first, a bit is byte & 1.
"""
import numpy as np

MAXB, MAXJ, MAXPDU, NF = 8, 16, 4, 16
TDMA_SLOTS, TDMA_TOL, TDMA_EXPIRE = 4320, 4, 72
N1 = {0: 268, 1: 124, 2: 60}
RESOURCE, FRAG, END, SYSINFO, ACCESS_DEFINE, BROADCAST, SUPPL, SYNC, NULL = range(9)
KIND_NAMES = ("RESOURCE", "FRAG", "END", "SYSINFO", "ACCESS-DEFINE", "BROADCAST", "SUPPLEMENTARY", "SYNC", "NULL")
TDMA_DTYPE = np.dtype([("bit0", "<i8"), ("anchor_bit", "<i8"), ("anchor_slot", "<i4"), ("locked", "<i4")])

# (name, first bit, width)
SYNC_LAYOUT = (("system_code", 0, 4), ("colour_code", 4, 6), ("tn", 10, 2), ("fn", 12, 5), ("mn", 17, 6),
               ("sharing_mode", 23, 2), ("ts_reserved_frames", 25, 3), ("dtx", 28, 1), ("frame18_extension", 29, 1),
               ("reserved", 30, 1), ("mcc", 31, 10), ("mnc", 41, 14), ("neighbour_cell_broadcast", 55, 2),
               ("cell_service_level", 57, 2), ("late_entry", 59, 1))
SYSINFO_LAYOUT = (("main_carrier", 4, 12), ("band", 16, 4), ("offset", 20, 2), ("duplex_spacing", 22, 3),
                  ("reverse_operation", 25, 1), ("num_cscch", 26, 2), ("ms_txpwr_max_cell", 28, 3),
                  ("rxlev_access_min", 31, 4), ("access_parameter", 35, 4), ("radio_downlink_timeout", 39, 4),
                  ("hyperframe_cck_flag", 43, 1), ("hyperframe_or_cck", 44, 16), ("optional_field_flag", 60, 2),
                  ("optional_field_value", 62, 20), ("location_area", 82, 14), ("subscriber_class", 96, 16),
                  ("bs_service_details", 112, 12))
RESOURCE_LAYOUT = (("fill", 2, 1), ("grant", 3, 1), ("enc", 4, 2), ("random_access", 6, 1), ("length", 7, 6),
                   ("addr_type", 13, 3))
END_LAYOUT = (("fill", 3, 1), ("grant", 4, 1), ("length", 5, 6))
# address type -> (has a 24-bit SSI / USSI / SMI, width of the event label or usage marker)
ADDRESS = {0: (False, 0), 1: (True, 0), 2: (False, 10), 3: (True, 0), 4: (True, 0), 5: (True, 10), 6: (True, 6),
           7: (True, 10)}


# ------------------------------------------------------------------------------ builders

def bits_of(v, n):
    assert 0 <= v < (1 << n), (v, n)
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def _lay(bits, layout, fields, base=0):
    for name, lo, n in layout:
        bits[base + lo:base + lo + n] = bits_of(int(fields.get(name, 0)), n)


def _body(rng, n, fill):
    """n bits after a header: random, or with fill bits (a 1, then 0s) when the fill flag is set."""
    if n <= 0:
        return []
    if fill:
        k = int(rng.integers(0, n))
        return rng.integers(0, 2, k).tolist() + [1] + [0] * (n - k - 1)
    return rng.integers(0, 2, n).tolist()


def resource(rng, length, addr_type, ssi=0, aux=0, fill=0, grant=0, enc=0, random_access=0, nbits=None):
    """A MAC-RESOURCE PDU of nbits bits (default 8 * length): header, address, then body bits."""
    hdr = [0] * 16
    _lay(hdr, RESOURCE_LAYOUT, dict(fill=fill, grant=grant, enc=enc, random_access=random_access, length=length,
                                   addr_type=addr_type))
    has_ssi, auxn = ADDRESS[addr_type]
    hdr += (bits_of(ssi, 24) if has_ssi else []) + (bits_of(aux, auxn) if auxn else [])
    nbits = 8 * length if nbits is None else nbits
    return (hdr + _body(rng, nbits - len(hdr), fill))[:max(nbits, 16)]


def null_pdu(fill=0, grant=0, enc=0, random_access=0, length=2):
    hdr = [0] * 16
    _lay(hdr, RESOURCE_LAYOUT, dict(fill=fill, grant=grant, enc=enc, random_access=random_access, length=length))
    return hdr


def mac_end(rng, length, fill=0, grant=0, nbits=None):
    hdr = [0, 1, 1] + [0] * 8
    _lay(hdr, END_LAYOUT, dict(fill=fill, grant=grant, length=length))
    nbits = 8 * length if nbits is None else nbits
    return (hdr + _body(rng, nbits - 11, fill))[:max(nbits, 16)]


def mac_frag(rng, nbits, fill=0):
    return [0, 1, 0, fill] + _body(rng, nbits - 4, fill)


def sysinfo(fields):
    b = [1, 0, 0, 0] + [0] * 120
    _lay(b, SYSINFO_LAYOUT, fields)
    return b


def broadcast(rng, sub, nbits):
    """ACCESS-DEFINE (sub 1) or another broadcast PDU (2, 3)."""
    return [1, 0] + bits_of(sub, 2) + rng.integers(0, 2, nbits - 4).tolist()


def supplementary(rng, nbits):
    return [1, 1] + rng.integers(0, 2, nbits - 2).tolist()


def sync(fields):
    b = [0] * 60
    _lay(b, SYNC_LAYOUT, fields)
    return b


def random_fields(rng, layout):
    return {name: int(rng.integers(0, 1 << n)) for name, lo, n in layout}


def sync_for_slot(rng, slot, cell=None, **over):
    """SYNC fields of slot count `slot` (TN/FN/MN), the rest random; cell = (mcc, mnc, colour code)."""
    f = random_fields(rng, SYNC_LAYOUT)
    f.update(tn=slot % 4, fn=slot // 4 % 18 + 1, mn=slot // 72 + 1)
    if cell is not None:
        f.update(mcc=cell[0], mnc=cell[1], colour_code=cell[2])
    f.update(over)
    return f


def block(rng, kind, pdus):
    """A type-1 block of N1[kind] bits: the PDUs one after another, cut at the block end, random after."""
    n1 = N1[kind]
    b = [v for p in pdus for v in p][:n1]
    b += rng.integers(0, 2, n1 - len(b)).tolist()
    return np.array(b, np.uint8)


# ------------------------------------------------------------------------------ the walk

def _get(t, lo, n):
    assert lo + n <= len(t), "read past the block"
    v = 0
    for b in t[lo:lo + n]:
        v = (v << 1) | (int(b) & 1)
    return v


def _span(length, rem):
    """(bits the PDU takes, malformed, the walk goes on) for length indication L with rem bits left."""
    if 2 <= length <= 34:
        if 8 * length <= rem:
            return 8 * length, 0, True
        if 8 * length - rem < 8:
            return rem, 0, True    # cut at the block end (SCH/F is 33.5 octets)
        return rem, 1, False
    return rem, 0 if length in (62, 63) else 1, False


def parse_sync(t):
    f = {name: _get(t, lo, n) for name, lo, n in SYNC_LAYOUT}
    bad = not (1 <= f["fn"] <= 18 and 1 <= f["mn"] <= 60)
    rec = [SYNC, 0, 60, int(bad), f["system_code"], f["colour_code"], f["tn"], f["fn"], f["mn"], f["sharing_mode"],
           f["ts_reserved_frames"], f["dtx"] | f["frame18_extension"] << 1 | f["late_entry"] << 2, f["mcc"], f["mnc"],
           f["neighbour_cell_broadcast"], f["cell_service_level"]]
    return rec, f


def slot_of(f):
    return ((f["mn"] - 1) * 18 + (f["fn"] - 1)) * 4 + f["tn"]


def parse_pdu(t, off):
    """The PDU at bit off of block t: (record, the walk goes on)."""
    rem = len(t) - off
    pt = _get(t, off, 2)
    rec = [0] * NF
    rec[1], rec[2] = off, rem
    if pt == 0:
        f = {name: _get(t, off + lo, n) for name, lo, n in RESOURCE_LAYOUT}
        rec[4:12] = [f["fill"], f["enc"], f["length"], f["addr_type"], -1, -1, 16,
                     f["grant"] | f["random_access"] << 1]
        if f["addr_type"] == 0:
            rec[0], rec[2] = NULL, 16
            return rec, False
        nbits, bad, more = _span(f["length"], rem)
        has_ssi, auxn = ADDRESS[f["addr_type"]]
        hdr = 16 + 24 * has_ssi + auxn
        if hdr > nbits:
            bad = 1
        else:
            if has_ssi:
                rec[8] = _get(t, off + 16, 24)
            if auxn:
                rec[9] = _get(t, off + hdr - auxn, auxn)
        rec[0], rec[2], rec[3], rec[10] = RESOURCE, nbits, bad, hdr
        return rec, more and not bad
    if pt == 1:
        rec[8] = rec[9] = -1
        rec[4] = _get(t, off + 3, 1)
        if _get(t, off + 2, 1) == 0:
            rec[0], rec[10] = FRAG, 4
            return rec, False
        f = {name: _get(t, off + lo, n) for name, lo, n in END_LAYOUT}
        nbits, bad, more = _span(f["length"], rem)
        rec[0], rec[2], rec[3], rec[6], rec[10], rec[11] = END, nbits, bad, f["length"], 11, f["grant"]
        return rec, more
    if pt == 3:
        rec[0] = SUPPL
        return rec, False
    sub = _get(t, off + 2, 2)
    rec[0] = (SYSINFO, ACCESS_DEFINE, BROADCAST, BROADCAST)[sub]
    if sub == 0:
        if rem < 124:
            rec[3] = 1
        else:
            f = {name: _get(t, off + lo, n) for name, lo, n in SYSINFO_LAYOUT}
            rec[2] = 124
            rec[4:16] = [f["main_carrier"], f["band"], f["offset"], f["duplex_spacing"], f["reverse_operation"],
                         f["num_cscch"], f["ms_txpwr_max_cell"], f["rxlev_access_min"],
                         f["access_parameter"] | f["radio_downlink_timeout"] << 4 | f["optional_field_flag"] << 8,
                         f["hyperframe_cck_flag"] << 16 | f["hyperframe_or_cck"], f["location_area"],
                         f["subscriber_class"] | f["bs_service_details"] << 16]
    return rec, False


def walk(type1, kind):
    """All PDUs of a CRC-good block: [record] (npdu = its length; the library records the first MAXPDU)."""
    t = [int(v) & 1 for v in np.asarray(type1)[:N1[kind]]]
    if kind == 2:
        return [parse_sync(t)[0]]
    recs, off = [], 0
    while len(t) - off >= 16:
        rec, more = parse_pdu(t, off)
        recs.append(rec)
        if not more:
            break
        off += 8 * rec[6]
    return recs


# ------------------------------------------------------------------------------ the timebase

class Tdma:
    """One channel's carried timebase (struct tetra_etsi_tdma)."""

    def __init__(self, bit0=0, anchor_bit=0, anchor_slot=0, locked=0):
        self.bit0, self.anchor_bit, self.anchor_slot, self.locked = int(bit0), int(anchor_bit), int(anchor_slot), int(locked)

    def state(self):
        return (self.bit0, self.anchor_bit, self.anchor_slot, self.locked)

    def predict(self, p):
        """Rule 2 for a burst at stream bit p: the grid's slot or None; drops an expired lock."""
        if not self.locked:
            return None
        d = p - self.anchor_bit
        k = (d + 255) // 510
        if d < 0 or k >= TDMA_EXPIRE:
            self.locked = 0
            return None
        return (self.anchor_slot + k) % TDMA_SLOTS if abs(d - 510 * k) <= TDMA_TOL else None

    def chunk(self, nsym, bursts, own):
        """bursts [(start bit, kind)], own [slot count of the burst's own good SYNC, or None] -> rows."""
        rows = []
        for (start, _), mine in zip(bursts, own):
            p = self.bit0 + int(start)
            was = self.locked
            slot, flags = self.predict(p), 0
            if mine is not None:
                flags = 1 | (2 if was and slot != mine else 0)
                slot, self.locked = mine, 1
            if slot is None:
                rows.append([0, 0, 0, 0])
                continue
            self.anchor_bit, self.anchor_slot = p, slot
            rows.append([slot % 4 + 1, slot // 4 % 18 + 1, slot // 72 + 1, flags])
        self.bit0 += 2 * max(int(nsym) - 1, 0)
        return rows


# ------------------------------------------------------------------------------ one call

def run(nsym, nburst, bursts, nblock, blocks, type1, tdma):
    """tetra_etsi_mac on arrays shaped as the library's: (npdu [C, MAXJ], {(c, j): [record]} (all of a
    block's PDUs), {(c, b): slot row}, tdma after).  tdma: [Tdma] per channel, updated in place."""
    C = len(nsym)
    npdu = np.zeros((C, MAXJ), np.int32)
    recs, rows = {}, {}
    for c in range(C):
        nb, nk = min(max(int(nburst[c]), 0), MAXB), min(max(int(nblock[c]), 0), MAXJ)
        good_sync = {}
        for j in range(nk):
            kind, crc = int(blocks[c, j, 0]), int(blocks[c, j, 1])
            if not crc or kind not in N1:
                continue
            r = walk(type1[c, j], kind)
            recs[(c, j)] = r
            npdu[c, j] = len(r)
            if kind == 2 and r[0][3] == 0:
                good_sync[j] = ((r[0][8] - 1) * 18 + (r[0][7] - 1)) * 4 + r[0][6]
        q, own, bl = 0, [], []
        for b in range(nb):
            kind = int(bursts[c, b, 1])
            own.append(good_sync.get(q) if kind == 2 else None)
            bl.append((int(bursts[c, b, 0]), kind))
            q += 1 if kind == 0 else 2
        for b, row in enumerate(tdma[c].chunk(nsym[c], bl, own)):
            rows[(c, b)] = row
    return npdu, recs, rows


def tdma_array(models):
    a = np.zeros(len(models), TDMA_DTYPE)
    for i, m in enumerate(models):
        a[i] = m.state()
    return a


def assert_equal(out, want, what=""):
    """The library's (npdu, pdus, slots) against run()'s result: npdu everywhere, live records and
    live slot rows exactly."""
    npdu, pdus, slots = out
    wn, recs, rows = want
    assert np.array_equal(npdu, wn), (what, np.argwhere(npdu != wn)[:5].tolist())
    for (c, j), r in recs.items():
        got = pdus[c, j, :min(len(r), MAXPDU)].tolist()
        assert got == r[:MAXPDU], (what, c, j, got, r[:MAXPDU])
    for (c, b), row in rows.items():
        assert slots[c, b].tolist() == row, (what, c, b, slots[c, b].tolist(), row)
