"""CPU model of tetra_etsi_sdu (TEST INFRASTRUCTURE): the TM-SDU extent of a PDU record (Part A), the
fragment walk with carried state (Part B), and two test-side writers.

The reader restates include/tetra_hip.h's description in plain Python on lists of bits, driven by the
tables below; a chain holds a list of bits, not bytes, so that it shares no shape with k_sdu_join's
byte funnel.  The writers (elements / resource_pdu / end_pdu / frag_pdu / fragment) go forwards from
the same layout as DESIGN.md §5.24 prints it -- fields in, bits out -- and share no code with the
reader.  Bit 0 is the first type-1 bit of the block, fields are MSB first, a bit is byte & 1.
"""
import numpy as np

import _etsi_mac_model as M

MAXB, MAXJ, MAXPDU, NF = M.MAXB, M.MAXJ, M.MAXPDU, M.NF
SDU_FIELDS, SDU_ROW, SDU_MAXBYTES, FRAG_CHAINS, DONE_FIELDS = 8, 40, 512, 4, 13
TDMA_TOL, GAP_DEFAULT = M.TDMA_TOL, M.TDMA_EXPIRE
OK, NONE, MALFORMED, ENCRYPTED, UNSUPPORTED = range(5)
WHOLE, FIRST, MIDDLE, LAST = range(4)
STATUS, OFFSET, NBITS, BYTE, ROLE, ELEMS, POWER_GRANT, CHAN = range(8)
(D_ROW, D_BURST, D_BLOCK, D_PDU, D_SSI, D_ADDR_TYPE, D_AUX, D_ENC, D_NBITS, D_NFRAG, D_SPAN, D_FED,
 D_GAPS) = range(13)
CHAIN_DTYPE = np.dtype([("last_bit", "<i8"), ("active", "<i4"), ("ssi", "<i4"), ("addr_type", "<i4"), ("aux", "<i4"),
                        ("enc", "<i4"), ("nbits", "<i4"), ("nfrag", "<i4"), ("span", "<i4"), ("fed", "<i4"),
                        ("reserved", "<i4"), ("data", "u1", (SDU_MAXBYTES,))])
FRAG_DTYPE = np.dtype([("bit0", "<i8"), ("dropped", "<i4"), ("orphans", "<i4"), ("chain", CHAIN_DTYPE, (FRAG_CHAINS,))])

# ------------------------------------------------------------------------------ the reader's tables
# An element: a presence flag of 1 bit, then its groups.  A group is read whole or not at all:
# (condition on the fields read so far, ((field, width), ...)).
CHANNEL_ALLOCATION = (
    (None, (("allocation_type", 2), ("timeslot_assigned", 4), ("updownlink_assigned", 2), ("clch_permission", 1),
            ("cell_change", 1))),
    (None, (("carrier", 12),)),
    (None, (("extended_flag", 1),)),
    (lambda f: f["extended_flag"] == 1, (("band", 4), ("offset", 2), ("duplex_spacing", 3), ("reverse_operation", 1))),
    (None, (("monitoring_pattern", 2),)),
    (lambda f: f["monitoring_pattern"] == 0, (("frame18_monitoring", 2),)),
)
ELEMENT_GROUPS = {"power_control": ((None, (("power_control", 4),)),),
                  "slot_granting": ((None, (("slot_granting", 8),)),),
                  "channel_allocation": CHANNEL_ALLOCATION}
ELEMENTS = {M.RESOURCE: ("power_control", "slot_granting", "channel_allocation"),
            M.END: ("slot_granting", "channel_allocation"), M.FRAG: ()}
ROLE_OF = {M.FRAG: MIDDLE, M.END: LAST}


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def _elements(t, kind, pos, end):
    """Walk the optional elements of a PDU of `kind` in t[pos:end]: (fields, new pos, status)."""
    f = {}
    try:
        for name in ELEMENTS[kind]:
            if pos + 1 > end:
                raise _Stop(MALFORMED)
            flag = t[pos]
            pos += 1
            if not flag:
                continue
            for cond, group in ELEMENT_GROUPS[name]:
                if cond is not None and not cond(f):
                    continue
                if pos + sum(n for _, n in group) > end:
                    raise _Stop(MALFORMED)
                for fname, n in group:
                    f[fname] = M._get(t, pos, n)
                    pos += n
                if f.get("updownlink_assigned") == 0:
                    raise _Stop(UNSUPPORTED)   # the augmented form is not walked
    except _Stop as s:
        return f, pos, s.status
    return f, pos, OK


def _raw(f):
    """ELEMS, POWER_GRANT, CHAN of the fields read."""
    elems = (1 if "power_control" in f else 0) | (2 if "slot_granting" in f else 0) | \
        (4 if "cell_change" in f else 0) | (8 if "reverse_operation" in f else 0)
    pg = f.get("power_control", 0) | f.get("slot_granting", 0) << 8
    if "reverse_operation" in f:
        pg |= (f["band"] << 6 | f["offset"] << 4 | f["duplex_spacing"] << 1 | f["reverse_operation"]) << 16
    chan = 0
    if "cell_change" in f:
        chan = (f["allocation_type"] << 8 | f["timeslot_assigned"] << 4 | f["updownlink_assigned"] << 2 |
                f["clch_permission"] << 1 | f["cell_change"])
    chan |= f.get("frame18_monitoring", 0) << 10 | f.get("carrier", 0) << 16 | f.get("monitoring_pattern", 0) << 28
    return elems, pg, chan


def sdu_of(t, rec):
    """Part A for one PDU record of block t (a list of n1 bits): ([STATUS .. CHAN] without BYTE set, SDU bits)."""
    kind, off, nbits, pstatus, fill, enc, length, hdr = (int(rec[i]) for i in (0, 1, 2, 3, 4, 5, 6, 10))
    role = (FIRST if length == 63 else WHOLE) if kind == M.RESOURCE else ROLE_OF.get(kind, WHOLE)
    out = [NONE, 0, 0, 0, role, 0, 0, 0]
    if kind not in ELEMENTS or pstatus != 0:
        return out, []
    if off < 0 or nbits < 0 or off + nbits > len(t) or hdr < 0 or hdr > nbits:
        out[STATUS] = MALFORMED
        return out, []
    end = off + nbits
    if kind == M.RESOURCE and enc != 0:
        out[STATUS], out[OFFSET], out[NBITS] = ENCRYPTED, off + hdr, nbits - hdr
        return out, t[off + hdr:end]
    f, pos, status = _elements(t, kind, off + hdr, end)
    out[ELEMS], out[POWER_GRANT], out[CHAN] = _raw(f)
    if status == OK and fill:
        ones = [i for i in range(pos, end) if t[i]]
        if ones:
            end = ones[-1]
        else:
            status = MALFORMED
    out[STATUS] = status
    if status != OK:
        return out, []
    out[OFFSET], out[NBITS] = pos, end - pos
    return out, t[pos:end]


def pack(bits):
    """MSB-first bytes of a bit list, the last byte zero-padded."""
    b = list(bits) + [0] * (-len(bits) % 8)
    return bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))


def unpack(data, nbits):
    return [(data[i >> 3] >> (7 - (i & 7))) & 1 for i in range(nbits)]


def part_a(nblock, blocks, type1, npdu, pdus):
    """{(c, j): [(record with BYTE, SDU bits)]} for every block the library writes records for."""
    out = {}
    for c in range(len(nblock)):
        for j in range(min(max(int(nblock[c]), 0), MAXJ)):
            kind, crc = int(blocks[c, j, 0]), int(blocks[c, j, 1])
            n = min(max(int(npdu[c, j]), 0), MAXPDU) if crc and kind in M.N1 else 0
            if n == 0:
                continue
            t = [int(v) & 1 for v in type1[c, j, :M.N1[kind]]]
            recs, at = [], 0
            for q in range(n):
                rec, bits = sdu_of(t, pdus[c, j, q])
                if at + (len(bits) + 7) // 8 > SDU_ROW:
                    rec[STATUS], rec[OFFSET], rec[NBITS], bits = MALFORMED, 0, 0, []
                rec[BYTE] = at
                at += (len(bits) + 7) // 8
                recs.append((rec, bits))
            out[(c, j)] = recs
    return out


# ------------------------------------------------------------------------------ Part B

class Chain:
    def __init__(self):
        self.active, self.last_bit, self.ssi, self.addr_type, self.aux, self.enc = 0, 0, 0, 0, 0, 0
        self.nfrag, self.span, self.fed, self.bits = 0, 0, 0, []


class Frag:
    """One carrier's carried fragment state (struct tetra_etsi_frag)."""

    def __init__(self, bit0=0):
        self.bit0, self.dropped, self.orphans = int(bit0), 0, 0
        self.chains = [Chain() for _ in range(FRAG_CHAINS)]

    def _k(self, ch, p):
        d = p - ch.last_bit
        k = (d + 255) // 510   # Python's floor division
        return d, k

    def _same(self, p):
        out = []
        for ch in self.chains:
            d, k = self._k(ch, p)
            if ch.active and k >= 0 and k % 4 == 0 and abs(d - 510 * k) <= TDMA_TOL:
                out.append(ch)
        return out

    def expire(self, p, gap_slots):
        for ch in self.chains:
            if ch.active and self._k(ch, p)[1] > gap_slots:
                ch.active = 0
                self.dropped += 1

    def record(self, p, rec, bits, pdu):
        """One Part A record of a burst at stream bit p; returns the finished chain on a completion."""
        role, status = rec[ROLE], rec[STATUS]
        if role == WHOLE:
            return None
        if role == FIRST:
            if status != OK:
                return None
            for ch in self._same(p):
                ch.active = 0
                self.dropped += 1
            free = [ch for ch in self.chains if not ch.active]
            if free:
                ch = free[0]
            else:
                ch = min(self.chains, key=lambda x: x.last_bit)   # the first among equals
                self.dropped += 1
            ch.active, ch.last_bit, ch.bits = 1, p, list(bits)
            ch.ssi, ch.addr_type, ch.aux, ch.enc = int(pdu[8]), int(pdu[7]), int(pdu[9]), int(pdu[5])
            ch.nfrag, ch.span, ch.fed = 1, 0, 1
            return None
        same = self._same(p)
        if status != OK or not same:
            self.orphans += 1
            return None
        ch = same[0]
        if len(ch.bits) + len(bits) > 8 * SDU_MAXBYTES:
            ch.active = 0
            self.dropped += 1
            return None
        k = self._k(ch, p)[1]
        ch.bits += list(bits)
        ch.nfrag, ch.span, ch.fed, ch.last_bit = ch.nfrag + 1, ch.span + k, ch.fed + (k > 0), p
        if role == LAST:
            ch.active = 0
            return ch
        return None

    def to_array(self):
        a = np.zeros((), FRAG_DTYPE)
        a["bit0"], a["dropped"], a["orphans"] = self.bit0, self.dropped, self.orphans
        for i, ch in enumerate(self.chains):
            c = a["chain"][i]
            for name in ("last_bit", "active", "ssi", "addr_type", "aux", "enc", "nfrag", "span", "fed"):
                c[name] = getattr(ch, name)
            c["nbits"] = len(ch.bits)
            d = pack(ch.bits)
            c["data"][:len(d)] = np.frombuffer(d, np.uint8)
        return a


def join(frags, G, row_bits, advance, gap_slots, maxd, nsym, nburst, bursts, nblock, blocks, recs, pdus, keep=None):
    """Part B over every group: frags [C / G] Frag, updated in place; recs = part_a(...).
    Returns (ndone [C / G], {(g, i): ([13 fields], bytes)} for the first maxd completions of group g)."""
    C = len(nburst)
    ndone, done = np.zeros(C // G, np.int32), {}
    streaming = G == 1 and row_bits == 0 and keep is None
    for g in range(C // G):
        fr = frags[g]
        entries = []
        for i in range(G):
            c = g * G + i
            for b in range(min(max(int(nburst[c]), 0), MAXB)):
                entries.append((i * row_bits + int(bursts[c, b, 0]), i, b))
        for pos, i, b in sorted(entries):
            c = g * G + i
            if keep is not None and keep[c, b] == 0:
                continue
            p = fr.bit0 + pos
            fr.expire(p, gap_slots)
            for j in range(min(max(int(nblock[c]), 0), MAXJ)):
                if int(blocks[c, j, 2]) != b or (c, j) not in recs:
                    continue
                for q, (rec, bits) in enumerate(recs[(c, j)]):
                    ch = fr.record(p, rec, bits, pdus[c, j, q])
                    if ch is not None:
                        if ndone[g] < maxd:
                            done[(g, int(ndone[g]))] = (
                                [c, b, j, q, ch.ssi, ch.addr_type, ch.aux, ch.enc, len(ch.bits), ch.nfrag, ch.span,
                                 ch.fed, ch.span // 4 + 1 - ch.fed], pack(ch.bits))
                        ndone[g] += 1
        fr.bit0 += 2 * max(int(nsym[g]) - 1, 0) if streaming else advance
    return ndone, done


def run(frags, G, row_bits, advance, gap_slots, maxd, nsym, nburst, bursts, nblock, blocks, type1, npdu, pdus,
        keep=None):
    """One tetra_etsi_sdu call: (recs, ndone, done)."""
    recs = part_a(nblock, blocks, type1, npdu, pdus)
    ndone, done = join(frags, G, row_bits, advance, gap_slots, maxd, nsym, nburst, bursts, nblock, blocks, recs, pdus, keep)
    return recs, ndone, done


def expected_arrays(recs, ndone, done, sdu, sdu_data, done_rec, done_data):
    """Write what the library writes into copies of the caller's (poisoned) output arrays."""
    sdu, sdu_data, done_rec, done_data = sdu.copy(), sdu_data.copy(), done_rec.copy(), done_data.copy()
    for (c, j), rs in recs.items():
        for q, (rec, bits) in enumerate(rs):
            sdu[c, j, q] = rec
            d = pack(bits)
            sdu_data[c, j, rec[BYTE]:rec[BYTE] + len(d)] = np.frombuffer(d, np.uint8)
    for (g, i), (f, d) in done.items():
        done_rec[g, i] = f
        done_data[g, i, :len(d)] = np.frombuffer(d, np.uint8)
    return sdu, sdu_data, done_rec, done_data


def assert_frag_equal(got, frags, what=""):
    """The library's frag array against the model's states: the heads, and of an active chain every field
    and its bytes (a freed chain's other fields are whatever it held)."""
    for g, fr in enumerate(frags):
        want = fr.to_array()
        for name in ("bit0", "dropped", "orphans"):
            assert got[g][name] == want[name], (what, g, name, int(got[g][name]), int(want[name]))
        for i in range(FRAG_CHAINS):
            a, b = got[g]["chain"][i], want["chain"][i]
            assert bool(a["active"]) == bool(b["active"]), (what, g, i, "active")
            if b["active"]:
                for name in ("last_bit", "ssi", "addr_type", "aux", "enc", "nbits", "nfrag", "span", "fed"):
                    assert a[name] == b[name], (what, g, i, name, int(a[name]), int(b[name]))
                n = (int(b["nbits"]) + 7) // 8
                assert bytes(a["data"][:n]) == bytes(b["data"][:n]), (what, g, i, "data")


# ------------------------------------------------------------------------------ the writers
# Written forwards from the layout tables of DESIGN.md §5.24; nothing above is used but bits_of and the
# header layouts of _etsi_mac_model's own builders.

def elements(kind, power_control=None, slot_granting=None, channel_allocation=None):
    """The optional-element bits of a MAC-RESOURCE (kind 0) or MAC-END (kind 2).  channel_allocation:
    dict(allocation_type, timeslot_assigned, updownlink_assigned, clch_permission, cell_change, carrier,
    extended=None or dict(band, offset, duplex_spacing, reverse_operation), monitoring_pattern,
    frame18_monitoring); an augmented one (updownlink_assigned 0) stops after its first ten bits."""
    b = []
    if kind == M.RESOURCE:
        b += [0] if power_control is None else [1] + M.bits_of(power_control, 4)
    else:
        assert power_control is None
    b += [0] if slot_granting is None else [1] + M.bits_of(slot_granting, 8)
    if channel_allocation is None:
        return b + [0]
    ca = channel_allocation
    b += [1] + M.bits_of(ca["allocation_type"], 2) + M.bits_of(ca["timeslot_assigned"], 4)
    b += M.bits_of(ca["updownlink_assigned"], 2) + [ca["clch_permission"], ca["cell_change"]]
    if ca["updownlink_assigned"] == 0:
        return b
    b += M.bits_of(ca["carrier"], 12)
    ext = ca.get("extended")
    if ext is None:
        b += [0]
    else:
        b += [1] + M.bits_of(ext["band"], 4) + M.bits_of(ext["offset"], 2) + M.bits_of(ext["duplex_spacing"], 3)
        b += [ext["reverse_operation"]]
    b += M.bits_of(ca["monitoring_pattern"], 2)
    if ca["monitoring_pattern"] == 0:
        b += M.bits_of(ca["frame18_monitoring"], 2)
    return b


def _finish(head, sdu_bits, fill, nbits):
    """head + SDU (+ fill bits: a 1, then 0s) cut or checked against nbits."""
    b = list(head) + list(sdu_bits)
    if fill:
        assert len(b) < nbits, "no room for the fill bits"
        b += [1] + [0] * (nbits - len(b) - 1)
    assert len(b) == nbits, (len(b), nbits)
    return b


def resource_pdu(length, addr_type, sdu_bits, nbits, ssi=0, aux=0, fill=0, enc=0, grant=0, random_access=0, elems=None):
    """A MAC-RESOURCE of nbits bits; elems: elements(0, ...) bits, default the three absent flags."""
    hdr = [0] * 16
    M._lay(hdr, M.RESOURCE_LAYOUT, dict(fill=fill, grant=grant, enc=enc, random_access=random_access, length=length,
                                       addr_type=addr_type))
    has_ssi, auxn = M.ADDRESS[addr_type]
    hdr += (M.bits_of(ssi, 24) if has_ssi else []) + (M.bits_of(aux, auxn) if auxn else [])
    return _finish(hdr + (elements(M.RESOURCE) if elems is None else list(elems)), sdu_bits, fill, nbits)


def end_pdu(length, sdu_bits, nbits, fill=0, grant=0, elems=None):
    hdr = [0, 1, 1] + [0] * 8
    M._lay(hdr, M.END_LAYOUT, dict(fill=fill, grant=grant, length=length))
    return _finish(hdr + (elements(M.END) if elems is None else list(elems)), sdu_bits, fill, nbits)


def frag_pdu(sdu_bits, nbits, fill=0):
    return _finish([0, 1, 0, fill], sdu_bits, fill, nbits)


def fragment(sdu_bits, kinds, addr_type=1, ssi=0x123456, aux=0):
    """Cut a TM-SDU into one PDU per block of `kinds` (0 SCH/F, 1 SCH/HD): MAC-RESOURCE (L = 63), MAC-FRAG
    ..., MAC-END.  All but the last are full; the MAC-END takes the rest, with fill bits up to its octet
    length L (cut at the block end).  Returns the PDUs' bit lists; the MAC-END may be shorter than its block."""
    assert len(kinds) >= 2
    sdu_bits, out, at = list(sdu_bits), [], 0
    has_ssi, auxn = M.ADDRESS[addr_type]
    for i, kind in enumerate(kinds):
        n1 = M.N1[kind]
        if i == 0:
            cap = n1 - 16 - 24 * has_ssi - auxn - 3
            out.append(resource_pdu(63, addr_type, sdu_bits[at:at + cap], n1, ssi=ssi, aux=aux))
        elif i < len(kinds) - 1:
            cap = n1 - 4
            out.append(frag_pdu(sdu_bits[at:at + cap], n1))
        else:
            rest = sdu_bits[at:]
            used = 11 + 2 + len(rest)
            assert used <= n1, "the last block cannot take the rest"
            length = max(2, (used + 7) // 8)
            nbits = min(8 * length, n1)
            out.append(end_pdu(length, rest, nbits, fill=int(nbits != used)))
            cap = len(rest)
        assert at + cap <= len(sdu_bits) or i == len(kinds) - 1, "the SDU is too short for these blocks"
        at += cap
    return out


def capacity(kinds, addr_type=1):
    """(fewest, most) TM-SDU bits fragment() can cut into blocks of `kinds`."""
    has_ssi, auxn = M.ADDRESS[addr_type]
    fixed = M.N1[kinds[0]] - 16 - 24 * has_ssi - auxn - 3 + sum(M.N1[k] - 4 for k in kinds[1:-1])
    return fixed, fixed + M.N1[kinds[-1]] - 13


# ------------------------------------------------------------------------------ rows for a call

BLOCKS_OF = {0: (0,), 1: (1, 1), 2: (2, 1)}   # burst kind -> its blocks' kinds


def build_rows(rng, rows):
    """rows: per row a list of bursts (start bit, burst kind, [block]) with block = None (CRC-bad, random
    bits) or a list of PDU bit lists (CRC-good).  Returns the library-shaped arrays (nburst, bursts, nblock,
    blocks, type1, npdu, pdus) with npdu / pdus from _etsi_mac_model's walk, as tetra_etsi_mac leaves them,
    and everything past the counts and past a block's bits poisoned."""
    C = len(rows)
    nburst, nblock = np.zeros(C, np.int32), np.zeros(C, np.int32)
    bursts = rng.integers(-9999, 9999, (C, MAXB, 2)).astype(np.int32)
    blocks = rng.integers(-9, 9, (C, MAXJ, 4)).astype(np.int32)
    type1 = rng.integers(0, 256, (C, MAXJ, 268)).astype(np.uint8)
    npdu = np.zeros((C, MAXJ), np.int32)
    pdus = rng.integers(-9999, 9999, (C, MAXJ, MAXPDU, NF)).astype(np.int32)
    for c, row in enumerate(rows):
        j = 0
        for b, (start, bkind, blks) in enumerate(row):
            bursts[c, b] = (start, bkind)
            for idx, (kind, content) in enumerate(zip(BLOCKS_OF[bkind], blks)):
                blocks[c, j] = (kind, 0 if content is None else 1, b, idx)
                if content is not None:
                    bits = M.block(rng, kind, content) if kind != 2 else np.array(content[0], np.uint8)
                    # only bit 0 of a type-1 byte counts: the other bits are poison
                    type1[c, j, :M.N1[kind]] = bits | (rng.integers(0, 128, M.N1[kind]).astype(np.uint8) << 1)
                    recs = M.walk(bits, kind)
                    npdu[c, j] = len(recs)
                    for q, r in enumerate(recs[:MAXPDU]):
                        pdus[c, j, q] = r
                j += 1
        nburst[c], nblock[c] = len(row), j
    return nburst, bursts, nblock, blocks, type1, npdu, pdus
