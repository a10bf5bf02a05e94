"""Calls for tetra_etsi_assign (TEST INFRASTRUCTURE): channel allocations written into PDUs by
_etsi_sdu_model's writers, rows shaped by its build_rows, the sdu / done arrays the SDU call would leave
(from the SDU model), and slots / tq rows as the MAC and traffic calls leave them.  The CPU tests hold the
model to each hand-made case's stated outcome; the GPU tests hold the kernels to the model on the same calls.
"""
import numpy as np

import _etsi_mac_model as M
import _etsi_sdu_cases as K
import _etsi_sdu_model as S
import _etsi_assign_model as A

SLOT = K.SLOT
BAND = 4   # the 400 MHz band


def key_of(carrier, off=0, band=BAND):
    """The key of carrier number `carrier` with a frequency offset of `off` keys (-1, 0, 1, 2)."""
    return band * 16000 + 4 * carrier + off


def alloc(carrier, bitmap, updown=1, ext=None, allocation_type=0, mon=3):
    """A channel_allocation dict for _etsi_sdu_model.elements; ext None or (band, offset field)."""
    return dict(allocation_type=allocation_type, timeslot_assigned=bitmap, updownlink_assigned=updown, clch_permission=0,
                cell_change=0, carrier=carrier,
                extended=None if ext is None else dict(band=ext[0], offset=ext[1], duplex_spacing=5, reverse_operation=1),
                monitoring_pattern=mon, frame18_monitoring=2)


def resource_alloc(rng, ca, ssi=0xABCDE1, addr_type=1, aux=0):
    """[a MAC-RESOURCE carrying ca and a short TM-SDU, a null PDU]: a block's PDUs."""
    el = S.elements(M.RESOURCE, None, None, ca)
    has_ssi, auxn = M.ADDRESS[addr_type]
    need = 16 + 24 * has_ssi + auxn + len(el) + 1
    length = (need + 7) // 8 + 1
    return [S.resource_pdu(length, addr_type, K.payload(rng, 8 * length - need), 8 * length, ssi=ssi, aux=aux, fill=1,
                           elems=el), M.null_pdu()]


def end_alloc(rng, ca, bits, n1=268):
    """[a MAC-END carrying ca and the last `bits` of a fragmented TM-SDU, a null PDU]."""
    el = S.elements(M.END, None, None, ca)
    used = 11 + len(el) + len(bits)
    length = max(2, (used + 7) // 8)
    nbits = min(8 * length, n1)
    return [S.end_pdu(length, bits, nbits, fill=int(nbits != used), elems=el), M.null_pdu()]


def grid(p):
    """The slots row of a burst at stream bit p of a carrier whose slot 0 began at bit 0."""
    s = (p + 255) // SLOT
    return [s % 4 + 1, (s // 4) % 18 + 1, (s // 72) % 60 + 1, 0]


def finish(rng, G, row_bits, advance, nsym, arrays, keep, bit0s, frags, maxd=4, slots=None, tq=None, unknown=0.0,
           invalid=0.0):
    """A call's dict from build_rows' arrays: the sdu / done arrays from the SDU model (frags [C / G] S.Frag, updated),
    everything the library does not write poisoned; slots / tq [C][MAXB] lists of rows to use as they are, else
    slots from the grid at the groups' bit0s (a fraction `unknown` reading 0) and tq drawn at random (a fraction
    `invalid` reading -1, a burst not kept NONE, a synchronisation burst NONE, frame 18 CONTROL)."""
    nburst, bursts = arrays[0], arrays[1]
    C = len(nburst)
    recs, ndone, done = S.run(frags, G, row_bits, advance, S.GAP_DEFAULT, maxd, nsym, *arrays, keep=keep)
    sdu, _, done_rec, _ = S.expected_arrays(
        recs, ndone, done, rng.integers(-99, 99, (C, S.MAXJ, S.MAXPDU, S.SDU_FIELDS)).astype(np.int32),
        np.zeros((C, S.MAXJ, S.SDU_ROW), np.uint8), rng.integers(-99, 99, (C // G, max(maxd, 1), S.DONE_FIELDS)).astype(np.int32),
        np.zeros((C // G, max(maxd, 1), S.SDU_MAXBYTES), np.uint8))
    sl = rng.integers(-9, 9, (C, S.MAXB, 4)).astype(np.int32)
    tqa = rng.integers(-9, 9, (C, S.MAXB, 4)).astype(np.int32)
    for c in range(C):
        for b in range(min(max(int(nburst[c]), 0), S.MAXB)):
            if slots is not None:
                sl[c, b] = slots[c][b]
            else:
                p = bit0s[c // G] + (c % G) * row_bits + int(bursts[c, b, 0])
                sl[c, b] = [0, 0, 0, 0] if rng.random() < unknown else grid(p)
            if tq is not None:
                tqa[c, b] = [tq[c][b], 0, 0, 0]
            elif rng.random() < invalid:
                tqa[c, b] = -1
            elif (keep is not None and keep[c, b] == 0) or bursts[c, b, 1] == 2:
                tqa[c, b] = [A.TCH_NONE, 0, 0, 0]
            elif sl[c, b, 1] == 18:
                tqa[c, b] = [A.TCH_CONTROL, 0, 0, 0]
            else:
                cls = int(rng.choice([A.TCH_CONTROL, A.TCH_CONTROL, A.TCH_FULL, A.TCH_FULL, A.TCH_HALF, A.TCH_LOST]))
                tqa[c, b] = [cls, 432 if cls == A.TCH_FULL else 216 if cls == A.TCH_HALF else 0, 1000, 0]
    return dict(G=G, row_bits=row_bits, advance=advance, nsym=nsym, arrays=arrays, keep=keep, slots=sl, tq=tqa, sdu=sdu,
                maxd=maxd, ndone=ndone, done=done_rec)


def rows_call(rng, rows, bit0s=None, frags=None, nsym=4 * 72 * SLOT // 2 + 1, maxd=4):
    """A streaming call (G = 1, keep NULL) of one row per carrier.  rows: per row a list of bursts (start bit,
    burst kind, [block], tq CLASS, (TN, FN)): the slots and tq rows are the given ones."""
    C = len(rows)
    arrays = S.build_rows(rng, [[r[:3] for r in row] for row in rows])
    pad = lambda row, f: [f(r) for r in row] + [None] * (S.MAXB - len(row))
    return finish(rng, 1, 0, 0, np.full(C, nsym, np.int32), arrays, None, bit0s or [0] * C,
                  frags or [S.Frag(b) for b in (bit0s or [0] * C)], maxd,
                  slots=[pad(row, lambda r: [r[4][0], r[4][1], 1, 0]) for row in rows],
                  tq=[pad(row, lambda r: r[3]) for row in rows])


def run_model(call, states, row_key, hold_slots=A.HOLD_DEFAULT, idle_max=A.IDLE_DEFAULT, shared_clock=0, maxe=8,
              with_tq=True, with_slots=True):
    """The model on a call's dict: (nev, ev, ta) of _etsi_assign_model.run."""
    a = call["arrays"]
    return A.run(states, call["G"], call["row_bits"], call["advance"], hold_slots, idle_max, shared_clock, call["nsym"],
                 a[0], a[1], a[2], a[3], a[5], a[6], call["keep"], call["slots"] if with_slots else None,
                 call["tq"] if with_tq else None, call["sdu"], call["maxd"], call["ndone"], call["done"], row_key, maxe)


# ------------------------------------------------------------------------------ a seeded sweep

class planting:
    """While entered, _etsi_sdu_cases.random_pdus -- what random_call draws a block's PDUs from -- returns, for a
    fraction `share` of the blocks that have room, a MAC-RESOURCE (one in eight: a MAC-END, which no chain
    awaits) whose channel allocation names one of `carriers`, half of them by the extended numbering with
    `ext` = (band, offset field); up/downlink, the bitmap and the address type vary."""

    def __init__(self, carriers, ext, share=0.35):
        self.carriers, self.ext, self.share = list(carriers), ext, share

    def pdus(self, rng, n1):
        if n1 < 124 or rng.random() >= self.share:
            return self.plain(rng, n1)
        ca = alloc(int(rng.choice(self.carriers)), int(rng.choice([0, 1, 2, 4, 8, 8, 4, 2, 1, 3, 12, 15])),
                   int(rng.choice([1, 1, 1, 3, 3, 2])), self.ext if rng.random() < 0.5 else None,
                   int(rng.integers(4)), int(rng.integers(4)))
        if rng.random() < 0.125:
            return end_alloc(rng, ca, K.payload(rng, int(rng.integers(0, 40))), n1)
        at = int(rng.choice([1, 1, 3, 5, 6]))
        return resource_alloc(rng, ca, int(rng.integers(1 << 24)), at, int(rng.integers(1 << M.ADDRESS[at][1]))
                              if M.ADDRESS[at][1] else 0)

    def __enter__(self):
        self.plain, K.random_pdus = K.random_pdus, self.pdus
        return self

    def __exit__(self, *exc):
        K.random_pdus = self.plain


def group_keys(rng, NG, off):
    """Keys for NG groups: carrier numbers 100 + g with a frequency offset of `off` keys; of three groups or
    more one is unknown (-1) and one lies on another offset.  Returns (keys int32, the carrier numbers to name)."""
    keys = np.array([key_of(100 + g, off) for g in range(NG)], np.int32)
    if NG >= 3:
        keys[int(rng.integers(NG))] = -1
        g = int(rng.integers(NG))
        if keys[g] >= 0:
            keys[g] = key_of(100 + g, (off + 2) % 4 - 1)
    return keys, [100 + g for g in range(NG)] + [99]


def random_stream(seed, C, G, ncalls=1, row_bits=4 * SLOT, off=None):
    """ncalls successive random calls (_etsi_sdu_cases.random_call, allocations planted) of C rows in groups of G
    on one clock: (calls, keys).  The groups' streams start at bit 0 and advance alike."""
    rng = np.random.default_rng(seed)
    NG = C // G
    off = int(rng.choice([0, 1, 2, -1])) if off is None else off
    keys, carriers = group_keys(rng, NG, off)
    ext = (BAND, {0: 0, 1: 1, -1: 2, 2: 3}[off])
    advance = 8 * SLOT if G == 1 else G * row_bits
    frags, calls = [S.Frag(0) for _ in range(NG)], []
    for n in range(ncalls):
        with planting(carriers, ext):
            arrays, keep = K.random_call(rng, C, G, row_bits)
        calls.append(finish(rng, G, 0 if G == 1 else row_bits, advance, np.full(C, advance // 2 + 1, np.int32), arrays, keep,
                            [n * advance] * NG, frags, unknown=0.1, invalid=0.03))
    return calls, keys
