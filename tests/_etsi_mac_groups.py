"""CPU model of tetra_etsi_mac_groups (TEST INFRASTRUCTURE): the merge of a carrier's overlapping chunk
rows and one TDMA timebase per carrier over the merged order, restated from include/tetra_hip.h in
plain Python on top of _etsi_mac_model's PDU walk.  Rows g G .. g G + G - 1 belong to group g.
"""
import numpy as np

import _etsi_mac_model as M

MAXG = 64


class GroupTdma:
    """One group's carried timebase (struct tetra_etsi_tdma) under the group rule: a burst behind the
    anchor keeps the lock, and only a burst at least a slot ahead (or an own SYNC) moves the anchor."""

    def __init__(self, bit0=0, anchor_bit=0, anchor_slot=0, locked=0):
        self.bit0, self.anchor_bit, self.anchor_slot, self.locked = int(bit0), int(anchor_bit), int(anchor_slot), int(locked)

    def state(self):
        return (self.bit0, self.anchor_bit, self.anchor_slot, self.locked)

    def predict(self, p):
        """(slot or None, k) for a burst at stream bit p; drops a lock that expired."""
        if not self.locked:
            return None, 0
        d = p - self.anchor_bit
        k = (d + 255) // 510          # Python's // floors toward minus infinity
        if k >= M.TDMA_EXPIRE:
            self.locked = 0
            return None, k
        if k <= -M.TDMA_EXPIRE or abs(d - 510 * k) > M.TDMA_TOL:
            return None, k
        return (self.anchor_slot + k) % M.TDMA_SLOTS, k

    def burst(self, pos, mine):
        """One burst at group position pos with own-SYNC slot count `mine` (or None) -> slot row."""
        p = self.bit0 + int(pos)
        was = self.locked
        slot, k = self.predict(p)
        flags = 0
        if mine is not None:
            flags = 1 | (2 if was and slot != mine else 0)
            slot, self.locked = mine, 1
            self.anchor_bit, self.anchor_slot = p, slot
        elif slot is not None and k >= 1:
            self.anchor_bit, self.anchor_slot = p, slot
        if slot is None:
            return [0, 0, 0, 0]
        return [slot % 4 + 1, slot // 4 % 18 + 1, slot // 72 + 1, flags]


def merged_order(nburst, bursts, c0, G, row_bits):
    """[(pos, row, b)] of group rows c0 .. c0 + G - 1, ordered."""
    live = []
    for i in range(G):
        for b in range(min(max(int(nburst[c0 + i]), 0), M.MAXB)):
            live.append((i * int(row_bits) + int(bursts[c0 + i, b, 0]), i, b))
    return sorted(live)


def run(G, row_bits, tol_bits, advance, nburst, bursts, nblock, blocks, type1, tdma):
    """tetra_etsi_mac_groups on arrays shaped as the library's: (npdu [C, MAXJ], {(c, j): [record]},
    {(c, b): slot row}, {(c, b): keep}).  tdma: [GroupTdma] per group, updated in place."""
    C = len(nburst)
    assert 1 <= G <= MAXG and C % G == 0 and row_bits >= 0 and tol_bits >= 0
    npdu = np.zeros((C, M.MAXJ), np.int32)
    recs, rows, keep, own = {}, {}, {}, {}
    for c in range(C):
        nb, nk = min(max(int(nburst[c]), 0), M.MAXB), min(max(int(nblock[c]), 0), M.MAXJ)
        good_sync = {}
        for j in range(nk):
            kind, crc = int(blocks[c, j, 0]), int(blocks[c, j, 1])
            if not crc or kind not in M.N1:
                continue
            r = M.walk(type1[c, j], kind)
            recs[(c, j)] = r
            npdu[c, j] = len(r)
            if kind == 2 and r[0][3] == 0:
                good_sync[j] = M.slot_of(dict(tn=r[0][6], fn=r[0][7], mn=r[0][8]))
        q = 0
        for b in range(nb):
            kind = int(bursts[c, b, 1])
            own[(c, b)] = good_sync.get(q) if kind == 2 else None
            q += 1 if kind == 0 else 2
    for g in range(C // G):
        prev = None
        for pos, i, b in merged_order(nburst, bursts, g * G, G, row_bits):
            c = g * G + i
            keep[(c, b)] = int(prev is None or pos - prev > tol_bits)
            prev = pos
            rows[(c, b)] = tdma[g].burst(pos, own[(c, b)])
        tdma[g].bit0 += int(advance)
    return npdu, recs, rows, keep


def assert_equal(out, want, what=""):
    """The library's (npdu, pdus, slots, keep) against run()'s result, live entries exactly."""
    npdu, pdus, slots, keep = out
    M.assert_equal((npdu, pdus, slots), want[:3], what)
    for (c, b), v in want[3].items():
        assert int(keep[c, b]) == v, (what, "keep", c, b, int(keep[c, b]), v)


# ------------------------------------------------------------------------------ hand-made inputs

POISON_KIND, POISON_BYTE, UNWRITTEN = 99, 0x7e, -77


def arrays_of(rng, rows):
    """rows [C][(start bit, burst kind, sync)] -> (nburst, bursts, nblock, blocks, type1), poisoned past
    every count and past a block's n1.  sync (SBs only): None, or dict(slot=, crc=1, **SYNC fields to
    override); only a BSCH block can be CRC-good here, so no other block is walked."""
    C = len(rows)
    nburst, nblock = np.zeros(C, np.int32), np.zeros(C, np.int32)
    bursts = np.full((C, M.MAXB, 2), POISON_KIND, np.int32)
    blocks = np.full((C, M.MAXJ, 4), POISON_KIND, np.int32)
    type1 = np.full((C, M.MAXJ, 268), POISON_BYTE, np.uint8)
    for c, row in enumerate(rows):
        j = 0
        for b, (start, kind, sy) in enumerate(row):
            bursts[c, b] = (start, kind)
            for i, bk in enumerate(((0,), (1, 1), (2, 1))[kind]):
                good = bk == 2 and sy is not None
                blocks[c, j] = (bk, int(good and sy.get("crc", 1)), b, i)
                if good:
                    over = {k: v for k, v in sy.items() if k not in ("slot", "crc")}
                    t = M.block(rng, 2, [M.sync(M.sync_for_slot(rng, sy["slot"], **over))])
                    type1[c, j, :60] = t | (rng.integers(0, 128, 60).astype(np.uint8) << 1)   # a bit is byte & 1
                j += 1
        nburst[c], nblock[c] = len(row), j
    return nburst, bursts, nblock, blocks, type1


def _sb(slot, **kw):
    return dict(slot=slot, **kw)


def hand_cases():
    """[dict(name, G, row_bits, tol, state, calls)]: one group each; a call is dict(advance, rows [G]
    [(start, kind, sync)], slots {(row, b): [tn, fn, mn, flags]}, keep {(row, b): 0 / 1}, state after).
    Every expected value is written out by hand from the rule in include/tetra_hip.h."""
    Z, LOCK = [0, 0, 0, 0], (0, 1000, 10, 1)
    out = []
    # three rows 1966 bits apart, each 2506 bits long; bursts at group bits 440 + 510 n; the copies in
    # the overlaps [1966, 2506) and [3932, 4472) sit -2, 0 and +2 bits off; the SB (slot 100) is n = 5
    out.append(dict(name="three rows, SB in row 1", G=3, row_bits=1966, tol=32, state=(0, 0, 0, 0), calls=[dict(
        advance=5898,
        rows=[[(440, 0, None), (950, 1, None), (1460, 0, None), (1970, 0, None), (2480, 1, None)],
              [(2, 0, None), (514, 1, None), (1024, 2, _sb(100)), (1534, 0, None), (2044, 1, None)],
              [(80, 1, None), (588, 0, None), (1098, 0, None)]],
        slots={(0, 0): Z, (0, 1): Z, (0, 2): Z, (0, 3): Z, (0, 4): Z, (1, 0): Z, (1, 1): Z,
               (1, 2): [1, 8, 2, 1], (1, 3): [2, 8, 2, 0], (1, 4): [3, 8, 2, 0],
               (2, 0): [3, 8, 2, 0], (2, 1): [4, 8, 2, 0], (2, 2): [1, 9, 2, 0]},
        keep={(0, 0): 1, (0, 1): 1, (0, 2): 1, (0, 3): 0, (0, 4): 1, (1, 0): 1, (1, 1): 0, (1, 2): 1, (1, 3): 1,
              (1, 4): 1, (2, 0): 0, (2, 1): 1, (2, 2): 1},
        state=(5898, 3932 + 1098, 104, 1))]))
    # the SB at group bit 2000 and its copy at 2001: both own-SYNC, FLAGS bit 1 clear; 4319 -> 0
    out.append(dict(name="the SB in the overlap", G=2, row_bits=1966, tol=32, state=(0, 0, 0, 0), calls=[dict(
        advance=3932,
        rows=[[(2000, 2, _sb(4319))], [(35, 2, _sb(4319)), (544, 0, None)]],
        slots={(0, 0): [4, 18, 60, 1], (1, 0): [4, 18, 60, 1], (1, 1): [1, 1, 1, 0]},
        keep={(0, 0): 1, (1, 0): 0, (1, 1): 1},
        state=(3932, 2510, 0, 1))]))
    # a stream: the second buffer starts 2000 bits on, inside the first one's span; its first two
    # bursts are the first buffer's last two, decoded again (one a bit late)
    out.append(dict(name="a carried tail", G=2, row_bits=1966, tol=32, state=(0, 0, 0, 0), calls=[
        dict(advance=2000,
             rows=[[(300, 2, _sb(10)), (810, 0, None), (1320, 1, None), (1830, 0, None)], [(374, 0, None), (884, 1, None)]],
             slots={(0, 0): [3, 3, 1, 1], (0, 1): [4, 3, 1, 0], (0, 2): [1, 4, 1, 0], (0, 3): [2, 4, 1, 0],
                    (1, 0): [3, 4, 1, 0], (1, 1): [4, 4, 1, 0]},
             keep={(0, 0): 1, (0, 1): 1, (0, 2): 1, (0, 3): 1, (1, 0): 1, (1, 1): 1},
             state=(2000, 2850, 15, 1)),
        dict(advance=0, rows=[[(341, 0, None), (850, 1, None)], []],
             slots={(0, 0): [3, 4, 1, 0], (0, 1): [4, 4, 1, 0]}, keep={(0, 0): 1, (0, 1): 1},
             state=(2000, 2850, 15, 1)),                              # k = -1 and 0: the anchor stays, locked
        dict(advance=2000, rows=[[(341, 0, None), (850, 1, None), (1360, 0, None)], [(414, 0, None)]],
             slots={(0, 0): [3, 4, 1, 0], (0, 1): [4, 4, 1, 0], (0, 2): [1, 5, 1, 0], (1, 0): [3, 5, 1, 0]},
             keep={(0, 0): 1, (0, 1): 1, (0, 2): 1, (1, 0): 1},
             state=(4000, 4380, 18, 1))]))

    def one(name, state, row, slots, after, advance=98):
        out.append(dict(name=name, G=1, row_bits=0, tol=32, state=state, calls=[dict(
            advance=advance, rows=[row], slots={(0, b): v for b, v in enumerate(slots)},
            keep={(0, b): 1 for b in range(len(row))}, state=after)]))

    one("r = +4 placed", LOCK, [(1514, 0, None)], [[4, 3, 1, 0]], (98, 1514, 11, 1))
    one("r = -4 placed", LOCK, [(1506, 0, None)], [[4, 3, 1, 0]], (98, 1506, 11, 1))
    one("r = +5 not placed", LOCK, [(1515, 0, None)], [Z], (98, 1000, 10, 1))
    one("r = -5 not placed", LOCK, [(1505, 0, None)], [Z], (98, 1000, 10, 1))
    one("behind, r = +4 placed, anchor kept", LOCK, [(494, 1, None)], [[2, 3, 1, 0]], (98, 1000, 10, 1))
    one("behind, r = -4 placed", LOCK, [(486, 1, None)], [[2, 3, 1, 0]], (98, 1000, 10, 1))
    one("behind, r = +5 not placed", LOCK, [(495, 1, None)], [Z], (98, 1000, 10, 1))
    one("behind, r = -5 not placed", LOCK, [(485, 1, None)], [Z], (98, 1000, 10, 1))
    one("k = 71 placed", LOCK, [(1000 + 71 * 510, 0, None)], [[2, 3, 2, 0]], (98, 37210, 81, 1))
    one("k = 72 expires the lock", LOCK, [(1000 + 72 * 510, 0, None), (1000 + 73 * 510, 0, None)], [Z, Z],
        (98, 1000, 10, 0))
    one("k = -71 placed", LOCK, [(1000 - 71 * 510, 0, None)], [[4, 3, 60, 0]], (98, 1000, 10, 1))
    one("k = -72 ignored, lock kept", LOCK, [(1000 - 72 * 510, 0, None), (1510, 0, None)], [Z, [4, 3, 1, 0]],
        (98, 1510, 11, 1))
    one("4319 -> 0 forwards", (0, 1000, 4319, 1), [(1510, 0, None)], [[1, 1, 1, 0]], (98, 1510, 0, 1))
    one("0 -> 4319 backwards", (0, 1000, 0, 1), [(490, 0, None)], [[4, 18, 60, 0]], (98, 1000, 0, 1))
    one("bit0 near 2^40", (1 << 40, (1 << 40) + 1000, 10, 1), [(1510, 0, None), (980, 0, None)],
        [[4, 3, 1, 0], Z], ((1 << 40) + 98, (1 << 40) + 1510, 11, 1))
    one("a contradicting SYNC re-anchors", LOCK, [(1510, 2, _sb(500)), (2020, 0, None)],
        [[1, 18, 7, 3], [2, 18, 7, 0]], (98, 2020, 501, 1))
    one("a SYNC with STATUS 1 is no anchor", (0, 0, 0, 0), [(10, 2, _sb(200, fn=0)), (520, 0, None)], [Z, Z],
        (98, 0, 0, 0))
    one("a CRC-bad BSCH is no anchor", (0, 0, 0, 0), [(10, 2, _sb(200, crc=0)), (520, 0, None)], [Z, Z],
        (98, 0, 0, 0))
    # the SB 520 bits behind the anchor: off the grid (no prediction), so bit 1; the next burst is on
    # the new grid (480 + 510) and off the old one (1000 - 10)
    one("an SB behind the anchor re-anchors backwards", LOCK, [(480, 2, _sb(9)), (990, 0, None)],
        [[2, 3, 1, 3], [3, 3, 1, 0]], (98, 990, 10, 1))
    # ties: group bit 700 three times; the order is (pos, row, b), read off the FLAGS and the anchor
    out.append(dict(name="ties", G=2, row_bits=100, tol=32, state=(0, 0, 0, 0), calls=[dict(
        advance=7, rows=[[(700, 2, _sb(20)), (700, 2, _sb(30))], [(600, 2, _sb(40))]],
        slots={(0, 0): [1, 6, 1, 1], (0, 1): [3, 8, 1, 3], (1, 0): [1, 11, 1, 3]},
        keep={(0, 0): 1, (0, 1): 0, (1, 0): 0}, state=(7, 700, 40, 1))]))
    return out


def random_groups(rng, NG, G, row_bits, full=False):
    """NG groups of G rows: a continuous downlink per group on a 510-bit grid (some bursts off it, some
    missing), every row holding the bursts that start in its window of row_bits + 540 bits (the copies
    jittered by a bit or two), SBs with the true slot (a few with another, a few CRC-bad).  full: every
    row's burst table full (bursts 270 bits apart instead).  nburst of some rows is set to 0, negative or
    above MAXB over a full table."""
    rows, odd = [], {}
    for g in range(NG):
        step = 270 if full else 510
        at, slot = int(rng.integers(0, 500)), int(rng.integers(0, M.TDMA_SLOTS))
        grid = []
        while at < (G - 1) * row_bits + row_bits + 540:
            if full or rng.integers(0, 8):
                kind = int(rng.integers(0, 3))
                sy = None
                if kind == 2 and rng.integers(0, 6):
                    sy = _sb(slot if rng.integers(0, 6) else int(rng.integers(0, M.TDMA_SLOTS)), crc=int(rng.integers(0, 8) != 0))
                grid.append((at + int(rng.choice((0, 0, 0, 1, -1, 4, -4, 5, -6))), kind, sy))
            at += step
            slot = (slot + 1) % M.TDMA_SLOTS
        for i in range(G):
            lo = i * row_bits
            row = [(p - lo + int(rng.integers(-2, 3)), k, sy) for p, k, sy in grid if lo <= p < lo + row_bits + 540]
            rows.append(row[:M.MAXB])
            if len(row) >= M.MAXB and rng.integers(0, 4) == 0:
                odd[len(rows) - 1] = int(rng.choice((M.MAXB + 1, 1000)))
            elif rng.integers(0, 12) == 0:
                odd[len(rows) - 1] = int(rng.choice((0, -1, -1000)))
    arrays = arrays_of(rng, rows)
    for c, v in odd.items():
        arrays[0][c] = v
    return arrays
