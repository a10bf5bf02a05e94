"""CPU model of tetra_etsi_mac_vote_groups (TEST INFRASTRUCTURE): tetra_etsi_mac_groups with the timebase
chosen by a vote and keep chosen by quality, restated from include/tetra_hip.h in plain Python on top of
_etsi_mac_model's PDU walk and _etsi_mac_groups' order and rule 1.  Rows g G .. g G + G - 1 belong to
group g.

The rule (exact integers, positions int64).
  Order.  A group's live bursts (row i, b < nburst clamped to 0..MAXB) have pos = i row_bits + start
    bit and are taken in the order (pos, row, b), as in tetra_etsi_mac_groups.
  Clusters.  A cluster is a maximal run of that order in which every burst's pos exceeds the previous
    burst's by at most tol_bits (the chain rule); its first burst is what tetra_etsi_mac_groups keeps.
  Keep.  Burst (c, b) has a quality key Q.  good = the number of j < nblock[c] (clamped to 0..MAXJ)
    with blocks[c][j] naming burst b, a kind in 0..2 and crc_ok != 0.  bq[c][b][TERR] < 0 (an invalid
    burst): Q = -1.  Else Q = good << 32 | (60 - min(60, TERR + HERR)) << 16 | min(WSUM, 65535), with
    TERR, HERR, WSUM from bq (a negative sum or WSUM, which no record has, reads as 0).  In every
    cluster exactly one burst has keep = 1: the one with the largest Q, on a tie the first in the order.
  Ballots.  A burst has an own SYNC as in tetra_etsi_mac_groups: an SB whose BSCH block is CRC-good
    with a STATUS 0 record, of slot count s.  Its weight is w = max(1, WSUM - 2 WERR) from that block's
    kq record, at most 15240 (a larger value, which no record has, reads as 15240); a kq record whose
    NERR reads -1 gives w = 1.  In every cluster the own-SYNC burst with the largest w (on a tie the
    first) is the cluster's ballot, cast where the walk reaches it; every other burst of the cluster is
    walked as a burst without a SYNC.
  The walk.  One per group over all live bursts in the order, kept or not, p = bit0 + pos.  State:
    tdma[g] and score = max(0, tscore[g]).  Rule 1 of tetra_etsi_mac_groups gives (pred, k); a lock
    that expires (k >= TETRA_TDMA_EXPIRE) also sets score to 0.  For a ballot (s, w):
      a. not locked: anchor = (p, s), locked, score = min(cap, w); the row is s, FLAGS 1; BALLOTS++;
      b. locked and pred == s: score = min(cap, score + w), anchor = (p, s); the row is s, FLAGS 1;
         BALLOTS++, AGREED++;
      c. locked and pred != s (another slot, or none): if w > score the ballot wins: anchor = (p, s),
         score = min(cap, w - score); the row is s, FLAGS 1 | 2; BALLOTS++, WON++.  Otherwise score -=
         w; if pred is a slot the burst takes it with FLAGS 2 | 4 (bit 2: own SYNC outvoted) and the
         anchor moves to (p, pred) only if k >= 1; if pred is none the row reads 0, 0, 0, 0;
         BALLOTS++, OUTVOTED++.
    Every other burst follows rules 3 and 4 of tetra_etsi_mac_groups.  After the walk bit0 += advance
    and tscore[g] = score; without a ballot tscore changes only by expiry (and a negative one to 0).
"""
import numpy as np

import _etsi_mac_model as M
import _etsi_mac_groups as MG
import _etsi_quality_model as Q

CAP_DEFAULT = 60960
W_MAX = 15240
BALLOTS, AGREED, OUTVOTED, WON = range(4)
POISON = Q.POISON


def quality_key(c, b, nblock, blocks, bq):
    """Q of burst (c, b)."""
    if int(bq[c, b, Q.TERR]) < 0:
        return -1
    good = 0
    for j in range(min(max(int(nblock[c]), 0), M.MAXJ)):
        kind, crc, bb = int(blocks[c, j, 0]), int(blocks[c, j, 1]), int(blocks[c, j, 2])
        good += bb == b and 0 <= kind <= 2 and crc != 0
    err = min(60, max(0, int(bq[c, b, Q.TERR]) + int(bq[c, b, Q.HERR])))
    return good << 32 | (60 - err) << 16 | min(max(int(bq[c, b, Q.BWSUM]), 0), 65535)


def weight(rec):
    """w of a BSCH block's kq record."""
    if int(rec[Q.NERR]) < 0:
        return 1
    return min(W_MAX, max(1, int(rec[Q.WSUM]) - 2 * int(rec[Q.WERR])))


def slot_row(slot, flags):
    return [0, 0, 0, 0] if slot is None else [slot % 4 + 1, slot // 4 % 18 + 1, slot // 72 + 1, flags]


def clusters(order, tol_bits):
    """The order [(pos, i, b)] cut by the chain rule: [[(pos, i, b)]]."""
    out = []
    for it in order:
        if out and it[0] - out[-1][-1][0] <= tol_bits:
            out[-1].append(it)
        else:
            out.append([it])
    return out


def run(G, row_bits, tol_bits, advance, cap, nburst, bursts, nblock, blocks, type1, bq, kq, tdma, tscore):
    """tetra_etsi_mac_vote_groups on arrays shaped as the library's: (npdu [C, MAXJ], {(c, j): [record]},
    {(c, b): slot row}, {(c, b): keep}, tvote [C / G, 4]).  tdma: [MG.GroupTdma] per group and tscore: a
    list of ints per group, both updated in place."""
    C = len(nburst)
    assert 1 <= G <= MG.MAXG and C % G == 0 and row_bits >= 0 and tol_bits >= 0 and cap > 0
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
            own[(c, b)] = None   # (s, w)
            if kind == 2 and q in good_sync:
                own[(c, b)] = (good_sync[q], weight(kq[c, q]))
            q += 1 if kind == 0 else 2
    tvote = np.zeros((C // G, 4), np.int32)
    for g in range(C // G):
        td = tdma[g]
        score = max(0, int(tscore[g]))
        tv = tvote[g]
        for cl in clusters(MG.merged_order(nburst, bursts, g * G, G, row_bits), tol_bits):
            best, ballot = None, None
            for pos, i, b in cl:
                c = g * G + i
                qk = quality_key(c, b, nblock, blocks, bq)
                if best is None or qk > best[0]:
                    best = (qk, c, b)
                if own[(c, b)] is not None and (ballot is None or own[(c, b)][1] > ballot[0]):
                    ballot = (own[(c, b)][1], c, b)
            for pos, i, b in cl:
                c = g * G + i
                keep[(c, b)] = int((c, b) == best[1:])
                p = td.bit0 + pos
                pred, k = td.predict(p)
                if not td.locked:
                    score = 0 if k >= M.TDMA_EXPIRE else score
                if ballot is None or (c, b) != ballot[1:]:
                    if pred is not None and k >= 1:
                        td.anchor_bit, td.anchor_slot = p, pred
                    rows[(c, b)] = slot_row(pred, 0)
                    continue
                s, w = own[(c, b)]
                tv[BALLOTS] += 1
                if not td.locked:                                   # a
                    td.anchor_bit, td.anchor_slot, td.locked = p, s, 1
                    score = min(cap, w)
                    rows[(c, b)] = slot_row(s, 1)
                elif pred == s:                                     # b
                    td.anchor_bit, td.anchor_slot = p, s
                    score = min(cap, score + w)
                    tv[AGREED] += 1
                    rows[(c, b)] = slot_row(s, 1)
                elif w > score:                                     # c, the ballot wins
                    td.anchor_bit, td.anchor_slot = p, s
                    score = min(cap, w - score)
                    tv[WON] += 1
                    rows[(c, b)] = slot_row(s, 3)
                else:                                               # c, outvoted
                    score -= w
                    tv[OUTVOTED] += 1
                    if pred is not None and k >= 1:
                        td.anchor_bit, td.anchor_slot = p, pred
                    rows[(c, b)] = slot_row(pred, 6)
        td.bit0 += int(advance)
        tscore[g] = score
    return npdu, recs, rows, keep, tvote


def assert_equal(out, want, what=""):
    """The library's (npdu, pdus, slots, keep, tvote) against run()'s result, live entries exactly."""
    MG.assert_equal(out[:4], want[:4], what)
    assert out[4].tolist() == want[4].tolist(), (what, "tvote", out[4].tolist(), want[4].tolist())


# ------------------------------------------------------------------------------ hand-made inputs

GOOD_BQ = (0, 0, 30000, 0)       # a burst record with nothing wrong (WSUM below the key's 65535)


def arrays_of(rng, rows):
    """rows [C][(start bit, burst kind, sync)] or [(start, kind, sync, extra)] -> (nburst, bursts, nblock,
    blocks, type1, bq, kq), poisoned past every count.  sync as _etsi_mac_groups.arrays_of.  extra: dict of
      w=      the BSCH block's kq record becomes (0, 0, w, 0), so its weight is w;
      kq=     that record as given (four values);
      bq=     the burst's record as given (four values; default GOOD_BQ);
      crc=    crc_ok of the burst's blocks in order (those not BSCH; a CRC-good one gets random type-1 bits).
    A CRC-good block's kq record defaults to (0, 0, 64 K, 0), a CRC-bad one's to (-1, 0, 0, 0)."""
    base = [[(it[0], it[1], it[2]) for it in row] for row in rows]
    nburst, bursts, nblock, blocks, type1 = MG.arrays_of(rng, base)
    C = len(rows)
    bq = np.full((C, M.MAXB, 4), POISON, np.int32)
    kq = np.full((C, M.MAXJ, 4), POISON, np.int32)
    for c, row in enumerate(rows):
        j = 0
        for b, it in enumerate(row):
            extra = it[3] if len(it) > 3 else {}
            bq[c, b] = extra.get("bq", GOOD_BQ)
            nblk = 1 if it[1] == 0 else 2
            for i in range(nblk):
                kind = int(blocks[c, j, 0])
                if kind != 2 and "crc" in extra:
                    blocks[c, j, 1] = int(extra["crc"][i])
                    if blocks[c, j, 1]:
                        type1[c, j, :M.N1[kind]] = rng.integers(0, 256, M.N1[kind]).astype(np.uint8)
                kq[c, j] = (0, 0, 64 * Q.K_OF[kind], 0) if blocks[c, j, 1] else (-1, 0, 0, 0)
                if kind == 2 and blocks[c, j, 1]:
                    if "w" in extra:
                        kq[c, j] = (0, 0, extra["w"], 0)
                    if "kq" in extra:
                        kq[c, j] = extra["kq"]
                j += 1
    return nburst, bursts, nblock, blocks, type1, bq, kq


def random_quality(rng, arrays, invalid=0.1):
    """Random bq / kq for lower-MAC outputs (nburst, bursts, nblock, blocks, type1): records in the ranges
    tetra_etsi_link_quality gives, a share `invalid` of them -1 records (an invalid burst; a block that is
    CRC-bad or of an invalid burst), copies of a burst often with equal records so that ties occur; POISON
    past every count."""
    nburst, bursts, nblock, blocks, _ = arrays
    C = len(nburst)
    bq = np.full((C, M.MAXB, 4), POISON, np.int32)
    kq = np.full((C, M.MAXJ, 4), POISON, np.int32)
    for c in range(C):
        for b in range(min(max(int(nburst[c]), 0), M.MAXB)):
            if rng.random() < invalid:
                bq[c, b] = -1
            elif rng.integers(0, 3) == 0:
                bq[c, b] = GOOD_BQ
            else:
                bq[c, b] = (rng.integers(0, 5), rng.integers(0, 3), rng.choice((20000, 30000, 65535, 65280, 70000)),
                            rng.integers(0, 511))
        for j in range(min(max(int(nblock[c]), 0), M.MAXJ)):
            u = rng.random()
            if u < invalid:
                kq[c, j] = -1
            elif u < 2 * invalid or not blocks[c, j, 1]:
                kq[c, j] = (-1, 0, 0, 0)
            elif rng.integers(0, 3) == 0:
                kq[c, j] = (0, 0, 7680, 0)
            else:
                wsum = int(rng.integers(0, W_MAX + 1))
                werr = int(rng.integers(0, wsum // 2 + 2))   # sometimes WSUM - 2 WERR < 1
                kq[c, j] = (rng.integers(0, 20), werr, wsum, rng.integers(0, 5))
    return bq, kq


def _sb(slot, **kw):
    return dict(slot=slot, **kw)


def hand_cases():
    """[dict(name, G, row_bits, tol, cap, state, score, calls)]: one group each; a call is dict(advance,
    rows [G][(start, kind, sync, extra)], slots {(row, b): [tn, fn, mn, flags]}, keep {(row, b): 0 / 1},
    tvote [4], state and score after).  Every expected value is written out by hand from the rule.  Slot s
    reads tn = s % 4 + 1, fn = s / 4 % 18 + 1, mn = s / 72 + 1: 10 -> 3, 3, 1; 13 -> 2, 4, 1; 700 -> 1, 14, 10."""
    Z, LOCK, CAP = [0, 0, 0, 0], (0, 1000, 10, 1), CAP_DEFAULT
    out = []

    def one(name, state, score, row, slots, tvote, after, score_after, cap=CAP, advance=98):
        out.append(dict(name=name, G=1, row_bits=0, tol=32, cap=cap, state=state, score=score, calls=[dict(
            advance=advance, rows=[row], slots={(0, b): v for b, v in enumerate(slots)},
            keep={(0, b): 1 for b in range(len(row))}, tvote=tvote, state=after, score=score_after)]))

    # a (5000), b (8000), c with w < score (5000), c with w == score (the incumbent stays, 0), c with
    # w = 1 against 0 (wins, 1), a burst on the new grid, b with w = 9000 - 2 x 1000 (7001), c won (1999)
    one("a b c in sequence", (0, 0, 0, 0), 0,
        [(100, 2, _sb(10), dict(w=5000)), (610, 2, _sb(11), dict(w=3000)), (1120, 2, _sb(500), dict(w=3000)),
         (1630, 2, _sb(600), dict(w=5000)), (2140, 2, _sb(700), dict(w=1)), (2650, 0, None),
         (3160, 2, _sb(702), dict(kq=(3, 1000, 9000, 2))), (3670, 2, _sb(5), dict(w=9000))],
        [[3, 3, 1, 1], [4, 3, 1, 1], [1, 4, 1, 6], [2, 4, 1, 6], [1, 14, 10, 3], [2, 14, 10, 0], [3, 14, 10, 1],
         [2, 2, 1, 3]], [7, 2, 2, 2], (98, 3670, 5, 1), 1999)
    # 9000 + 5000 -> 10000; + 15240 -> 10000; a contradiction of 15240 wins: min(10000, 5240)
    one("saturation at cap", LOCK, 9000,
        [(1510, 2, _sb(11), dict(w=5000)), (2020, 2, _sb(12), dict(w=15240)), (2530, 2, _sb(99), dict(w=15240))],
        [[4, 3, 1, 1], [1, 4, 1, 1], [4, 7, 2, 3]], [3, 2, 0, 1], (98, 2530, 99, 1), 5240, cap=10000)
    one("the first ballot saturates", (0, 0, 0, 0), 0, [(100, 2, _sb(10), dict(w=5000))], [[3, 3, 1, 1]],
        [1, 0, 0, 0], (98, 100, 10, 1), 100, cap=100)
    one("a weight above 15240 reads 15240", (0, 0, 0, 0), 0, [(100, 2, _sb(10), dict(w=20000))], [[3, 3, 1, 1]],
        [1, 0, 0, 0], (98, 100, 10, 1), 15240)
    one("a kq record of -1 weighs 1", LOCK, 2, [(1510, 2, _sb(11), dict(kq=(-1, -1, -1, -1))),
                                                 (2020, 2, _sb(12), dict(kq=(-1, 0, 0, 0)))],
        [[4, 3, 1, 1], [1, 4, 1, 1]], [2, 2, 0, 0], (98, 2020, 12, 1), 4)
    one("WSUM - 2 WERR below 1 weighs 1", LOCK, 2, [(1510, 2, _sb(11), dict(kq=(9, 600, 1000, 0)))],
        [[4, 3, 1, 1]], [1, 1, 0, 0], (98, 1510, 11, 1), 3)
    one("a negative score reads 0: w = 1 wins", LOCK, -500, [(1510, 2, _sb(500), dict(w=1))], [[1, 18, 7, 3]],
        [1, 0, 0, 1], (98, 1510, 500, 1), 1)
    one("a negative score without a ballot becomes 0", LOCK, -500, [(1510, 0, None)], [[4, 3, 1, 0]],
        [0, 0, 0, 0], (98, 1510, 11, 1), 0)
    one("no ballot: the score stays", LOCK, 777, [(1510, 0, None), (2020, 2, _sb(12, crc=0))],
        [[4, 3, 1, 0], [1, 4, 1, 0]], [0, 0, 0, 0], (98, 2020, 12, 1), 777)
    one("expiry zeroes the score", LOCK, 9000, [(1000 + 72 * 510, 0, None)], [Z], [0, 0, 0, 0], (98, 1000, 10, 0), 0)
    one("expiry, then a ballot starts from 0", LOCK, 9000,
        [(1000 + 72 * 510, 0, None), (1000 + 73 * 510, 2, _sb(7), dict(w=100))], [Z, [4, 2, 1, 1]], [1, 0, 0, 0],
        (98, 1000 + 73 * 510, 7, 1), 100)
    # tetra_etsi_mac_groups gives this SB FLAGS 3; here the lock is gone when the ballot is cast: case a
    one("an SB expires the lock itself: case a", LOCK, 9000, [(1000 + 72 * 510, 2, _sb(7), dict(w=100))],
        [[4, 2, 1, 1]], [1, 0, 0, 0], (98, 1000 + 72 * 510, 7, 1), 100)
    # k = -1 (pred 9), k = 0 (pred 10), k = 1 (pred 11, r = 2): only the last moves the anchor
    one("outvoted on the grid: FLAGS 6, the anchor moves for k >= 1", LOCK, 9000,
        [(490, 2, _sb(600), dict(w=100)), (1004, 2, _sb(500), dict(w=100)), (1512, 2, _sb(700), dict(w=100))],
        [[2, 3, 1, 6], [3, 3, 1, 6], [4, 3, 1, 6]], [3, 0, 3, 0], (98, 1512, 11, 1), 8700)
    one("outvoted on the grid at k = 0: the anchor stays", LOCK, 9000, [(1004, 2, _sb(500), dict(w=100))],
        [[3, 3, 1, 6]], [1, 0, 1, 0], (98, 1000, 10, 1), 8900)
    one("outvoted off the grid reads zeros", LOCK, 9000, [(1200, 2, _sb(500), dict(w=100)), (1510, 0, None)],
        [Z, [4, 3, 1, 0]], [1, 0, 1, 0], (98, 1510, 11, 1), 8900)
    # k = -1 from slot 0: 4319 (agreed); k = 2 from 4319: 1 (agreed); k = 1: 2, the own 4319 outvoted
    one("bit0 near 2^40, both slot wraps", (1 << 40, (1 << 40) + 1000, 0, 1), 50,
        [(490, 2, _sb(4319), dict(w=10)), (1510, 2, _sb(1), dict(w=10)), (2020, 2, _sb(4319), dict(w=5))],
        [[4, 18, 60, 1], [2, 1, 1, 1], [3, 1, 1, 6]], [3, 2, 1, 0], ((1 << 40) + 98, (1 << 40) + 2020, 2, 1), 65)
    # the feature: three SBs of full weight lock the grid (45720); a foreign SB 200 bits off it with another
    # slot is outvoted and reads zeros; the four bursts after it are placed (13 .. 16)
    one("a foreign SYNC off the grid", (0, 0, 0, 0), 0,
        [(100, 2, _sb(10), dict(w=15240)), (610, 2, _sb(11), dict(w=15240)), (1120, 2, _sb(12), dict(w=15240)),
         (1320, 2, _sb(2000), dict(w=5000)), (1630, 0, None), (2140, 1, None), (2650, 0, None), (3160, 0, None)],
        [[3, 3, 1, 1], [4, 3, 1, 1], [1, 4, 1, 1], Z, [2, 4, 1, 0], [3, 4, 1, 0], [4, 4, 1, 0], [1, 5, 1, 0]],
        [4, 2, 1, 0], (98, 3160, 16, 1), 40720)
    one("a foreign SYNC on the grid bit", (0, 0, 0, 0), 0,
        [(100, 2, _sb(10), dict(w=15240)), (610, 2, _sb(11), dict(w=15240)), (1120, 2, _sb(12), dict(w=15240)),
         (1630, 2, _sb(2000), dict(w=5000)), (2140, 0, None), (2650, 1, None), (3160, 0, None), (3670, 0, None)],
        [[3, 3, 1, 1], [4, 3, 1, 1], [1, 4, 1, 1], [2, 4, 1, 6], [3, 4, 1, 0], [4, 4, 1, 0], [1, 5, 1, 0],
         [2, 5, 1, 0]], [4, 2, 1, 0], (98, 3670, 17, 1), 40720)

    def two(name, rows, slots, keep, tvote, after, score_after, state=(0, 0, 0, 0), score=0, row_bits=1966,
            advance=3932):
        out.append(dict(name=name, G=2, row_bits=row_bits, tol=32, cap=CAP, state=state, score=score, calls=[dict(
            advance=advance, rows=rows, slots=slots, keep=keep, tvote=tvote, state=after, score=score_after)]))

    # the SB at group bit 2000 and its copy at 2001: one ballot, the heavier copy's; the other copy is walked
    # without a SYNC (before the lock: zeros); 4319 -> 0
    two("two own-SYNC copies: the heavier is the ballot",
        [[(2000, 2, _sb(4319), dict(w=3000))], [(35, 2, _sb(4319), dict(w=4000)), (544, 0, None)]],
        {(0, 0): Z, (1, 0): [4, 18, 60, 1], (1, 1): [1, 1, 1, 0]}, {(0, 0): 1, (1, 0): 0, (1, 1): 1}, [1, 0, 0, 0],
        (3932, 2510, 0, 1), 4000)
    two("two own-SYNC copies of equal weight: the first is the ballot",
        [[(2000, 2, _sb(4319), dict(w=3000))], [(35, 2, _sb(4319), dict(w=3000)), (544, 0, None)]],
        {(0, 0): [4, 18, 60, 1], (1, 0): [4, 18, 60, 0], (1, 1): [1, 1, 1, 0]}, {(0, 0): 1, (1, 0): 0, (1, 1): 1},
        [1, 0, 0, 0], (3932, 2510, 0, 1), 3000)
    # the lighter copy's SYNC is not heard at all, whatever slot it names
    two("the lighter copy names another slot: no contradiction",
        [[(2000, 2, _sb(4319), dict(w=4000))], [(35, 2, _sb(17), dict(w=3000)), (544, 0, None)]],
        {(0, 0): [4, 18, 60, 1], (1, 0): [4, 18, 60, 0], (1, 1): [1, 1, 1, 0]}, {(0, 0): 1, (1, 0): 0, (1, 1): 1},
        [1, 0, 0, 0], (3932, 2510, 0, 1), 4000)
    # keep: rows 0 and 1 on the same bits (row_bits 0), copies two bits apart, six clusters in order:
    #   good 0 < 2 (the feature: row 0's copy CRC-bad in both blocks, row 1's good in both); errors 4 > 3;
    #   WSUM 20000 < 20001; a tie (the first); an invalid burst (Q = -1) against Q = 0; one good block more
    #   outweighs every error and every WSUM
    P = lambda start, crc, bq=GOOD_BQ: (start, 1, None, dict(crc=crc, bq=bq))
    two("keep by quality",
        [[P(1000, (0, 0)), P(1510, (1, 1), (3, 1, 30000, 0)), P(2020, (1, 1), (0, 0, 20000, 0)), P(2530, (1, 1)),
          P(3040, (1, 1), (-1, -1, -1, -1)), P(3550, (1, 1), (20, 2, 100, 0))],
         [P(1002, (1, 1)), P(1512, (1, 1), (2, 1, 30000, 0)), P(2022, (1, 1), (0, 0, 20001, 0)), P(2532, (1, 1)),
          P(3042, (0, 0), (30, 40, 0, 0)), P(3552, (1, 0), (0, 0, 65535, 0))]],
        {(i, b): Z for i in range(2) for b in range(6)},
        {(0, 0): 0, (1, 0): 1, (0, 1): 0, (1, 1): 1, (0, 2): 0, (1, 2): 1, (0, 3): 1, (1, 3): 0, (0, 4): 0, (1, 4): 1,
         (0, 5): 1, (1, 5): 0}, [0, 0, 0, 0], (0, 0, 0, 0), 0, row_bits=0, advance=0)
    # a chain of three copies (tol 32: 1000, 1030, 1060 is one cluster): the best is the last
    two("a chain of three: one kept",
        [[P(1000, (1, 0)), P(1060, (1, 1))], [P(1030, (0, 0)), P(1600, (0, 0))]],
        {(0, 0): Z, (0, 1): Z, (1, 0): Z, (1, 1): Z}, {(0, 0): 0, (0, 1): 1, (1, 0): 0, (1, 1): 1}, [0, 0, 0, 0],
        (0, 0, 0, 0), 0, row_bits=0, advance=0)
    # a stream (tests/_etsi_mac_groups.py's carried tail): the score travels with the timebase; the third
    # call's SB agrees (7680 + 1000)
    out.append(dict(name="state and score over three calls", G=2, row_bits=1966, tol=32, cap=CAP, state=(0, 0, 0, 0),
                    score=0, calls=[
        dict(advance=2000,
             rows=[[(300, 2, _sb(10)), (810, 0, None), (1320, 1, None), (1830, 0, None)], [(374, 0, None), (884, 1, None)]],
             slots={(0, 0): [3, 3, 1, 1], (0, 1): [4, 3, 1, 0], (0, 2): [1, 4, 1, 0], (0, 3): [2, 4, 1, 0],
                    (1, 0): [3, 4, 1, 0], (1, 1): [4, 4, 1, 0]},
             keep={(0, 0): 1, (0, 1): 1, (0, 2): 1, (0, 3): 1, (1, 0): 1, (1, 1): 1}, tvote=[1, 0, 0, 0],
             state=(2000, 2850, 15, 1), score=7680),
        dict(advance=0, rows=[[(341, 0, None), (850, 1, None)], []],
             slots={(0, 0): [3, 4, 1, 0], (0, 1): [4, 4, 1, 0]}, keep={(0, 0): 1, (0, 1): 1}, tvote=[0, 0, 0, 0],
             state=(2000, 2850, 15, 1), score=7680),
        dict(advance=2000, rows=[[(341, 0, None), (850, 1, None), (1360, 2, _sb(16), dict(w=1000))], [(414, 0, None)]],
             slots={(0, 0): [3, 4, 1, 0], (0, 1): [4, 4, 1, 0], (0, 2): [1, 5, 1, 1], (1, 0): [3, 5, 1, 0]},
             keep={(0, 0): 1, (0, 1): 1, (0, 2): 1, (1, 0): 1}, tvote=[1, 1, 0, 0],
             state=(4000, 4380, 18, 1), score=8680)]))
    return out
