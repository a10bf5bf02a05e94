"""Scenarios for tetra_etsi_sdu (TEST INFRASTRUCTURE): bursts on a stream's bit axis, cut into calls of
one group of G rows, shaped as the library's arrays by _etsi_sdu_model.build_rows.  The CPU tests hold
the model to each scenario's stated outcome; the GPU tests hold the kernel to the model on the same calls.
"""
import numpy as np

import _etsi_mac_model as M
import _etsi_sdu_model as S

SLOT = 510
FIRST_CAP, MID_CAP, LAST_CAP = 268 - 40 - 3, 268 - 4, 268 - 13   # SCH/F, address type 1


def first(bits, ssi=0x123456, n1=268):
    return [S.resource_pdu(63, 1, bits, n1, ssi=ssi)]


def mid(bits, n1=268):
    return [S.frag_pdu(bits, n1)]


def last(bits, n1=268):
    """A MAC-END with the rest of an SDU, then a null PDU so that the block's walk stops."""
    used = 13 + len(bits)
    length = max(2, (used + 7) // 8)
    nbits = min(8 * length, n1)
    return [S.end_pdu(length, bits, nbits, fill=int(nbits != used)), M.null_pdu()]


def ndb(p, pdus):
    """A normal burst (training sequence n) at stream bit p with one SCH/F block; pdus None: CRC-bad."""
    return (p, 0, [pdus])


def ndp(p, pdus1, pdus2):
    return (p, 1, [pdus1, pdus2])


class Scenario:
    """bursts [(stream bit, burst kind, [block])] -> calls of one group.  G == 1: one row per call, the
    streaming form (nsym gives the advance).  G > 1: rows row_bits apart and 2 row_bits long (the last one
    row_bits), so a burst in an overlap is in two rows; keep marks the first copy."""

    def __init__(self, name, bursts, G=1, bit0=0, gap_slots=S.GAP_DEFAULT, maxd=4, ncalls=None, chunk=8 * SLOT,
                 row_bits=4 * SLOT, use_keep=True):
        self.name, self.bursts, self.G, self.bit0, self.gap_slots, self.maxd = name, bursts, G, bit0, gap_slots, maxd
        self.chunk = chunk if G == 1 else G * row_bits
        self.row_bits = 0 if G == 1 else row_bits
        self.use_keep = use_keep and G > 1
        self.ncalls = ncalls or max(p for p, _, _ in bursts) // self.chunk + 1

    def calls(self, rng):
        out = []
        for n in range(self.ncalls):
            rows, keeps = [[] for _ in range(self.G)], [[] for _ in range(self.G)]
            for p, kind, blks in self.bursts:
                rel = p - n * self.chunk
                if not 0 <= rel < self.chunk:
                    continue
                if self.G == 1:
                    rows[0].append((rel, kind, blks))
                    continue
                seen = False
                for i in range(self.G):
                    length = 2 * self.row_bits if i < self.G - 1 else self.row_bits
                    if i * self.row_bits <= rel < i * self.row_bits + length:
                        rows[i].append((rel - i * self.row_bits, kind, blks))
                        keeps[i].append(0 if seen else 1)
                        seen = True
            arrays = S.build_rows(rng, rows)
            keep = None
            if self.use_keep:
                keep = rng.integers(-5, 5, (self.G, S.MAXB)).astype(np.int32)   # poison past nburst
                keep[keep == 0] = 7
                for i, k in enumerate(keeps):
                    keep[i, :len(k)] = k
            out.append(dict(G=self.G, row_bits=self.row_bits, advance=self.chunk, gap_slots=self.gap_slots,
                            maxd=self.maxd, nsym=np.full(self.G, self.chunk // 2 + 1, np.int32), arrays=arrays,
                            keep=keep))
        return out


def run_model(sc, rng):
    """The model over a scenario's calls: (every done record in order [(fields, bytes)], ndone per call, Frag)."""
    fr = S.Frag(sc.bit0)
    done, counts = [], []
    for call in sc.calls(rng):
        _, ndone, d = S.run([fr], call["G"], call["row_bits"], call["advance"], call["gap_slots"], call["maxd"],
                            call["nsym"], *call["arrays"], keep=call["keep"])
        done += [d[k] for k in sorted(d)]
        counts.append(int(ndone[0]))
    return done, counts, fr


def payload(rng, n):
    return rng.integers(0, 2, n).tolist()


def chain_bursts(rng, sdu, nfrag, p0, step=4 * SLOT, ssi=0x123456):
    """An SDU cut into nfrag SCH/F fragments on bursts step apart from p0 (fragment() with a null PDU after
    the MAC-END)."""
    pdus = S.fragment(sdu, [0] * nfrag, ssi=ssi)
    return [ndb(p0 + i * step, [pd] if i < nfrag - 1 else [pd, M.null_pdu()]) for i, pd in enumerate(pdus)]


def sdu_len(rng, nfrag):
    lo, hi = S.capacity([0] * nfrag)
    return int(rng.integers(lo, hi + 1))


# ------------------------------------------------------------------------------ Part B at its edges
# Each returns (Scenario, expected): expected = dict(done=[bit lists], dropped, orphans, ...).

def edge_cases(rng):
    A, B = payload(rng, FIRST_CAP), payload(rng, FIRST_CAP)
    ea, eb = payload(rng, 77), payload(rng, 130)
    p = 1000
    out = []

    def add(name, bursts, **kw):
        exp = {k: kw.pop(k) for k in ("done", "dropped", "orphans", "gaps", "counts", "active") if k in kw}
        out.append((Scenario(name, bursts, **kw), exp))

    add("tol 4 joins", [ndb(p, first(A)), ndb(p + 4 * SLOT + 4, last(ea))], done=[A + ea], dropped=0, orphans=0)
    add("tol -4 joins", [ndb(p, first(A)), ndb(p + 4 * SLOT - 4, last(ea))], done=[A + ea], dropped=0, orphans=0)
    add("tol 5 does not", [ndb(p, first(A)), ndb(p + 4 * SLOT + 5, last(ea))], done=[], dropped=0, orphans=1, active=1)
    add("k % 4 != 0", [ndb(p, first(A)), ndb(p + SLOT, last(ea))], done=[], dropped=0, orphans=1, active=1)
    add("gap == gap_slots joins", [ndb(p, first(A)), ndb(p + 72 * SLOT, last(ea))], done=[A + ea], dropped=0, orphans=0)
    add("gap_slots + 4 expires", [ndb(p, first(A)), ndb(p + 76 * SLOT, last(ea))], done=[], dropped=1, orphans=1,
        active=0)
    add("supersede", [ndb(p, first(A)), ndb(p + 4 * SLOT, first(B)), ndb(p + 8 * SLOT, last(eb))], done=[B + eb],
        dropped=1, orphans=0)
    starts = [ndb(p + i * SLOT, first(payload(rng, FIRST_CAP), ssi=100 + i)) for i in range(4)]
    add("fifth start evicts the oldest",
        starts + [ndb(p + 4 * SLOT + 100, first(B, ssi=555)), ndb(p + 8 * SLOT + 100, last(eb)),
                  ndb(p + 8 * SLOT, last(ea))],   # the evicted chain's MAC-END finds nothing
        done=[B + eb], dropped=1, orphans=1, active=3)
    long = [ndb(p, first(A))] + [ndb(p + (i + 1) * 4 * SLOT, mid(payload(rng, MID_CAP))) for i in range(15)]
    add("overflow", long + [ndb(p + 16 * 4 * SLOT, last(ea))], done=[], dropped=1, orphans=1, active=0)
    add("END without a chain", [ndb(p, last(ea))], done=[], dropped=0, orphans=1)
    h1, h2 = payload(rng, 124 - 43), payload(rng, 60)
    add("SCH/HD block 1 starts, block 2 ends", [ndp(p, first(h1, n1=124), last(h2, n1=124))], done=[h1 + h2],
        dropped=0, orphans=0, gaps=[0])
    m = payload(rng, MID_CAP)
    add("GAPS over a CRC-bad burst",
        [ndb(p, first(A)), ndb(p + 4 * SLOT, None), ndb(p + 8 * SLOT, mid(m)), ndb(p + 12 * SLOT, last(ea))],
        done=[A + m + ea], dropped=0, orphans=0, gaps=[1])
    add("maxd below the completions",
        [ndb(p, first(A)), ndb(p + SLOT, first(B, ssi=9)), ndb(p + 4 * SLOT, last(ea)), ndb(p + 5 * SLOT, last(eb))],
        maxd=1, done=[A + ea], counts=[2], dropped=0, orphans=0)
    ma, mb = payload(rng, MID_CAP), payload(rng, MID_CAP)
    add("two chains on two timeslots",
        [ndb(p, first(A, ssi=1)), ndb(p + SLOT, first(B, ssi=2)), ndb(p + 4 * SLOT, mid(ma)), ndb(p + 5 * SLOT, mid(mb)),
         ndb(p + 8 * SLOT, last(ea)), ndb(p + 9 * SLOT, last(eb))], done=[A + ma + ea, B + mb + eb], dropped=0,
        orphans=0, gaps=[0, 0])
    e8 = payload(rng, 8 * 6 - 13)   # a MAC-END of exactly six octets, no fill
    b2 = payload(rng, 268 - 48 - 43)
    add("[END of A][start of B]",
        [ndb(p, first(A)), ndb(p + 4 * SLOT, [S.end_pdu(6, e8, 48), S.resource_pdu(63, 1, b2, 220, ssi=77)]),
         ndb(p + 8 * SLOT, last(eb))], done=[A + e8, b2 + eb], dropped=0, orphans=0)
    add("bit0 above 2^31", [ndb(p, first(A)), ndb(p + 4 * SLOT, last(ea)), ndb(p + 8 * SLOT, first(B))],
        bit0=(1 << 33) + 7, done=[A + ea], dropped=0, orphans=0, active=1)
    return out


def group_cases(rng):
    """G > 1: a chain over overlapping rows; every burst of an overlap sits in two rows."""
    out = []
    for G, nfrag in ((2, 3), (3, 5), (2, 8)):
        sdu = payload(rng, sdu_len(rng, nfrag))
        out.append((Scenario(f"G {G}, {nfrag} fragments", chain_bursts(rng, sdu, nfrag, 300), G=G), sdu))
    return out


# ------------------------------------------------------------------------------ a seeded sweep

def random_pdus(rng, n1):
    """One block's PDUs: ~20 % fragments, ~10 % malformed, the rest MAC-RESOURCEs with random elements."""
    u = rng.random()
    if u < 0.07:
        at = int(rng.choice([1, 2, 3, 5, 6]))
        has_ssi, auxn = M.ADDRESS[at]
        return [S.resource_pdu(63, at, payload(rng, n1 - 16 - 24 * has_ssi - auxn - 3), n1, ssi=int(rng.integers(1 << 24)),
                               aux=int(rng.integers(1 << auxn)) if auxn else 0)]
    if u < 0.14:
        return mid(payload(rng, n1 - 4), n1)
    if u < 0.21:
        return last(payload(rng, int(rng.integers(0, n1 - 13 + 1))), n1)
    if u < 0.31:   # malformed: a fill flag over zeros, elements past the end, a bad length
        v = rng.integers(0, 3)
        if v == 0:
            return [[0, 0, 1, 0, 0, 0, 0] + M.bits_of(5, 6) + [0, 1, 0] + M.bits_of(3, 10) + [0] * 14, M.null_pdu()]
        if v == 1:
            return [[0, 0, 0, 0, 0, 0, 0] + M.bits_of(4, 6) + [0, 1, 0] + M.bits_of(3, 10) + [1, 1, 1, 1, 1, 1], M.null_pdu()]
        return [M.mac_end(rng, 1)]
    if u < 0.36:
        return [M.block(rng, 0, [])[:n1].tolist()]   # anything at all
    pdus, room = [], n1
    for _ in range(int(rng.integers(1, 4))):
        at = int(rng.integers(1, 8))
        has_ssi, auxn = M.ADDRESS[at]
        ca = None
        if rng.random() < 0.5:
            ca = dict(allocation_type=int(rng.integers(4)), timeslot_assigned=int(rng.integers(16)),
                      updownlink_assigned=int(rng.integers(0 if rng.random() < 0.1 else 1, 4)),
                      clch_permission=int(rng.integers(2)), cell_change=int(rng.integers(2)),
                      carrier=int(rng.integers(4096)),
                      extended=dict(band=int(rng.integers(16)), offset=int(rng.integers(4)),
                                    duplex_spacing=int(rng.integers(8)), reverse_operation=int(rng.integers(2)))
                      if rng.random() < 0.5 else None,
                      monitoring_pattern=int(rng.integers(4)), frame18_monitoring=int(rng.integers(4)))
        el = S.elements(M.RESOURCE, int(rng.integers(16)) if rng.random() < 0.5 else None,
                        int(rng.integers(256)) if rng.random() < 0.5 else None, ca)
        fill = int(rng.integers(2))
        need = 16 + 24 * has_ssi + auxn + len(el) + fill
        length = int(rng.integers((need + 7) // 8, (need + 7) // 8 + 6))
        if 8 * length > room or length > 34:
            break
        enc = int(rng.integers(1, 4)) if rng.random() < 0.1 else 0
        pdus.append(S.resource_pdu(length, at, payload(rng, 8 * length - need), 8 * length, ssi=int(rng.integers(1 << 24)),
                                   aux=int(rng.integers(1 << auxn)) if auxn else 0, fill=fill, enc=enc, elems=el))
        room -= 8 * length
    return pdus + [M.null_pdu()]


def random_call(rng, C, G, row_bits=4 * SLOT):
    """One call of C rows in groups of G: bursts on a slot grid with a little jitter, blocks from
    random_pdus, 1 in 8 blocks CRC-bad; with G > 1 the bursts of an overlap are in both rows and keep is
    the first copy's.  Returns (rows arrays, keep or None)."""
    rows, keeps = [], []
    for g in range(C // G):
        if G == 1:
            nb = int(rng.integers(0, S.MAXB + 1))
            bursts = [(i * SLOT + int(rng.integers(-2, 3)), i) for i in range(nb)]
            grows = [[(p,) + random_burst(rng) for p, _ in bursts]]
            gkeep = [[1] * nb]
        else:
            span = (G + 1) * row_bits
            made = [(s * SLOT + 40 + int(rng.integers(-2, 3)),) + random_burst(rng)
                    for s in range(span // SLOT) if rng.random() < 0.8]
            grows, gkeep = [[] for _ in range(G)], [[] for _ in range(G)]
            for p, kind, blks in made:
                seen = False
                for i in range(G):
                    if i * row_bits <= p < (i + 2) * row_bits and len(grows[i]) < S.MAXB:
                        grows[i].append((p - i * row_bits, kind, blks))
                        gkeep[i].append(0 if seen else 1)
                        seen = True
        rows += grows
        keeps += gkeep
    arrays = S.build_rows(rng, rows)
    keep = None
    if G > 1:
        keep = rng.integers(1, 9, (C, S.MAXB)).astype(np.int32)
        for i, k in enumerate(keeps):
            keep[i, :len(k)] = k
    return arrays, keep


def random_burst(rng):
    kind = int(rng.choice([0, 0, 1, 2]))
    blks = []
    for bk in S.BLOCKS_OF[kind]:
        if rng.random() < 0.125:
            blks.append(None)
        elif bk == 2:
            blks.append([M.sync(M.random_fields(rng, M.SYNC_LAYOUT))])
        else:
            blks.append(random_pdus(rng, M.N1[bk]))
    return kind, blks
