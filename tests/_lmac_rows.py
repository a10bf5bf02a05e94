"""Rows of dibits and int8 soft bits built on the CPU for the lower-MAC tests (TEST INFRASTRUCTURE).

The ETSI lower MAC's production kernels (k_etsi_sync, k_etsi_viterbi, k_etsi_traceback,
k_cell_acquire, k_etsi_tail) are otherwise fed the demodulator's output on synthesised captures,
where training sequences match in full and hard and soft bits agree in sign.  The rows here are
placed instead: bursts at chosen bit offsets with chosen scored bits flipped, and soft bits of the
block fields set independently of the hard bits.  tests/test_lmac_rows.py proves on the CPU oracle
that they mean what tests/test_gpu_lmac_rows.py assumes.

Burst layout (oracle/etsi.py make_burst, EN 300 392-2 §9.4.4): 510 bits; the scan scores the head
q11..q22 at 0..11, the tail q1..q10 at 500..509 and the training sequence (n / p at 244..265, y at
214..251); the coded blocks sit at 14..229 and 282..497 (normal bursts) or 94..213 and 282..497
(synchronisation burst).
"""
import numpy as np

import etsi as E

LmacStreamModel = E.LmacStream   # the lower-MAC half of oracle.etsi.Stream.push, restated once

NDB_N, NDB_P, SB = E.BURST_NDB_N, E.BURST_NDB_P, E.BURST_SB
TOTAL = {NDB_N: 44, NDB_P: 44, SB: 60}   # scored bits
THRESH = {NDB_N: 40, NDB_P: 40, SB: 54}  # matches a burst needs
# the coded blocks of a burst kind: (block kind, [(first bit, length), ...] of its type-5 bits)
BLOCK_FIELDS = {NDB_N: [(0, [(14, 216), (282, 216)])],
                NDB_P: [(1, [(14, 216)]), (1, [(282, 216)])],
                SB: [(2, [(94, 120)]), (1, [(282, 216)])]}
NP_DIFFER = np.flatnonzero(E.N_BITS != E.P_BITS) + 244   # the 10 of 22 positions where n and p differ:
# a burst cannot score >= 40 of 44 on both, so no input makes the n / p choice a tie at the threshold
SOFT_CLASSES = ("clean", "m128", "zero", "tern", "uniform", "inverted", "gauss")
SOFT_DRAW = SOFT_CLASSES + ("gauss",) * 5   # a block's class is drawn from these: half are Gaussian
GAUSS_MEAN = 32
# per block kind, the sigma at which the oracle passes the CRC on about half of 300 random blocks
# (shares measured one below / at / one above: SCH/F 0.56 at 21 and 0.38 at 22; SCH/HD 0.67 / 0.45 /
# 0.27; BSCH 0.56 / 0.49 / 0.25): tests/test_lmac_rows.py holds the share in [0.25, 0.75]
GAUSS_SIGMA = {0: 21.5, 1: 23.0, 2: 25.0}


def plant(bits, off, burst):
    """Write a 510-bit burst at bit offset off (odd offsets included)."""
    bits[off:off + 510] = burst


def hard_of(bits):
    """Dibits of a bit stream: bit p is dibit p >> 1, b1 in the high bit (inverse of Receiver.hard_bits)."""
    b = np.asarray(bits, np.uint8)
    assert len(b) % 2 == 0
    return ((b[0::2] << 1) | b[1::2]).astype(np.uint8)


def soft_of(bits, amp=127):
    """+amp for a 0, -amp for a 1."""
    return np.where(np.asarray(bits) == 0, amp, -amp).astype(np.int8)


def scored_positions(kind):
    train = range(214, 252) if kind == SB else range(244, 266)
    return np.array(list(range(0, 12)) + list(train) + list(range(500, 510)))


def flip_scored(burst, kind, positions):
    """A copy of the burst with the given scored bits flipped."""
    pos = np.asarray(positions, np.int64)
    assert len(set(pos.tolist())) == len(pos) and set(pos.tolist()) <= set(scored_positions(kind).tolist())
    out = burst.copy()
    out[pos] ^= 1
    return out


def sync_pdu(rng, mcc, mnc, cc):
    """60 BSCH type-1 bits carrying a cell (the fields bsch_cell_init reads), the rest random."""
    t = rng.integers(0, 2, 60).astype(np.uint8)
    for v, lo, n in ((cc, 4, 6), (mcc, 31, 10), (mnc, 41, 14)):
        t[lo:lo + n] = [(v >> (n - 1 - i)) & 1 for i in range(n)]
    return t


def random_cell(rng):
    return E.scramble_init(int(rng.integers(1, 1024)), int(rng.integers(0, 1 << 14)), int(rng.integers(0, 64)))


# ------------------------------------------------------------------------------ soft-bit classes

def soft_class(name, tx, rng, kind=0):
    """int8 soft bits of one class for a field whose transmitted (type-5) bits are tx."""
    n = len(tx)
    clean = soft_of(tx, 127)
    if name == "clean":
        return clean
    if name == "m128":   # -128 mixed in at a tenth of the positions, whatever the bit
        out = clean.copy()
        out[rng.random(n) < 0.1] = -128
        return out
    if name == "zero":
        return np.zeros(n, np.int8)
    if name == "tern":
        return rng.integers(-1, 2, n).astype(np.int8)
    if name == "uniform":
        return rng.integers(-128, 128, n).astype(np.int8)
    if name == "inverted":
        return soft_of(1 - np.asarray(tx), 127)
    if name == "gauss":
        v = np.where(np.asarray(tx) == 0, GAUSS_MEAN, -GAUSS_MEAN) + rng.normal(0.0, GAUSS_SIGMA[kind], n)
        return np.rint(v).clip(-127, 127).astype(np.int8)
    raise ValueError(name)


def block_soft(soft_row, start, fields):
    """The type-5 soft block of one coded block cut out of a row's soft bits."""
    return np.concatenate([soft_row[start + o:start + o + n] for o, n in fields])


# ------------------------------------------------------------------------------ scan thresholds

def threshold_case(rng, kind, extra, where="any", nbits=1600):
    """A random row with one burst of `kind` at a random offset, TOTAL - THRESH + extra scored bits
    flipped (extra 0: exactly at the threshold; 1: one past it).  `where` keeps the flips in one
    field: head, tail (bit 509 among them), y32 (the sync sequence's last six bits), np (positions
    where n and p differ).  Returns (bits, off, kind, found)."""
    cell = E.scramble_seq(random_cell(rng), 432)
    burst, _ = E.make_burst(kind, rng, cell)
    nflip = TOTAL[kind] - THRESH[kind]
    pool = {"any": scored_positions(kind), "head": np.arange(0, 12), "tail": np.arange(500, 509),
            "y32": np.arange(246, 252), "np": NP_DIFFER}[where]
    if where == "tail":
        pos = np.concatenate([[509], rng.choice(pool, nflip - 1, replace=False)])
    else:
        pos = rng.choice(pool, nflip, replace=False)
    if extra:   # one more, anywhere among the scored bits not flipped yet
        rest = np.setdiff1d(scored_positions(kind), pos)
        pos = np.concatenate([pos, rng.choice(rest, extra, replace=False)])
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    off = int(rng.integers(0, nbits - 510 + 1))
    plant(bits, off, flip_scored(burst, kind, pos))
    return bits, off, kind, extra == 0


FIXED_THRESHOLD_CASES = [(k, w) for k in (NDB_N, NDB_P, SB) for w in ("head", "tail")] + \
                        [(SB, "y32"), (NDB_N, "np"), (NDB_P, "np")]


def threshold_rows(seed, trials):
    """`trials` random cases per (kind, at / one past the threshold), then the fixed cases (each at
    and one past): [(bits, off, kind, found)]."""
    rng = np.random.default_rng(seed)
    rows = [threshold_case(rng, k, e) for k in (NDB_N, NDB_P, SB) for e in (0, 1) for _ in range(trials)]
    rows += [threshold_case(rng, k, e, w) for k, w in FIXED_THRESHOLD_CASES for e in (0, 1)]
    return rows


# ------------------------------------------------------------------------------ burst streams

GAPS = (0, 0, 0, 1, 7, 64, 300, 511)
CHUNKS = (1, 2, 5, 100, 255, 256, 257, 700, 1500, 1790)   # dibits


def burst_stream(seed, cell_init=None, kinds=None, payloads=None):
    """A stream of 3-13 bursts of random kinds with gaps from GAPS between them (random bits in the
    gaps), an even number of bits.  Returns (bits, [(start, kind)], [[(block kind, type-1)]], cell init)."""
    rng = np.random.default_rng(seed)
    cell_init = cell_init if cell_init is not None else random_cell(rng)
    cell = E.scramble_seq(cell_init, 432)
    n = int(rng.integers(3, 14)) if kinds is None else len(kinds)
    parts, planted, jobs, at = [], [], [], 0
    for i in range(n):
        g = int(rng.choice(GAPS))
        parts.append(rng.integers(0, 2, g).astype(np.uint8))
        at += g
        k = int(rng.integers(0, 3)) if kinds is None else kinds[i]
        b, j = E.make_burst(k, rng, cell, None if payloads is None else payloads[i])
        parts.append(b)
        planted.append((at, k))
        jobs.append(j)
        at += 510
    g = int(rng.choice(GAPS))
    g += (at + g) & 1
    parts.append(rng.integers(0, 2, g).astype(np.uint8))
    return np.concatenate(parts), planted, jobs, cell_init


def place_bursts(rng, items, tail_gap=0):
    """A row of bursts, each with its own scrambling: items = [(gap bits before, burst kind, cell init
    the blocks are scrambled with, payloads or None)].  An even number of bits.  Returns
    (bits, [(start, kind)], [[(block kind, type-1)]])."""
    parts, planted, jobs, at = [], [], [], 0
    for g, k, init, pay in items:
        parts.append(rng.integers(0, 2, g).astype(np.uint8))
        at += g
        b, j = E.make_burst(k, rng, E.scramble_seq(int(init), 432), None if pay is None else list(pay))
        parts.append(b)
        planted.append((at, k))
        jobs.append(j)
        at += 510
    g = tail_gap + ((at + tail_gap) & 1)
    parts.append(rng.integers(0, 2, g).astype(np.uint8))
    return np.concatenate(parts), planted, jobs


def cell_fields(rng):
    """A random cell: (scrambling init, (mcc, mnc, colour code))."""
    f = int(rng.integers(1, 1024)), int(rng.integers(0, 1 << 14)), int(rng.integers(0, 64))
    return E.scramble_init(*f), f


def sync_payloads(rng, fields):
    """Payloads of a synchronisation burst whose BSCH announces the cell `fields`."""
    return [sync_pdu(rng, *fields), rng.integers(0, 2, 124).astype(np.uint8)]


def chunk_cuts(seed, ndibits, sizes=CHUNKS):
    """Cut ndibits into chunks of random sizes from `sizes`: [(first dibit, count)]."""
    rng = np.random.default_rng(seed)
    out, at = [], 0
    while at < ndibits:
        n = min(int(rng.choice(sizes)), ndibits - at)
        out.append((at, n))
        at += n
    return out


def cuts_at(ndibits, points):
    """Chunks with seams at the given dibits."""
    p = [0] + sorted({int(v) for v in points if 0 < v < ndibits}) + [ndibits]
    return [(a, b - a) for a, b in zip(p, p[1:])]


# ------------------------------------------------------------------------------ Viterbi batch

def viterbi_batch(seed, C, wmod=0):
    """C rows for the production trellis: three bursts each (every burst kind, order rotated by the
    channel), the first at start bit ch mod 4 and the next ones after gaps of 0..3 bits, so the soft
    segments sit at every byte alignment; the hard bits are the clean bursts (the scan fires), the
    soft bits of every coded block are of a class drawn from SOFT_DRAW, set independently.  The last
    channel's last burst ends on the row's last bit.  Row width (symbols): the first that holds the
    longest row with width mod 4 = wmod.  Returns dict(hard [C, smax], soft [C, 2 smax], nsym, cells,
    blocks: per channel [(start, burst kind, block kind, fields, class, type-1, tx type-5)])."""
    rng = np.random.default_rng(seed)
    cells = np.array([random_cell(rng) for _ in range(C)], np.uint32)
    rows = []
    for ch in range(C):
        scr = E.scramble_seq(int(cells[ch]), 432)
        at = ch % 4
        bits, soft, blocks = [rng.integers(0, 2, at).astype(np.uint8)], [], []
        soft.append(rng.integers(-128, 128, at).astype(np.int8))
        for i in range(3):
            bk = (ch + i) % 3
            burst, jobs = E.make_burst(bk, rng, scr)
            sb = rng.integers(-128, 128, 510).astype(np.int8)   # outside the blocks: never read
            for (kind, fields), (_, t1) in zip(BLOCK_FIELDS[bk], jobs):
                cls = SOFT_DRAW[int(rng.integers(0, len(SOFT_DRAW)))]
                tx = np.concatenate([burst[o:o + n] for o, n in fields])
                v = soft_class(cls, tx, rng, kind)
                p = 0
                for o, n in fields:
                    sb[o:o + n] = v[p:p + n]
                    p += n
                blocks.append((at, bk, kind, fields, cls, t1, tx))
            bits.append(burst)
            soft.append(sb)
            at += 510
            if i < 2:
                g = int(rng.integers(0, 4))
                if ch == C - 1 and i == 1:
                    g += (at + g) & 1
            else:   # an even number of bits; the last channel's row ends with its last burst
                g = (at & 1) if ch == C - 1 else (at & 1) + 2 * int(rng.integers(0, 3))
            bits.append(rng.integers(0, 2, g).astype(np.uint8))
            soft.append(rng.integers(-128, 128, g).astype(np.int8))
            at += g
        rows.append((np.concatenate(bits), np.concatenate(soft), blocks))
    smax = max(len(b) for b, _, _ in rows) // 2 + 1
    smax += (wmod - smax) % 4
    hard = np.zeros((C, smax), np.uint8)
    soft = np.zeros((C, 2 * smax), np.int8)
    nsym = np.zeros(C, np.int32)
    for ch, (b, s, _) in enumerate(rows):
        hard[ch, :len(b) // 2] = hard_of(b)
        soft[ch, :len(s)] = s
        nsym[ch] = len(b) // 2 + 1
    return dict(hard=hard, soft=soft, nsym=nsym, cells=cells, blocks=[r[2] for r in rows])


# ------------------------------------------------------------------------------ oracle views

def oracle_rows(hard, soft, nsym, cells):
    """Receiver.lower_mac per row: [[(start, burst kind, [(kind, type-1, crc_ok)])]]."""
    rx = E.Receiver()
    out = []
    for ch in range(len(nsym)):
        nd = max(int(nsym[ch]) - 1, 0)
        out.append(rx.lower_mac(soft[ch, :2 * nd], hard[ch, :nd], int(cells[ch])))
    return out


def flatten(want):
    """An oracle row result in the library's output layout: (bursts [(start, kind)], blocks
    [(kind, crc_ok, burst, index)], type-1 bits per block)."""
    bursts = [(s, k) for s, k, _ in want]
    blocks = [(kind, int(ok), b, i) for b, (_, _, dec) in enumerate(want) for i, (kind, _, ok) in enumerate(dec)]
    bits = [t1 for _, _, dec in want for _, t1, _ in dec]
    return bursts, blocks, bits


# ------------------------------------------------------------------------------ the library's calls

def pack_rows(rows, smax):
    """[(bits, soft)] -> hard [C, smax], soft [C, 2 smax], nsym [C] (nsym - 1 dibits per row)."""
    C = len(rows)
    hard = np.zeros((C, smax), np.uint8)
    soft = np.zeros((C, 2 * smax), np.int8)
    nsym = np.zeros(C, np.int32)
    for ch, (b, s) in enumerate(rows):
        hard[ch, :len(b) // 2] = hard_of(b)
        soft[ch, :len(b)] = s
        nsym[ch] = len(b) // 2 + 1
    return hard, soft, nsym


def lmac_outputs(C):
    from tetraear import _hip
    return dict(nburst=np.zeros(C, np.int32), bursts=np.zeros((C, _hip.ETSI_MAXB, 2), np.int32),
                nblock=np.zeros(C, np.int32), blocks=np.zeros((C, _hip.ETSI_MAXJ, 4), np.int32),
                type1=np.zeros((C, _hip.ETSI_MAXJ, 268), np.uint8))


def run_lmac(hard, soft, nsym, cells=None, cell_init=None):
    """tetra_lmac_etsi with the configured cells, or tetra_lmac_etsi_acquire on cell_init (in/out)."""
    from tetraear import _hip
    c = _hip.ctx()
    C, smax = hard.shape
    o = lmac_outputs(C)
    outs = [_hip.ptr(o[k]) for k in ("nburst", "bursts", "nblock", "blocks", "type1")]
    if cell_init is not None:
        c.check(c.lib.tetra_lmac_etsi_acquire(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, smax,
                                              _hip.ptr(cell_init), *outs), "tetra_lmac_etsi_acquire")
    else:
        cells = np.ascontiguousarray(cells, np.uint32)
        c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(cells), C), "tetra_etsi_set_cells")
        c.check(c.lib.tetra_lmac_etsi(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, smax, *outs),
                "tetra_lmac_etsi")
    return o


def assert_rows_equal(out, want_rows, what=""):
    """The library's outputs against oracle row results, per channel: nburst, every burst's (start,
    kind), nblock, every block's (kind, crc_ok, burst, index) and its first n1 type-1 bits."""
    for ch, want in enumerate(want_rows):
        bursts, blocks, bits = flatten(want)
        nb, nk = int(out["nburst"][ch]), int(out["nblock"][ch])
        got_b = [tuple(int(v) for v in out["bursts"][ch, b]) for b in range(min(nb, 8))]
        assert (nb, got_b) == (len(bursts), bursts), (what, ch, nb, got_b, bursts)
        got_k = [tuple(int(v) for v in out["blocks"][ch, j]) for j in range(min(nk, 16))]
        assert (nk, got_k) == (len(blocks), blocks), (what, ch, nk, got_k, blocks)
        for j, t1 in enumerate(bits):
            assert np.array_equal(out["type1"][ch, j, :len(t1)], t1), (what, ch, j, blocks[j])


def live_outputs(out):
    """The written part of the library's outputs per channel (entries past the counts are not
    written): (bursts, blocks, type-1 bits per block)."""
    res = []
    for ch in range(len(out["nburst"])):
        nb, nk = int(out["nburst"][ch]), int(out["nblock"][ch])
        blocks = out["blocks"][ch, :nk].tolist()
        n1 = [E.KIND_PARAMS[b[0]][3] for b in blocks]
        bits = [out["type1"][ch, j, :n].tolist() for j, n in enumerate(n1)]
        res.append((out["bursts"][ch, :nb].tolist(), blocks, bits))
    return res
