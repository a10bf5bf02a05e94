"""tetra_etsi_link_quality restated in numpy (TEST INFRASTRUCTURE).

The records of include/tetra_hip.h: per burst the known bits that came out wrong and the soft bits'
strength, per CRC-good block the coded bits that disagree in sign with the re-encoded type-1 bits.
The type-5 bits come from oracle/etsi_spec.py `encode`, the independent restatement of the channel
coding, and are held against oracle/etsi.py `encode_block` on every block scored.  All integers:
the kernel is held to this model bit for bit.
"""
import functools

import numpy as np

import etsi as E
import etsi_spec as S

MAXB, MAXJ, NF = 8, 16, 4
NERR, WERR, WSUM, NZERO = range(4)
TERR, HERR, BWSUM, NSAT = range(4)
K_OF = {k: v[0] for k, v in E.KIND_PARAMS.items()}
N1_OF = {k: v[3] for k, v in E.KIND_PARAMS.items()}
TRAINING = {0: (244, E.N_BITS), 1: (244, E.P_BITS), 2: (214, E.Y_BITS)}   # burst kind -> (offset, sequence)
W_HEAD, W_TAIL = E.Q_BITS[10:22], E.Q_BITS[0:10]
POISON = -777


@functools.lru_cache(maxsize=4096)
def _type5(bits, kind, init):
    t1 = np.frombuffer(bits, np.uint8)
    c = np.asarray(S.encode(t1, kind, init), np.uint8)
    assert np.array_equal(c, E.encode_block(t1, kind, E.scramble_seq(init, K_OF[kind]))), "the two encoders differ"
    return c


def type5(type1, kind, init):
    """The K type-5 bits of a block's first n1 type-1 bits (a bit is byte & 1)."""
    t1 = np.ascontiguousarray(np.asarray(type1[:N1_OF[kind]], np.uint8) & 1)
    return _type5(t1.tobytes(), int(kind), int(init))


def block_offsets(kind, blk):
    """Bits from the burst's start to the block's K type-5 positions."""
    off = 282 if blk == 1 else 94 if kind == 2 else 14
    i = np.arange(K_OF[kind])
    return off + i + (52 if kind == 0 else 0) * (i >= 216)


def score(s, c):
    """The block record of soft values s against coded bits c."""
    s = np.asarray(s, np.int64)
    mag = np.abs(s)
    bad = (s != 0) & ((s < 0) != (np.asarray(c) == 1))
    return [int(bad.sum()), int(mag[bad].sum()), int(mag.sum()), int((s == 0).sum())]


def burst_valid(start, kind, origin, stride):
    return 0 <= kind <= 2 and origin + start >= 0 and origin + start + 510 <= 2 * stride


def link_quality(soft, hard, origin, G, cell_init, nburst, bursts, nblock, blocks, type1, bq=None, kq=None):
    """soft [C, 2 stride] int8, hard [C, stride] uint8 and a lower-MAC call's outputs -> (bq [C, 8, 4],
    kq [C, 16, 4]) int32; what the call does not write keeps bq / kq as passed (POISON when None)."""
    C, stride = hard.shape
    assert soft.shape == (C, 2 * stride) and G >= 1 and C % G == 0 and len(cell_init) == C // G and origin >= 0
    bq = np.full((C, MAXB, NF), POISON, np.int32) if bq is None else bq.copy()
    kq = np.full((C, MAXJ, NF), POISON, np.int32) if kq is None else kq.copy()
    for c in range(C):
        nb, nk = min(max(int(nburst[c]), 0), MAXB), min(max(int(nblock[c]), 0), MAXJ)
        hb = E.Receiver.hard_bits(hard[c])
        s64 = soft[c].astype(np.int64)
        for b in range(nb):
            start, kind = int(bursts[c, b, 0]), int(bursts[c, b, 1])
            if not burst_valid(start, kind, origin, stride):
                bq[c, b] = -1
                continue
            p = origin + start
            t0, seq = TRAINING[kind]
            mag = np.abs(s64[p:p + 510])
            bq[c, b] = [int((hb[p + t0:p + t0 + len(seq)] != seq).sum()),
                        int((hb[p:p + 12] != W_HEAD).sum() + (hb[p + 500:p + 510] != W_TAIL).sum()),
                        int(mag.sum()), int((mag >= 127).sum())]
        for j in range(nk):
            kind, crc, b, blk = (int(v) for v in blocks[c, j])
            ok = 0 <= kind <= 2 and 0 <= b < nb and (blk == 0 or (blk == 1 and kind == 1))
            if not ok or not burst_valid(int(bursts[c, b, 0]), int(bursts[c, b, 1]), origin, stride):
                kq[c, j] = -1
            elif crc == 0:
                kq[c, j] = [-1, 0, 0, 0]
            else:
                init = 3 if kind == 2 else int(cell_init[c // G])
                p = origin + int(bursts[c, b, 0]) + block_offsets(kind, blk)
                kq[c, j] = score(s64[p], type5(type1[c, j], kind, init))
    return bq, kq


def call(soft, hard, origin, G, cell_init, o, bq=None, kq=None, device=False, ctx=None):
    """tetra_etsi_link_quality on host arrays, or on device copies of them: (rc, bq, kq).  o: the
    lower-MAC call's outputs as _lmac_rows.lmac_outputs; bq / kq: what the outputs hold before."""
    from tetraear import _hip
    c = ctx if ctx is not None else _hip.ctx()
    C, stride = hard.shape
    bq = np.full((C, MAXB, NF), POISON, np.int32) if bq is None else bq.copy()
    kq = np.full((C, MAXJ, NF), POISON, np.int32) if kq is None else kq.copy()
    ci = None if cell_init is None else np.ascontiguousarray(cell_init, np.uint32)
    args = [soft, hard, None if ci is None else ci.view(np.int32), o["nburst"], o["bursts"], o["nblock"], o["blocks"],
            o["type1"], bq, kq]
    if device:
        import torch
        dev = torch.device("cuda", 0)
        args = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args]
        torch.cuda.synchronize(dev)
    p = [_hip.ptr(a) for a in args]
    rc = c.lib.tetra_etsi_link_quality(c.handle, p[0], p[1], C, stride, origin, G, *p[2:])
    if device:
        c.synchronize()
        bq, kq = args[8].cpu().numpy(), args[9].cpu().numpy()
    return rc, bq, kq


def oracle_outputs(want_rows):
    """Oracle row results (_lmac_rows.oracle_rows) in the library's output layout, poison past the counts."""
    import _lmac_rows as R
    C = len(want_rows)
    o = dict(nburst=np.zeros(C, np.int32), bursts=np.full((C, MAXB, 2), POISON, np.int32),
             nblock=np.zeros(C, np.int32), blocks=np.full((C, MAXJ, 4), POISON, np.int32),
             type1=np.full((C, MAXJ, 268), 0xA5, np.uint8))
    for c, want in enumerate(want_rows):
        bursts, blocks, bits = R.flatten(want)
        o["nburst"][c], o["nblock"][c] = len(bursts), len(blocks)
        for b, v in enumerate(bursts):
            o["bursts"][c, b] = v
        for j, (v, t1) in enumerate(zip(blocks, bits)):
            o["blocks"][c, j] = v
            o["type1"][c, j, :len(t1)] = t1
    return o


# ------------------------------------------------------------------------------ built rows

FLIP_STEP = 48   # type-5 positions between planted sign flips


@functools.lru_cache(maxsize=None)
def built_rows():
    """Rows of placed bursts (tests/_lmac_rows.py) whose records are known without the model:
    dict(hard, soft, nsym, cells [C], planted per row, jobs per row, expect [(row, 'b' / 'k', index,
    field, value)]).  Rows 0, 1: clean at amplitudes 127 and 64.  Rows 2..7: e = 1, 2, 3 sign flips
    FLIP_STEP type-5 positions apart in one block of each kind, at amplitudes 64 and 127.  Row 8:
    training, head and tail bits flipped within the scan's thresholds.  Row 9: zeroed soft bytes, and
    SCH/F's gap at type-5 position 216."""
    import _lmac_rows as R
    rng = np.random.default_rng(2024)
    N, P, SB = R.NDB_N, R.NDB_P, R.SB
    rows, cells, planted_all, jobs_all, expect = [], [], [], [], []

    def add(items_kinds, amp, cell=None):
        cell = R.random_cell(rng) if cell is None else cell
        bits, planted, jobs = R.place_bursts(rng, [(int(rng.integers(0, 9)), k, cell, None) for k in items_kinds],
                                             int(rng.integers(0, 7)))
        rows.append([bits, R.soft_of(bits, amp)])
        cells.append(cell)
        planted_all.append(planted)
        jobs_all.append(jobs)
        return len(rows) - 1, planted

    def slot(kinds, b, blk):   # block slot of (burst b, block blk): 1 block per NDB(n), 2 per NDB(p) / SB
        return sum(1 if k == N else 2 for k in kinds[:b]) + blk

    for amp in (127, 64):
        kinds = [N, SB, P]
        r, planted = add(kinds, amp)
        for b, (s, k) in enumerate(planted):
            expect += [(r, "b", b, f, v) for f, v in ((TERR, 0), (HERR, 0), (BWSUM, 510 * amp),
                                                      (NSAT, 510 if amp >= 127 else 0))]
            for blk, (kind, _) in enumerate(jobs_all[r][b]):
                expect += [(r, "k", slot(kinds, b, blk), f, v)
                           for f, v in ((NERR, 0), (WERR, 0), (WSUM, K_OF[kind] * amp), (NZERO, 0))]
    for amp in (64, 127):
        for e in (1, 2, 3):
            kinds = [P, N, SB]
            r, planted = add(kinds, amp)
            for b, blk, kind in ((0, 1, 1), (1, 0, 0), (2, 0, 2)):
                i0 = int(rng.integers(0, K_OF[kind] - FLIP_STEP * (e - 1)))
                pos = planted[b][0] + block_offsets(kind, blk)[i0 + FLIP_STEP * np.arange(e)]
                rows[r][1][pos] = -rows[r][1][pos]
                j = slot(kinds, b, blk)
                expect += [(r, "k", j, NERR, e), (r, "k", j, WERR, e * amp), (r, "k", j, WSUM, K_OF[kind] * amp),
                           (r, "k", j, NZERO, 0)]
    # scored bits flipped: NDB 4 of 44 may differ, SB 6 of 60
    kinds = [N, P, SB]
    r, planted = add(kinds, 127)
    for b, (train, edge) in enumerate(((4, 0), (2, 2), (3, 3))):
        s, k = planted[b]
        t0, seq = TRAINING[k]
        pos = np.concatenate([t0 + rng.choice(len(seq), train, replace=False),
                              rng.choice(np.r_[0:12, 500:510], edge, replace=False)]).astype(np.int64)
        rows[r][0][s:s + 510] = R.flip_scored(rows[r][0][s:s + 510], k, pos)
        expect += [(r, "b", b, TERR, train), (r, "b", b, HERR, edge), (r, "b", b, BWSUM, 510 * 127)]
    # zeros: five in an SCH/HD block; one either side of SCH/F's gap (type-5 215 at burst bit 229, 216
    # at 282), two inside the gap (not the block's)
    kinds = [P, N]
    r, planted = add(kinds, 100)
    s0, s1 = planted[0][0], planted[1][0]
    rows[r][1][s0 + block_offsets(1, 0)[[3, 50, 99, 150, 215]]] = 0
    rows[r][1][[s1 + 229, s1 + 282, s1 + 230, s1 + 281]] = 0
    expect += [(r, "k", 0, NZERO, 5), (r, "k", 0, WSUM, 211 * 100), (r, "k", 0, NERR, 0), (r, "k", 1, NZERO, 0),
               (r, "k", 2, NZERO, 2), (r, "k", 2, WSUM, 430 * 100), (r, "k", 2, NERR, 0),
               (r, "b", 0, BWSUM, 505 * 100), (r, "b", 1, BWSUM, 506 * 100), (r, "b", 1, NSAT, 0)]
    smax = max(len(b) for b, _ in rows) // 2 + 3
    hard, soft, nsym = R.pack_rows([(b, s) for b, s in rows], smax)
    return dict(hard=hard, soft=soft, nsym=nsym, cells=np.array(cells, np.uint32), planted=planted_all,
                jobs=jobs_all, expect=expect)
