"""The lower MAC's cell vote restated with the oracle (TEST INFRASTRUCTURE).

tetra_lmac_etsi_vote_groups / _stream_vote (include/tetra_hip.h carries the rule): every CRC-good
BSCH of a group is a ballot (c_i, w_i) -- the init its type-1 bits announce, and the correlation of
its 120 soft bytes with the re-encoded codeword, max(1, WSUM - 2 WERR) -- the cell kept so far
defends with its score, the largest total wins, and the winner's score is its margin, capped.
`vote` is that rule on plain Python integers; oracle_vote_groups finds the ballots with
oracle/etsi.py (Receiver.sync, decode_block, bsch_cell_init) and weighs them with
tests/_etsi_quality_model.py (type5, score), then decodes every row with the winner as
tests/_lmac_groups.py oracle_groups does.  VoteStream is the same over oracle.etsi.LmacStream.
The kernel is held to this model exactly.
"""
import numpy as np

import etsi as E
import _etsi_quality_model as Q
import _lmac_groups as GR
import _lmac_rows as R

N, P, SB = R.NDB_N, R.NDB_P, R.SB
CAP = 8 * 120 * 127   # TETRA_ETSI_VOTE_CAP_DEFAULT
FULL = 120 * 127      # a BSCH block at full scale
BSCH_SCR = E.scramble_seq(3, 120)


def weight(soft120, type1):
    """w of one CRC-good BSCH: its soft bytes against its own type-1 bits re-encoded (kind 2, init 3)."""
    rec = Q.score(soft120, Q.type5(type1, 2, 3))
    return max(1, rec[Q.WSUM] - 2 * rec[Q.WERR])


def vote(cell, score, ballots, cap):
    """The rule: (cell, score) in, ballots [(c_i, w_i)] in order -> (cell, score, agree) out."""
    assert cap > 0
    if not ballots:
        return int(cell), int(score), 0
    cell = int(cell)
    T = {cell: max(int(score), 0)}
    last = {}
    for i, (c, w) in enumerate(ballots):
        T[c] = T.get(c, 0) + int(w)
        last[c] = i
    top = max(T.values())
    tied = [c for c in T if T[c] == top]
    win = cell if cell in tied else max(tied, key=lambda c: last[c])
    others = sum(v for c, v in T.items() if c != win)
    return win, min(int(cap), max(1, T[win] - others)), sum(1 for c, _ in ballots if c == win)


def row_ballots(rx, hard_row, soft_row, bursts):
    """The ballots of one row's bursts [(row bit, kind)] in order."""
    out = []
    for s, bk in bursts:
        if bk == E.BURST_SB:
            t, ok = rx.decode_block(soft_row[s + 94:s + 214], 2, BSCH_SCR)
            if ok:
                out.append((E.bsch_cell_init(t), weight(soft_row[s + 94:s + 214], t)))
    return out


def oracle_vote_groups(hard, soft, nsym, G, cell_init, score, cap):
    """hard [C, smax], soft [C, 2 smax], nsym [C], cell_init / score [C / G] -> (per row the lower_mac
    result, cell_init after, score after, ngood, agree, the ballots per group)."""
    C = len(nsym)
    assert G >= 1 and C % G == 0 and len(cell_init) == C // G == len(score)
    rx = E.Receiver()
    rows, cells, scores, ngood, agree, ballots = [], [], [], [], [], []
    for g in range(C // G):
        bl = []
        for ch in range(g * G, g * G + G):
            nd = max(int(nsym[ch]) - 1, 0)
            bl += row_ballots(rx, hard[ch], soft[ch], rx.sync(hard[ch, :nd]))
        c, s, a = vote(cell_init[g], score[g], bl, cap)
        for ch in range(g * G, g * G + G):
            nd = max(int(nsym[ch]) - 1, 0)
            rows.append(rx.lower_mac(soft[ch, :2 * nd], hard[ch, :nd], c))
        cells.append(c)
        scores.append(s)
        ngood.append(len(bl))
        agree.append(a)
        ballots.append(bl)
    return rows, cells, scores, ngood, agree, ballots


class VoteStream:
    """tetra_lmac_etsi_stream_vote for one channel: oracle.etsi.LmacStream with the chunk's cell chosen
    by the vote over the row it is about to decode (the carried tail in front of the new dibits)."""

    def __init__(self, rx=None, cap=CAP, cell=3, score=0):
        self.m = E.LmacStream(rx, cell_init=cell)   # a given cell: push decodes with m.cell as it stands
        self.cap, self.score, self.agree, self.ngood = cap, score, 0, 0

    @property
    def cell(self):
        return self.m.cell

    def push(self, hard, soft):
        m = self.m
        row_h = np.concatenate([m.tail_hard, np.asarray(hard, np.uint8)])
        row_s = np.concatenate([m.tail_soft, np.asarray(soft, np.int8)])
        bursts, _ = m.rx.sync_from(row_h, m.phase, m.maxb)
        bl = row_ballots(m.rx, row_h, row_s, bursts)
        m.cell, self.score, self.agree = vote(m.cell, self.score, bl, self.cap)
        self.ngood = len(bl)
        return m.push(hard, soft)


# ------------------------------------------------------------------------------ soft amplitudes, rows

def scale_burst(soft, start, amp):
    """One burst's soft bytes (510 from row bit `start`) scaled to +-amp, signs kept (in place)."""
    v = soft[start:start + 510]
    soft[start:start + 510] = (np.sign(v.astype(np.int32)) * amp).astype(np.int8)


def row(rng, items, tail_gap=0, amps=None, noise_bsch=()):
    """_lmac_groups.row with burst i's soft bytes at +-amps[i] (None: 127): (bits, soft)."""
    bits, planted, _ = R.place_bursts(rng, items, tail_gap)
    soft = R.soft_of(bits)
    for i, (s, k) in enumerate(planted):
        if amps is not None and amps[i] is not None:
            scale_burst(soft, s, amps[i])
        if i in noise_bsch:
            soft[s + 94:s + 214] = rng.integers(-127, 128, 120).astype(np.int8)
    return bits, soft


def sync_item(rng, announce, scrambled_with=None, gap=0):
    """A place_bursts item: a synchronisation burst whose BSCH announces cell `announce` = (init,
    fields), its second block scrambled with `scrambled_with` (an init; None: the announced cell's)."""
    init, fields = announce
    return (gap, SB, init if scrambled_with is None else scrambled_with, R.sync_payloads(rng, fields))


def case_ballots(rng, order, amps=None, normal_with=0):
    """One group of one row per ballot: row i holds a synchronisation burst announcing cell
    order[i] (an index into the two or three random cells returned) at amplitude amps[i], then a normal
    burst; every block but the BSCH is scrambled with cell `normal_with`.  (rows, cells [(init, fields)])."""
    cells = [R.cell_fields(rng) for _ in range(max(order) + 1)]
    assert len({c[0] for c in cells}) == len(cells)
    use = cells[normal_with][0]
    rows = []
    for i, k in enumerate(order):
        a = None if amps is None else amps[i]
        rows.append(row(rng, [sync_item(rng, cells[k], use, gap=2 * i + 1), (i % 3, (N, P)[i & 1], use, None)],
                        2 * (i % 4), amps=[a, None]))
    return rows, cells


def case_foreign_last(rng):
    """Foreign last: three full-strength BSCH of cell A in rows 0..2, then one of cell B at a third of
    the amplitude in row 3, all CRC-good; every other block scrambled with A.  (rows, A, B) inits."""
    rows, cells = case_ballots(rng, [0, 0, 0, 1], [127, 127, 127, 42])
    return rows, cells[0][0], cells[1][0]


def random_vote_groups(seed, NG, G):
    """_lmac_groups.random_groups with a random amplitude per burst (1 .. 127, a quarter at 127), random
    incoming scores (0, small, about a block, at the cap, negative): (rows, inits, scores)."""
    rows, inits = GR.random_groups(seed, NG, G)
    rng = np.random.default_rng(seed + 77)
    rx = E.Receiver()
    out = []
    for bits, soft in rows:
        soft = soft.copy()
        for s, _ in rx.sync(R.hard_of(bits)) if len(bits) >= 510 else []:
            if rng.random() < 0.75:
                scale_burst(soft, s, int(rng.integers(1, 128)))
        out.append((bits, soft))
    scores = [int(rng.choice([0, 0, 5, 900, FULL, 3 * FULL, CAP, -17])) for _ in range(NG)]
    return out, inits, scores


# ------------------------------------------------------------------------------ the library's calls

NAMES = ("nburst", "bursts", "nblock", "blocks", "type1")
POISON = -777


def poisoned_outputs(C):
    """The lower MAC's outputs filled with poison: nothing past a count may be relied on or written."""
    o = R.lmac_outputs(C)
    for k in ("bursts", "blocks"):
        o[k][:] = POISON
    o["type1"][:] = 0xA5
    return o


def run_vote_groups(hard, soft, nsym, G, cell_init, score, cap=CAP, device=False, soft_off=0):
    """tetra_lmac_etsi_vote_groups on host arrays (or device copies): (outputs, cell_init, score, ngood,
    agree, return code).  soft_off (device only; host rows are staged to aligned memory): the soft rows
    start that many bytes off an aligned address."""
    from tetraear import _hip
    c = _hip.ctx()
    C, smax = hard.shape
    NG = len(cell_init)
    o = poisoned_outputs(C)
    state = np.array(cell_init, np.uint32)
    sc = np.array(score, np.int32)
    ngood, agree = np.full(NG, POISON, np.int32), np.full(NG, POISON, np.int32)
    if device:
        import torch
        dev = torch.device("cuda", 0)
        t = {k: torch.from_numpy(v).to(dev) for k, v in o.items()}
        sbuf = torch.zeros(soft.size + 64, dtype=torch.int8, device=dev)
        ts = sbuf[soft_off:soft_off + soft.size]
        ts.copy_(torch.from_numpy(np.ascontiguousarray(soft).reshape(-1)))
        ins = [ts, torch.from_numpy(hard).to(dev), torch.from_numpy(nsym).to(dev)]
        small = [torch.from_numpy(a).to(dev) for a in (state.view(np.int32), sc, ngood, agree)]
        torch.cuda.synchronize(dev)
        rc = c.lib.tetra_lmac_etsi_vote_groups(c.handle, *[_hip.ptr(a) for a in ins], C, smax, G, cap,
                                               *[_hip.ptr(a) for a in small], *[_hip.ptr(t[k]) for k in NAMES])
        c.synchronize()
        o = {k: v.cpu().numpy() for k, v in t.items()}
        state, sc, ngood, agree = (a.cpu().numpy() for a in small)
        state = state.view(np.uint32)
    else:
        assert soft_off == 0
        rc = c.lib.tetra_lmac_etsi_vote_groups(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, smax, G, cap,
                                               _hip.ptr(state), _hip.ptr(sc), _hip.ptr(ngood), _hip.ptr(agree),
                                               *[_hip.ptr(o[k]) for k in NAMES])
    return o, state, sc, ngood, agree, rc


def check_vote_groups(hard, soft, nsym, G, cell_init, score, cap=CAP, what="", device=False, soft_off=0):
    """The library against oracle_vote_groups: rows, cell_init, score, ngood, agree.  Returns (outputs,
    want rows, cells, scores, ngood, agree, ballots)."""
    from tetraear import _hip
    want = oracle_vote_groups(hard, soft, nsym, G, cell_init, score, cap)
    out, state, sc, ngood, agree, rc = run_vote_groups(hard, soft, nsym, G, cell_init, score, cap, device, soft_off)
    _hip.ctx().check(rc, "tetra_lmac_etsi_vote_groups")
    R.assert_rows_equal(out, want[0], what)
    got = (state.tolist(), sc.tolist(), ngood.tolist(), agree.tolist())
    assert got == tuple(want[1:5]), (what, got, want[1:])
    return (out,) + want
