"""Cell acquisition per group of rows, restated with the oracle (TEST INFRASTRUCTURE).

tetra_lmac_etsi_acquire_groups takes rows g G .. g G + G - 1 as the pieces of one carrier in time
order.  oracle_groups is its rule in terms of oracle/etsi.py alone: Receiver.sync on every row,
decode_block on every synchronisation burst's BSCH field with colour code 0, bsch_cell_init of the
last CRC-good one over the group's rows in order, then Receiver.lower_mac on every row of the group
with that init.  The rows come from tests/_lmac_rows.py's builders.
"""
import numpy as np

import etsi as E
import _lmac_rows as R

N, P, SB = R.NDB_N, R.NDB_P, R.SB


def oracle_groups(hard, soft, nsym, G, cell_init):
    """hard [C, smax], soft [C, 2 smax], nsym [C], cell_init [C / G] ->
    (per row the lower_mac result, cell_init after [C / G], ngood [C / G])."""
    C = len(nsym)
    assert G >= 1 and C % G == 0 and len(cell_init) == C // G
    rx = E.Receiver()
    bsch = E.scramble_seq(3, 120)
    rows, after, ngood = [], [], []
    for g in range(C // G):
        init, good = int(cell_init[g]), 0
        for ch in range(g * G, g * G + G):
            nd = max(int(nsym[ch]) - 1, 0)
            for s, bk in rx.sync(hard[ch, :nd]):
                if bk == E.BURST_SB:
                    t, ok = rx.decode_block(soft[ch, s + 94:s + 214], 2, bsch)
                    if ok:
                        init = E.bsch_cell_init(t)
                        good += 1
        for ch in range(g * G, g * G + G):
            nd = max(int(nsym[ch]) - 1, 0)
            rows.append(rx.lower_mac(soft[ch, :2 * nd], hard[ch, :nd], init))
        after.append(init)
        ngood.append(good)
    return rows, after, ngood


def crc_flags(want_row):
    """crc_ok of every block of one lower_mac row result, in block order."""
    return [bool(ok) for _, _, dec in want_row for _, _, ok in dec]


def row(rng, items, tail_gap=0, noise_bsch=()):
    """One row of placed bursts (R.place_bursts items) with +-127 soft bits; noise_bsch: indices of
    synchronisation bursts whose BSCH field's soft bits are replaced by noise (the CRC fails)."""
    bits, planted, _ = R.place_bursts(rng, items, tail_gap)
    soft = R.soft_of(bits)
    for i in noise_bsch:
        s, k = planted[i]
        assert k == SB
        soft[s + 94:s + 214] = rng.integers(-127, 128, 120).astype(np.int8)
    return bits, soft


def empty_row(rng, nbits=0):
    """A row without a burst: nbits random bits (< 510, so none fits)."""
    assert nbits < 510 and nbits % 2 == 0
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    return bits, R.soft_of(bits)


def pack(rows, smax=None):
    """[(bits, soft)] -> hard, soft, nsym of R.pack_rows at a width that holds the longest row."""
    if smax is None:
        smax = max(len(b) for b, _ in rows) // 2 + 3
    return R.pack_rows(rows, smax)


def run_groups(hard, soft, nsym, G, cell_init, device=False):
    """tetra_lmac_etsi_acquire_groups on host arrays (or, device=True, on device copies of them):
    (outputs dict as R.lmac_outputs, cell_init after [C / G], ngood [C / G], return code)."""
    from tetraear import _hip
    c = _hip.ctx()
    C, smax = hard.shape
    o = R.lmac_outputs(C)
    state = np.array(cell_init, np.uint32)
    ngood = np.full(len(state), -1, np.int32)
    names = ("nburst", "bursts", "nblock", "blocks", "type1")
    if device:
        import torch
        dev = torch.device("cuda", 0)
        t = {k: torch.from_numpy(v).to(dev) for k, v in o.items()}
        ins = [torch.from_numpy(a).to(dev) for a in (soft, hard, nsym)]
        ts, tg = torch.from_numpy(state.view(np.int32)).to(dev), torch.from_numpy(ngood).to(dev)
        torch.cuda.synchronize(dev)
        rc = c.lib.tetra_lmac_etsi_acquire_groups(c.handle, *[_hip.ptr(a) for a in ins], C, smax, G, _hip.ptr(ts),
                                                  _hip.ptr(tg), *[_hip.ptr(t[k]) for k in names])
        c.synchronize()
        o = {k: v.cpu().numpy() for k, v in t.items()}
        state, ngood = ts.cpu().numpy().view(np.uint32), tg.cpu().numpy()
    else:
        rc = c.lib.tetra_lmac_etsi_acquire_groups(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, smax, G,
                                                  _hip.ptr(state), _hip.ptr(ngood), *[_hip.ptr(o[k]) for k in names])
    return o, state, ngood, rc


def check_groups(hard, soft, nsym, G, cell_init, what="", device=False):
    """The library against oracle_groups: rows, cell_init and ngood.  Returns (outputs, want rows,
    cell_init after, ngood)."""
    from tetraear import _hip
    want, after, good = oracle_groups(hard, soft, nsym, G, cell_init)
    out, state, ngood, rc = run_groups(hard, soft, nsym, G, cell_init, device)
    _hip.ctx().check(rc, "tetra_lmac_etsi_acquire_groups")
    R.assert_rows_equal(out, want, what)
    assert state.tolist() == after, (what, state.tolist(), after)
    assert ngood.tolist() == good, (what, ngood.tolist(), good)
    return out, want, after, good


# ------------------------------------------------------------------------------ the hand-built cases

def case_sync_in_row(rng, where, G=3):
    """A group of G rows of one cell A, the synchronisation burst only in row `where`:
    (rows, [3], A).  Every block of every row decodes once the group knows A."""
    A, fA = R.cell_fields(rng)
    rows = []
    for r in range(G):
        if r == where:
            rows.append(row(rng, [(5, N, A, None), (2, SB, A, R.sync_payloads(rng, fA)), (0, P, A, None)], 6))
        else:
            rows.append(row(rng, [(3 + r, N, A, None), (1, P, A, None), (64, N, A, None)], 2 * r))
    return rows, [3], A


def case_two_cells(rng):
    """One group of three rows: cell A announced in row 0, cell B in row 2 (the later one wins);
    the normal bursts are scrambled with B except one of A in row 1.  (rows, [3], A, B)."""
    (A, fA), (B, fB) = R.cell_fields(rng), R.cell_fields(rng)
    rows = [row(rng, [(1, SB, A, R.sync_payloads(rng, fA)), (0, N, B, None)]),
            row(rng, [(4, N, A, None), (0, P, B, None)]),
            row(rng, [(0, P, B, None), (7, SB, B, R.sync_payloads(rng, fB)), (0, N, B, None)])]
    return rows, [3], A, B


def case_broken_after_good(rng):
    """Cell A announced in row 0; row 1 holds a synchronisation burst of cell B whose BSCH is noise
    (CRC fails): A stays.  (rows, [3], A)."""
    (A, fA), (B, fB) = R.cell_fields(rng), R.cell_fields(rng)
    rows = [row(rng, [(2, SB, A, R.sync_payloads(rng, fA)), (0, N, A, None)]),
            row(rng, [(0, P, A, None), (3, SB, A, R.sync_payloads(rng, fB)), (1, N, A, None)], noise_bsch=(1,))]
    return rows, [3], A


def case_zero_cell(rng):
    """The all-zero cell (MCC = MNC = colour code = 0): init 3, as "unknown", but ngood > 0."""
    Z = E.scramble_init(0, 0, 0)
    assert Z == 3
    rows = [row(rng, [(0, N, Z, None), (5, P, Z, None)]),
            row(rng, [(9, SB, Z, R.sync_payloads(rng, (0, 0, 0))), (0, N, Z, None)])]
    return rows, [3], Z


def random_groups(seed, NG, G):
    """NG groups of G rows for the sweep: per row 0..3 bursts of random kinds with gaps from R.GAPS,
    a synchronisation burst with probability 1/3 per burst (announcing the group's cell, or now and
    then another), a quarter of the BSCH fields noise; the soft bits of a block field now and then
    of a class from R.SOFT_CLASSES; incoming inits 3, the cell, or another cell.  Rows of up to about
    1600 bits.  Returns (rows, cell_init)."""
    rng = np.random.default_rng(seed)
    rows, inits = [], []
    for g in range(NG):
        (A, fA), (B, fB) = R.cell_fields(rng), R.cell_fields(rng)
        inits.append([3, A, B][int(rng.integers(0, 3))])
        for r in range(G):
            n = int(rng.integers(0, 4))
            if n == 0:
                rows.append(empty_row(rng, 2 * int(rng.integers(0, 200))))
                continue
            items, noise = [], []
            for i in range(n):
                k = int(rng.integers(0, 3))
                cell, fields = (A, fA) if rng.random() < 0.8 else (B, fB)
                if k == SB:
                    items.append((int(rng.choice(R.GAPS[:6])), SB, cell, R.sync_payloads(rng, fields)))
                    if rng.random() < 0.25:
                        noise.append(i)
                else:
                    items.append((int(rng.choice(R.GAPS[:6])), k, cell, None))
            bits, soft = row(rng, items, 2 * int(rng.integers(0, 8)), noise)
            if rng.random() < 0.3:   # one stretch of the row in another soft class
                cls = R.SOFT_CLASSES[int(rng.integers(0, len(R.SOFT_CLASSES)))]
                a = int(rng.integers(0, len(bits) - 216))
                soft[a:a + 216] = R.soft_class(cls, bits[a:a + 216], rng, 1)
            rows.append((bits, soft))
    return rows, inits
