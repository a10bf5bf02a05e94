"""tetra_lmac_etsi_vote_groups / _stream_vote (k_cell_vote_groups between the BSCH pass and the SCH pass
of the production trellis) on rows built on the CPU: every case against tests/_lmac_vote.py
oracle_vote_groups / VoteStream -- nburst, every burst, nblock, every block and its type-1 bits
(assert_rows_equal), cell_init, score, ngood and agree.  Integer and bit-exact: no tolerance anywhere.
tests/test_lmac_vote_model.py proves on the CPU that the model and the built cases mean what is
assumed here.  Then the Python surface on the smallest wideband capture
tests/test_gpu_wideband_acquire.py uses.
"""
import numpy as np
import pytest

import etsi as E
import _lmac_groups as GR
import _lmac_rows as R
import _lmac_vote as V

pytestmark = pytest.mark.gpu

N, P, SB = R.NDB_N, R.NDB_P, R.SB


def _poison_kept(out):
    """Entries past the counts are as the caller left them: nothing is written there."""
    for ch in range(len(out["nburst"])):
        nb, nk = int(out["nburst"][ch]), int(out["nblock"][ch])
        assert np.all(out["bursts"][ch, nb:] == V.POISON) and np.all(out["blocks"][ch, nk:] == V.POISON), ch
        assert np.all(out["type1"][ch, nk:] == 0xA5), ch


@pytest.mark.parametrize("G,NG", [(1, 67), (3, 1), (3, 5), (3, 67), (32, 5)])
def test_group_shapes(G, NG):
    """Groups of 1, 3 and 32 rows; 1, 5 and 67 groups (a partial workgroup of four waves): random rows,
    amplitudes, incoming cells and scores.  Host pointers, and for five groups device pointers, where
    the outputs hold poison past every count before and after (host outputs are staged: what lies
    past a count there is unspecified)."""
    rows, inits, scores = V.random_vote_groups(100 * G + NG, NG, G)
    hard, soft, nsym = GR.pack(rows)
    res = V.check_vote_groups(hard, soft, nsym, G, inits, scores, what="G %d, %d groups" % (G, NG), device=NG == 5)
    if NG == 5:
        _poison_kept(res[0])
    assert sum(res[4]) > 0


def test_many_ballots_in_one_group():
    """G = 32 with three synchronisation bursts per row: 96 ballots in a group (more than a wave has
    lanes), three cells at random amplitudes, a second group beside it."""
    rng = np.random.default_rng(11)
    cells = [R.cell_fields(rng) for _ in range(3)]
    rows = []
    for r in range(64):
        ks = rng.integers(0, 3, 3)
        items = [V.sync_item(rng, cells[k], cells[0][0], gap=int(rng.integers(0, 4))) for k in ks]
        rows.append(V.row(rng, items, 2, amps=[int(a) for a in rng.integers(1, 128, 3)]))
    hard, soft, nsym = GR.pack(rows)
    res = V.check_vote_groups(hard, soft, nsym, 32, [cells[2][0], 3], [V.FULL, 0], what="96 ballots")
    assert res[4] == [96, 96] and len({c for c, _ in res[6][0]}) == 3


def test_short_rows_and_a_full_burst_table():
    """Rows with nsym 0 and 1 inside a group, and a row of 8 bursts (ETSI_MAXB, 16 blocks) of which
    four are synchronisation bursts of two cells."""
    rng = np.random.default_rng(12)
    A, B = R.cell_fields(rng), R.cell_fields(rng)
    full = [(0, N, A[0], None), V.sync_item(rng, A), (0, P, A[0], None), V.sync_item(rng, B, A[0]),
            V.sync_item(rng, A), (0, N, A[0], None), (0, P, A[0], None), V.sync_item(rng, B, A[0])]
    rows = [GR.empty_row(rng), V.row(rng, [V.sync_item(rng, A, gap=2), (0, P, A[0], None)]),
            GR.empty_row(rng), V.row(rng, [(4, N, A[0], None)]),
            V.row(rng, [(0, N, A[0], None)]), V.row(rng, full, amps=[None, 90, None, 127, 60, None, None, 20]),
            GR.empty_row(rng, 100), V.row(rng, [(1, P, A[0], None)])]
    hard, soft, nsym = GR.pack(rows, 2050)
    nsym[0], nsym[2] = 0, 1
    out, want, cells, scores, good, agree, _ = V.check_vote_groups(hard, soft, nsym, 4, [3, 3], [0, 0], what="short, full")
    assert cells == [A[0], A[0]] and good == [1, 4] and agree == [1, 2]
    assert scores == [V.FULL, 120 * (90 + 60 - 127 - 20)]
    assert int(out["nburst"][5]) == 8 and int(out["nblock"][5]) == 14
    assert all(all(GR.crc_flags(w)) for w in want)


def test_device_pointers_give_the_host_pointers_outputs():
    rows, inits, scores = V.random_vote_groups(60, 9, 3)
    hard, soft, nsym = GR.pack(rows)
    host = V.check_vote_groups(hard, soft, nsym, 3, inits, scores, what="host pointers")
    dev = V.check_vote_groups(hard, soft, nsym, 3, inits, scores, what="device pointers", device=True)
    assert R.live_outputs(host[0]) == R.live_outputs(dev[0])
    _poison_kept(dev[0])


@pytest.mark.parametrize("off,cap", [(1, V.CAP), (2, 2000), (3, V.CAP)])
def test_random_sweep_on_unaligned_soft_rows(off, cap):
    """About 40 seeded random groups on device soft rows that start 1, 2 or 3 bytes off a dword, two
    values of cap; the state is carried into a second call on other rows."""
    rows, inits, scores = V.random_vote_groups(2000 + off, 14, 3)
    hard, soft, nsym = GR.pack(rows)
    scores = [min(s, cap) for s in scores]
    res = V.check_vote_groups(hard, soft, nsym, 3, inits, scores, cap, "sweep", device=True, soft_off=off)
    rows2, _, _ = V.random_vote_groups(2500 + off, 14, 3)
    h2, s2, n2 = GR.pack(rows2)
    V.check_vote_groups(h2, s2, n2, 3, res[2], res[3], cap, "sweep, second call", device=True, soft_off=off)


def test_foreign_last():
    """Three full-strength BSCH of cell A, then one of cell B at a third of the amplitude, all CRC-good,
    the normal bursts scrambled with A.  tetra_lmac_etsi_acquire_groups returns B and the A-scrambled
    blocks fail (the rows plant what is claimed); the vote returns A and they pass."""
    rng = np.random.default_rng(7)
    rows, A, B = V.case_foreign_last(rng)
    hard, soft, nsym = GR.pack(rows)
    out, state, ngood, rc = GR.run_groups(hard, soft, nsym, 4, [3])
    assert rc == 0 and state.tolist() == [B] and ngood.tolist() == [4]
    sch = lambda o: [bool(o["blocks"][ch, j, 1]) for ch in range(4) for j in range(int(o["nblock"][ch]))
                     if o["blocks"][ch, j, 0] != 2]
    bsch = lambda o: [bool(o["blocks"][ch, j, 1]) for ch in range(4) for j in range(int(o["nblock"][ch]))
                      if o["blocks"][ch, j, 0] == 2]
    assert len(sch(out)) == 2 + 3 + 2 + 3 and not any(sch(out)) and bsch(out) == [True] * 4
    out, want, cells, scores, good, agree, _ = V.check_vote_groups(hard, soft, nsym, 4, [3], [0], what="foreign last")
    assert (cells, good, agree) == ([A], [4], [3]) and scores == [3 * V.FULL - 120 * 42]
    assert all(sch(out)) and bsch(out) == [True] * 4


def test_ballot_order_and_incumbency():
    """A then B: B (tie, latest); A, A, B: A; an incumbent A at the cap outlasts B's ballots until its
    score is worn below one of them; a negative score reads as 0."""
    rng = np.random.default_rng(6)
    rows, cells = V.case_ballots(rng, [0, 1])
    hard, soft, nsym = GR.pack(rows)
    assert V.check_vote_groups(hard, soft, nsym, 2, [3], [0], what="A, B")[2] == [cells[1][0]]
    rows, cells = V.case_ballots(rng, [0, 0, 1])
    hard, soft, nsym = GR.pack(rows)
    assert V.check_vote_groups(hard, soft, nsym, 3, [3], [0], what="A, A, B")[2] == [cells[0][0]]
    rows, cells = V.case_ballots(rng, [1, 1], normal_with=1)
    A, B = cells[0][0], cells[1][0]
    hard, soft, nsym = GR.pack(rows)
    state, score, seen = [A, A], [2 * V.FULL + 10, -5], []
    for k in range(3):
        res = V.check_vote_groups(hard[:2], soft[:2], nsym[:2], 1, state, score, 2 * V.FULL + 10, "call %d" % k)
        state, score = res[2], res[3]
        seen.append((state, score))
    assert seen == [([A, B], [V.FULL + 10, V.FULL]), ([A, B], [10, 2 * V.FULL]), ([B, B], [V.FULL - 10, 2 * V.FULL + 10])]


def test_error_returns_write_nothing():
    rng = np.random.default_rng(51)
    rows, _, A = GR.case_sync_in_row(rng, 1)
    rows = rows + rows[:2]
    hard, soft, nsym = GR.pack(rows)
    bad = [(2, V.CAP), (3, V.CAP), (0, V.CAP), (5, 0), (5, -1)]   # C % G != 0, G == 0, cap <= 0
    for G, cap in bad:
        out, state, sc, ngood, agree, rc = V.run_vote_groups(hard, soft, nsym, G, [3, 7], [1, 2], cap)
        assert rc == -1, (G, cap)
        assert (state.tolist(), sc.tolist(), ngood.tolist(), agree.tolist()) == ([3, 7], [1, 2], [V.POISON] * 2, [V.POISON] * 2)
        assert np.all(out["nburst"] == 0) and np.all(out["bursts"] == V.POISON)
    # G > 32 (33 rows, one group); 32 is served
    rows33 = [GR.empty_row(rng, 20) for _ in range(32)] + [rows[1]]
    h, s, n = GR.pack(rows33)
    assert V.run_vote_groups(h, s, n, 33, [3], [0])[5] == -1
    out, state, sc, ngood, agree, rc = V.run_vote_groups(h[1:], s[1:], n[1:], 32, [3], [0])
    assert (rc, state.tolist(), sc.tolist(), ngood.tolist(), agree.tolist()) == (0, [A], [V.FULL], [1], [1])
    # NULL cell_init / score / ngood / agree; what tetra_lmac_etsi refuses (a row too long)
    from tetraear import _hip
    c = _hip.ctx()
    C, smax = hard.shape
    o = V.poisoned_outputs(C)
    st, sc, ng, ag = np.array([3], np.uint32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    outs = [_hip.ptr(o[k]) for k in V.NAMES]
    ins = [_hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym)]
    for k in range(4):
        small = [_hip.ptr(a) for a in (st, sc, ng, ag)]
        small[k] = None
        assert c.lib.tetra_lmac_etsi_vote_groups(c.handle, *ins, C, smax, 5, V.CAP, *small, *outs) == -1, k
    assert c.lib.tetra_lmac_etsi_vote_groups(c.handle, *ins, C, 4000, 5, V.CAP, _hip.ptr(st), _hip.ptr(sc), _hip.ptr(ng),
                                             _hip.ptr(ag), *outs) == -1
    # the streaming form: NULL cell_init or score, cap <= 0, rows that alias half
    R_ = _hip.ETSI_RESERVE
    srow, hrow = np.zeros((1, 2 * 900), np.int8), np.zeros((1, 900), np.uint8)
    lead, ns = np.full(1, 2 * R_, np.int32), np.ones(1, np.int32)
    def stream(cap, ci, s_, nsoft=srow, nhard=hrow, stride=900):
        return c.lib.tetra_lmac_etsi_stream_vote(c.handle, _hip.ptr(srow), _hip.ptr(hrow), _hip.ptr(ns), 1, stride,
                                                 _hip.ptr(lead), _hip.ptr(nsoft), _hip.ptr(nhard), cap, ci, s_, None,
                                                 *[_hip.ptr(V.poisoned_outputs(1)[k]) for k in V.NAMES])
    assert stream(V.CAP, None, _hip.ptr(sc)) == -1 and stream(V.CAP, _hip.ptr(st), None) == -1
    assert stream(0, _hip.ptr(st), _hip.ptr(sc)) == -1 and stream(V.CAP, _hip.ptr(st), _hip.ptr(sc), stride=R_) == -1
    assert stream(V.CAP, _hip.ptr(st), _hip.ptr(sc), nsoft=np.zeros_like(srow)) == -1
    assert stream(V.CAP, _hip.ptr(st), _hip.ptr(sc)) == 0 and (st.tolist(), sc.tolist()) == ([3], [0])


def test_table_follows_the_state_after_configured_cells():
    """One context: a vote acquires A; tetra_etsi_set_cells + tetra_lmac_etsi with other cells rewrite the
    scrambler table; a vote without a synchronisation burst on the old state decodes with A again."""
    rng = np.random.default_rng(52)
    rows, init, A = GR.case_sync_in_row(rng, 1)
    hard, soft, nsym = GR.pack(rows)
    res = V.check_vote_groups(hard, soft, nsym, 3, init, [0], what="first vote")
    assert res[2] == [A] and res[3] == [V.FULL]
    B, _ = R.cell_fields(rng)
    rows_b = [GR.row(rng, [(r, N, B, None), (0, P, B, None)]) for r in range(3)]
    hb, sb, nb = GR.pack(rows_b, hard.shape[1])
    cells = np.full(3, B, np.uint32)
    R.assert_rows_equal(R.run_lmac(hb, sb, nb, cells), R.oracle_rows(hb, sb, nb, cells), "configured cells")
    rows_a = [GR.row(rng, [(2 * r, P, A, None), (1, N, A, None)]) for r in range(3)]
    ha, sa, na = GR.pack(rows_a, hard.shape[1])
    res = V.check_vote_groups(ha, sa, na, 3, res[2], res[3], what="second vote")
    assert res[2] == [A] and res[3] == [V.FULL] and res[4] == [0] and all(all(GR.crc_flags(w)) for w in res[1])


@pytest.mark.parametrize("alias", [True, False], ids=["same_rows", "other_rows"])
def test_stream_vote_carries_the_score(alias):
    """Three chunks (and an empty one) through tetra_lmac_etsi_stream_vote against VoteStream on the whole
    stream: channel 0's first synchronisation burst straddles the first seam in its BSCH field, so it
    votes with soft bytes carried in the tail; its second one announces another cell at a lower
    amplitude and loses to the carried score.  Channel 1 hears the other cell twice in one chunk after
    a weak ballot for the first: it changes cell.  Channel 2 hears nothing."""
    from tetraear import _hip
    c = _hip.ctx()
    rng = np.random.default_rng(9)
    A, B = R.cell_fields(rng), R.cell_fields(rng)
    chans = []
    bits, planted, _ = R.place_bursts(rng, [(3, N, A[0], None), V.sync_item(rng, A), (1, P, A[0], None),
                                            V.sync_item(rng, B, A[0]), (0, N, A[0], None)])
    soft = R.soft_of(bits)
    V.scale_burst(soft, planted[3][0], 50)
    hard = R.hard_of(bits)
    chans.append((hard, soft, R.cuts_at(len(hard), [(planted[1][0] + 150) // 2, (planted[3][0] - 40) // 2])))
    bits, planted, _ = R.place_bursts(rng, [V.sync_item(rng, A, gap=5), (0, N, A[0], None), V.sync_item(rng, B),
                                            V.sync_item(rng, B), (2, P, B[0], None)])
    soft = R.soft_of(bits)
    V.scale_burst(soft, planted[0][0], 9)
    hard = R.hard_of(bits)
    chans.append((hard, soft, R.cuts_at(len(hard), [400, (planted[2][0] - 10) // 2])))
    bits, _, _ = R.place_bursts(rng, [(7, N, A[0], None), (0, P, A[0], None)])
    chans.append((R.hard_of(bits), R.soft_of(bits), R.cuts_at(len(bits) // 2, [300, 500])))
    C, RES, stride = len(chans), _hip.ETSI_RESERVE, 2048
    bufs = [(np.zeros((C, 2 * stride), np.int8), np.zeros((C, stride), np.uint8)) for _ in range(1 if alias else 2)]
    lead = np.full(C, 2 * RES, np.int32)
    cell, score = np.full(C, 3, np.uint32), np.zeros(C, np.int32)
    models = [V.VoteStream(E.Receiver()) for _ in chans]
    trace = []
    for k in range(4):
        soft, hard = bufs[k % len(bufs)]
        nsoft, nhard = bufs[(k + 1) % len(bufs)]
        nsym = np.ones(C, np.int32)
        new = []
        for ch, (h, s, cuts) in enumerate(chans):
            at, n = cuts[k] if k < len(cuts) else (len(h), 0)
            hard[ch, RES:RES + n] = h[at:at + n]
            soft[ch, 2 * RES:2 * (RES + n)] = s[2 * at:2 * (at + n)]
            nsym[ch] = n + 1
            new.append((h[at:at + n], s[2 * at:2 * (at + n)]))
        o = V.poisoned_outputs(C)
        agree = np.full(C, V.POISON, np.int32)
        c.check(c.lib.tetra_lmac_etsi_stream_vote(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, stride,
                                                  _hip.ptr(lead), _hip.ptr(nsoft), _hip.ptr(nhard), V.CAP, _hip.ptr(cell),
                                                  _hip.ptr(score), _hip.ptr(agree), *[_hip.ptr(o[n_]) for n_ in V.NAMES]),
                "tetra_lmac_etsi_stream_vote")
        want = [m.push(nh, ns)["bursts"] for m, (nh, ns) in zip(models, new)]
        R.assert_rows_equal(o, want, "stream chunk %d" % k)
        for ch, m in enumerate(models):
            T = len(m.m.tail_hard)
            assert int(lead[ch]) == 2 * (RES - T) + m.m.phase, (k, ch)
            assert np.array_equal(nsoft[ch, 2 * (RES - T):2 * RES], m.m.tail_soft), (k, ch)
        got = (cell.tolist(), score.tolist(), agree.tolist())
        assert got == ([m.cell for m in models], [m.score for m in models], [m.agree for m in models]), (k, got)
        trace.append((int(cell[0]), int(score[0]), int(cell[1]), int(score[1])))
    assert trace[0][:2] == (3, 0) and trace[1][:2] == (A[0], V.FULL) and trace[3][:2] == (A[0], V.FULL - 6000)
    assert trace[0][2:] == (A[0], 120 * 9) and trace[3][2:] == (B[0], 2 * V.FULL - 120 * 9)
    assert (int(cell[2]), int(score[2])) == (3, 0)


# ------------------------------------------------------------------------------ the Python surface

def _views(frames):
    return [[(f["position"], f["burst_kind"], f["crc_ok"],
              [(b["channel"], b["crc_ok"], b["block"], b["bits"].tobytes()) for b in f["blocks"]]) for f in fr]
            for fr in frames]


def test_etsi_lower_mac_vote_batch_and_stream():
    """EtsiLowerMac(vote=True): with one cell per channel the frames of decode_batch and of decode_stream
    over three chunks are those of EtsiLowerMac(); cell_score > 0 where a cell was acquired, and
    reset_stream() clears it.  TetraDecoder(mode="etsi", vote=True) passes the keyword on."""
    from tetraear.core.etsi import EtsiLowerMac
    from tetraear.core import TetraDecoder
    b = R.viterbi_batch(300, 12, 2)
    plain, vote = EtsiLowerMac(), EtsiLowerMac(vote=True)
    assert vote.vote and vote.vote_cap == V.CAP and vote.cell_score is None and not plain.vote
    fp, fv = plain.decode_batch(b["soft"], b["hard"], b["nsym"]), vote.decode_batch(b["soft"], b["hard"], b["nsym"])
    assert _views(fp) == _views(fv) and sum(len(f) for f in fp) == 36
    assert np.array_equal(plain.cell_state, vote.cell_state) and np.array_equal(plain.acquired, vote.acquired)
    assert vote.cell_score.dtype == np.int32 and np.array_equal(vote.cell_score > 0, vote.acquired) and vote.acquired.any()
    vote.reset_stream()
    assert vote.cell_score is None
    plain, vote = EtsiLowerMac(), EtsiLowerMac(vote=True, vote_cap=5000)
    nd = int(b["nsym"].min()) - 1
    for a, e in ((0, 400), (400, 1000), (1000, nd)):
        ns = np.full(12, e - a + 1, np.int32)
        h, s = b["hard"][:, a:e], b["soft"][:, 2 * a:2 * e]
        assert _views(plain.decode_stream(s, h, ns)) == _views(vote.decode_stream(s, h, ns)), a
    assert np.array_equal(plain.cell_state, vote.cell_state) and vote.acquired.any()
    assert np.array_equal(vote.cell_score > 0, vote.acquired) and vote.cell_score.max() <= 5000
    with pytest.raises(ValueError):
        EtsiLowerMac(mcc=1, mnc=2, colour_code=3, vote=True)
    d = TetraDecoder(auto_decrypt=False, mode="etsi", vote=True)
    assert d._etsi_rx().vote and not TetraDecoder(auto_decrypt=False, mode="etsi")._etsi_rx().vote


NW = 3_300_000   # tests/test_gpu_wideband_acquire.py's capture: three timing chunks per carrier


@pytest.fixture(scope="module")
def capture3():
    from tetraear.signal.wideband import synth_wideband
    return synth_wideband(NW, seed=17, snr_db=25.0, cfo_max=300.0)


def _wb_views(frames, key="sample"):
    return [[(f[key], f["position"], f["burst_kind"], f["chunk"], f["crc_ok"],
              [(b["channel"], b["crc_ok"], b["block"], b["bits"].tobytes()) for b in f["blocks"]]) for f in fr]
            for fr in frames]


def test_wideband_decode_acquire_with_a_score(capture3):
    """decode_acquire(score=...): one cell per carrier, so the frames, the state and ngood are the
    non-voting call's; score is updated in place, > 0 exactly where a BSCH was heard."""
    from tetraear.signal.wideband import WidebandReceiver
    x, cells = capture3[0], capture3[1]
    rx = WidebandReceiver()
    unknown = np.full(len(cells), 3, np.uint32)
    want, state0, ngood0 = rx.decode_acquire(x, unknown)
    score = np.zeros(len(cells), np.int32)
    got, state, ngood = rx.decode_acquire(x, unknown, score=score)
    assert _wb_views(got) == _wb_views(want)
    assert np.array_equal(state, state0) and np.array_equal(ngood, ngood0) and (ngood > 0).any()
    assert np.array_equal(score > 0, ngood > 0) and score.max() <= V.CAP
    print("score where acquired: min %d median %d max %d" % (score[ngood > 0].min(), np.median(score[ngood > 0]), score.max()))
    with pytest.raises(ValueError):
        rx.decode_acquire(x, unknown, score=np.zeros(len(cells), np.int64))


def test_wideband_stream_vote(capture3):
    """WidebandStream(vote=True) over two pieces: the frames and cells of WidebandStream(), cell_scores > 0
    where acquired, carried from piece to piece and cleared by reset()."""
    from tetraear.signal import wideband as WB
    x = capture3[0]
    plain, vote = WB.WidebandStream(), WB.WidebandStream(vote=True)
    assert plain.cell_scores is None and vote.cell_scores.tolist() == [0] * vote.M
    prev = None
    for a, b in ((0, 1_700_001), (1_700_001, NW)):
        fp, fv = plain.decode(x[a:b]), vote.decode(x[a:b])
        assert _wb_views(fp, "stream_sample") == _wb_views(fv, "stream_sample"), a
        assert np.array_equal(plain.cell_state, vote.cell_state) and np.array_equal(plain.acquired, vote.acquired)
        sc = vote.cell_scores
        assert np.array_equal(sc > 0, vote.acquired)
        if prev is not None:
            assert np.all(sc >= prev) and np.any(sc > prev)   # one cell per carrier: the score only grows
        prev = sc
    assert vote.acquired.sum() > 0.8 * vote.M
    vote.reset()
    assert vote.cell_scores.tolist() == [0] * vote.M
    with pytest.raises(ValueError):
        WB.WidebandStream(cells=np.full(vote.M, 3, np.uint32), vote=True)
