"""The cell-vote model (tests/_lmac_vote.py) on the CPU: what tests/test_gpu_lmac_vote.py holds
tetra_lmac_etsi_vote_groups / _stream_vote to means what is assumed there.  With a fresh score and one
cell heard it is tests/_lmac_groups.py oracle_groups; the ballot-order, weight and incumbency cases
have their answers computed by hand here.  Integer and bit-exact: no tolerance anywhere.
"""
import numpy as np
import pytest

import etsi as E
import _etsi_quality_model as Q
import _lmac_groups as GR
import _lmac_rows as R
import _lmac_vote as V

N, P, SB = R.NDB_N, R.NDB_P, R.SB


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        fx, fy = R.flatten(x), R.flatten(y)
        assert fx[:2] == fy[:2]
        assert all(np.array_equal(p, q) for p, q in zip(fx[2], fy[2]))


@pytest.mark.parametrize("case", ["sync_in_row", "broken_after_good", "zero_cell"])
def test_fresh_score_and_one_cell_is_the_last_good_rule(case):
    """score = 0 and one distinct cell among the ballots: rows, cell and ngood equal oracle_groups's."""
    rng = np.random.default_rng(5)
    rows, init, A = {"sync_in_row": lambda: GR.case_sync_in_row(rng, 1), "broken_after_good": lambda: GR.case_broken_after_good(rng),
                     "zero_cell": lambda: GR.case_zero_cell(rng)}[case]()
    hard, soft, nsym = GR.pack(rows)
    G = len(rows)
    want, after, ngood = GR.oracle_groups(hard, soft, nsym, G, init)
    got, cells, scores, good, agree, ballots = V.oracle_vote_groups(hard, soft, nsym, G, init, [0], V.CAP)
    _same(got, want)
    assert cells == after == [A] and good == ngood == agree and good[0] >= 1
    assert scores == [min(V.CAP, sum(w for _, w in ballots[0]))] and all(c == A for c, _ in ballots[0])
    assert all(w == V.FULL for _, w in ballots[0])   # +-127 rows: every ballot at full scale


def test_ballot_order():
    """+-127 soft bits, score 0, incoming cell unknown.  A then B: a tie, the later ballot wins (B, as
    last-wins).  A, A, B: A (last-wins gives B).  The normal bursts, scrambled with A, decode only
    under A."""
    rng = np.random.default_rng(6)
    rows, cells = V.case_ballots(rng, [0, 1])
    A, B = cells[0][0], cells[1][0]
    hard, soft, nsym = GR.pack(rows)
    _, c, s, good, agree, _ = V.oracle_vote_groups(hard, soft, nsym, 2, [3], [0], V.CAP)
    assert (c, s, good, agree) == ([B], [1], [2], [1])   # margin 0: score max(1, 0)
    assert GR.oracle_groups(hard, soft, nsym, 2, [3])[1] == [B]
    rows, cells = V.case_ballots(rng, [0, 0, 1])
    A, B = cells[0][0], cells[1][0]
    hard, soft, nsym = GR.pack(rows)
    got, c, s, good, agree, _ = V.oracle_vote_groups(hard, soft, nsym, 3, [3], [0], V.CAP)
    assert (c, s, good, agree) == ([A], [V.FULL], [3], [2])
    last, after, _ = GR.oracle_groups(hard, soft, nsym, 3, [3])
    assert after == [B]
    sch = lambda rows_: [ok for w in rows_ for _, _, dec in w for k, _, ok in dec if k != 2]
    assert all(sch(got)) and not any(sch(last))


def test_foreign_last_rows_plant_what_is_claimed():
    rng = np.random.default_rng(7)
    rows, A, B = V.case_foreign_last(rng)
    hard, soft, nsym = GR.pack(rows)
    got, c, s, good, agree, ballots = V.oracle_vote_groups(hard, soft, nsym, 4, [3], [0], V.CAP)
    assert ballots[0] == [(A, V.FULL)] * 3 + [(B, 120 * 42)]
    assert (c, s, good, agree) == ([A], [3 * V.FULL - 120 * 42], [4], [3])
    assert all(all(GR.crc_flags(w)) for w in got)
    assert GR.oracle_groups(hard, soft, nsym, 4, [3])[1] == [B]


@pytest.mark.parametrize("amp,e", [(127, 0), (64, 1), (127, 2), (20, 3), (1, 0), (1, 3)])
def test_weight_of_a_built_block(amp, e):
    """A BSCH at amplitude a with e planted sign flips 48 type-5 positions apart reads w = 120 a - 2 e a;
    at +-1 it still votes (w >= 1)."""
    rng = np.random.default_rng(100 * amp + e)
    A = R.cell_fields(rng)
    bits, soft = V.row(rng, [(4, N, A[0], None), V.sync_item(rng, A, gap=3)], 2, amps=[None, amp])
    s = 4 + 510 + 3
    pos = s + 94 + int(rng.integers(0, 120 - Q.FLIP_STEP * max(e - 1, 0))) + Q.FLIP_STEP * np.arange(e)
    soft[pos] = -soft[pos]
    hard, sf, nsym = GR.pack([(bits, soft)])
    _, c, sc, good, agree, ballots = V.oracle_vote_groups(hard, sf, nsym, 1, [3], [0], V.CAP)
    assert ballots == [[(A[0], 120 * amp - 2 * e * amp)]] and ballots[0][0][1] >= 1
    assert (c, sc, good, agree) == ([A[0]], [120 * amp - 2 * e * amp], [1], [1])


def test_weight_floor():
    """max(1, ...): soft bytes that disagree with the codeword as much as they agree still weigh 1."""
    t = np.zeros(60, np.uint8)
    c5 = Q.type5(t, 2, 3)
    s = np.where(c5 == 0, 10, -10).astype(np.int8)
    assert V.weight(s, t) == 1200
    s[:60] = -s[:60]
    assert V.weight(s, t) == 1
    s[60:] = 0
    assert V.weight(s, t) == 1


def test_incumbency_by_hand():
    A, B, C, D = 7, 11, 15, 19
    # score saturates at cap
    assert V.vote(A, 0, [(A, 60)], 100) == (A, 60, 1)
    assert V.vote(A, 60, [(A, 60)], 100) == (A, 100, 1)
    assert V.vote(A, 100, [(A, 60), (A, 60)], 100) == (A, 100, 2)
    # a challenger of 30 per call against an incumbent at 100: 70, 40, 10, then 10 < 30 and B takes over
    state = (A, 100)
    seen = []
    for _ in range(5):
        state = V.vote(state[0], state[1], [(B, 30)], 100)[:2]
        seen.append(state)
    assert seen == [(A, 70), (A, 40), (A, 10), (B, 20), (B, 50)]
    # a tie keeps the incumbent, at the floor
    assert V.vote(A, 30, [(B, 30)], 100) == (A, 1, 0)
    assert V.vote(A, 30, [(B, 31)], 100) == (B, 1, 1)
    # three cells split a call: the incumbent among the tied stays; else the latest last ballot wins
    assert V.vote(A, 0, [(A, 10), (B, 10), (C, 10)], 100) == (A, 1, 1)
    assert V.vote(D, 0, [(A, 10), (B, 10), (C, 10)], 100) == (C, 1, 1)
    assert V.vote(D, 0, [(C, 10), (B, 10), (A, 5), (C, 5), (B, 5)], 100) == (B, 1, 2)
    assert V.vote(D, 0, [(C, 10), (B, 10), (A, 5), (B, 5), (C, 5)], 100) == (C, 1, 2)
    # no ballot: nothing moves (a negative score stays as it is; with a ballot it reads as 0)
    assert V.vote(A, -5, [], 100) == (A, -5, 0)
    assert V.vote(A, -5, [(B, 3)], 100) == (B, 3, 1)
    assert V.vote(A, -5, [(A, 3)], 100) == (A, 3, 1)


def test_stream_model_carries_the_score():
    """VoteStream over a stream cut inside a synchronisation burst's BSCH: the ballot is cast in the
    chunk that decodes the burst, and the score it leaves defends the cell in the next chunks."""
    rng = np.random.default_rng(9)
    A, B = R.cell_fields(rng), R.cell_fields(rng)
    bits, planted, _ = R.place_bursts(rng, [(3, N, A[0], None), V.sync_item(rng, A), (1, P, A[0], None),
                                            V.sync_item(rng, B, A[0]), (0, N, A[0], None)])
    soft = R.soft_of(bits)
    V.scale_burst(soft, planted[3][0], 50)
    hard = R.hard_of(bits)
    cuts = R.cuts_at(len(hard), [(planted[1][0] + 150) // 2, (planted[3][0] - 40) // 2])
    m = V.VoteStream(E.Receiver())
    seen = []
    for at, n in cuts + [(len(hard), 0)]:
        r = m.push(hard[at:at + n], soft[2 * at:2 * (at + n)])
        seen.append((m.cell, m.score, m.ngood, m.agree, [ok for _, _, dec in r["bursts"] for _, _, ok in dec]))
    assert [s[:4] for s in seen] == [(3, 0, 0, 0), (A[0], V.FULL, 1, 1), (A[0], V.FULL - 6000, 1, 0),
                                     (A[0], V.FULL - 6000, 0, 0)]
    assert all(all(s[4]) for s in seen[1:]) and sum(len(s[4]) for s in seen) == 8
