"""The rows tests/_lmac_rows.py builds, on the CPU oracle: they mean what tests/test_gpu_lmac_rows.py
assumes, so a GPU mismatch there is a finding about the kernel and not about the fixture.

  * a burst with TOTAL - THRESH scored bits flipped is found (alone), with one more it is not;
  * the chunked scan (LmacStreamModel) equals the whole-stream scan and the planted list;
  * the soft-bit classes decode as their names say;
  * the Gaussian class is neither all CRC-good nor all CRC-bad (the GPU test's maximum-likelihood
    check rests on its CRC-good blocks), and the oracle's decode of it is at least as likely as the
    transmitted codeword by the independent restatement oracle/etsi_spec.py.
Everything is integer and bit-exact: no tolerance anywhere.
"""
import numpy as np
import pytest

import etsi as E
import etsi_spec as S
import _lmac_rows as R

VITERBI_SEEDS = (100, 101, 102, 103)   # tests/test_gpu_lmac_rows.py: row width mod 4 = seed - 100


def test_threshold_known_answers():
    """NDB: 40 of 44, SB: 54 of 60 -- found exactly at the threshold, alone; nothing one past it.
    (n and p differ in 10 of their 22 bits, so no input scores >= 40 on both: the n / p choice at the
    threshold cannot tie, and no case is built for it.)"""
    rx = E.Receiver()
    rows = R.threshold_rows(1, 200)
    count = {}
    for bits, off, kind, found in rows:
        got = rx.sync(R.hard_of(bits))
        want = [(off, kind)] if found else []
        key = (kind, found)
        n, ok = count.get(key, (0, 0))
        count[key] = (n + 1, ok + (got == want))
    print("threshold cases (kind, at threshold) -> (cases, as expected):", count)
    assert all(n == ok for n, ok in count.values()), count
    assert all(n >= 200 for n, _ in count.values())


@pytest.mark.parametrize("kind,where", R.FIXED_THRESHOLD_CASES)
def test_threshold_fixed_fields(kind, where):
    """All the flips in one field: the head, the tail (bit 509 among them), the sync sequence's
    last six bits, positions where n and p differ."""
    rx = E.Receiver()
    rng = np.random.default_rng(7)
    for _ in range(20):
        bits, off, k, _ = R.threshold_case(rng, kind, 0, where)
        assert rx.sync(R.hard_of(bits)) == [(off, kind)]
        bits, off, k, _ = R.threshold_case(rng, kind, 1, where)
        assert rx.sync(R.hard_of(bits)) == []


def test_np_sequences_differ_in_ten():
    assert len(R.NP_DIFFER) == 10 and R.TOTAL[R.NDB_N] - 10 < R.THRESH[R.NDB_N]


def test_random_rows_hold_no_burst():
    rx = E.Receiver()
    rng = np.random.default_rng(2)
    hits = sum(len(rx.sync(R.hard_of(rng.integers(0, 2, 4096).astype(np.uint8)))) for _ in range(200))
    assert hits == 0, hits


def test_builders_invert_the_oracle_views():
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, 1000).astype(np.uint8)
    assert np.array_equal(E.Receiver.hard_bits(R.hard_of(bits)), bits)
    assert np.array_equal(R.soft_of(bits, 5), np.where(bits == 0, 5, -5))
    for kind in (R.NDB_N, R.NDB_P, R.SB):
        pos = R.scored_positions(kind)
        assert len(pos) == R.TOTAL[kind] == len(set(pos.tolist()))
        burst, _ = E.make_burst(kind, rng, E.scramble_seq(R.random_cell(rng), 432))
        train = {R.NDB_N: (244, E.N_BITS), R.NDB_P: (244, E.P_BITS), R.SB: (214, E.Y_BITS)}[kind]
        want = np.concatenate([E.Q_BITS[10:22], train[1], E.Q_BITS[0:10]])
        assert np.array_equal(burst[pos], want)
        for off in (0, 1, 77):
            row = np.zeros(700, np.uint8)
            R.plant(row, off, burst)
            assert np.array_equal(row[off:off + 510], burst) and not row[:off].any() and not row[off + 510:].any()


def test_chunked_scan_equals_whole_scan():
    """300 streams cut into chunks of CHUNKS dibits: the bursts the chunked scan finds, each once,
    are the whole-stream scan's and the planted ones; every block decodes to its payload; the carried
    tail stays within RESERVE and a row within the kernel's 2048 dibits."""
    rx = E.Receiver()
    nburst = max_tail = max_row = 0
    for seed in range(300):
        bits, planted, jobs, cell = R.burst_stream(seed)
        hard, soft = R.hard_of(bits), R.soft_of(bits)
        whole, _ = rx.sync_from(hard, 0, maxb=64)
        assert whole == planted, seed
        m = R.LmacStreamModel(rx, cell)
        got = []
        for at, n in R.chunk_cuts(seed, len(hard)):
            r = m.push(hard[at:at + n], soft[2 * at:2 * (at + n)])
            max_row = max(max_row, r["tail"] + n)
            max_tail = max(max_tail, len(m.tail_hard))
            for pos, kind, dec in r["bursts"]:
                got.append((2 * at + pos, kind))
                want = jobs[len(got) - 1]
                assert [(k, ok) for k, _, ok in dec] == [(k, True) for k, _ in want], (seed, at)
                assert all(np.array_equal(t, w) for (_, t, _), (_, w) in zip(dec, want)), (seed, at)
        assert got == planted, (seed, got, planted)
        nburst += len(got)
    print("chunked scan:", nburst, "bursts; longest carried tail", max_tail, "dibits; longest row", max_row)
    assert max_tail <= E.RESERVE and max_row <= 2048 and nburst > 2000


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_soft_classes_on_the_oracle(kind):
    rng = np.random.default_rng(10 + kind)
    K, a, n2, n1 = E.KIND_PARAMS[kind]
    for _ in range(20):
        init = R.random_cell(rng)
        scr = E.scramble_seq(init, K)
        t1 = rng.integers(0, 2, n1).astype(np.uint8)
        tx = E.encode_block(t1, kind, scr)
        assert np.array_equal(tx, S.encode(t1, kind, init))
        bits, ok = E.Receiver.decode_block(R.soft_class("clean", tx, rng, kind), kind, scr)
        assert ok and np.array_equal(bits, t1)
        bits, ok = E.Receiver.decode_block(R.soft_class("zero", tx, rng, kind), kind, scr)
        assert not ok and not bits.any()   # every ACS a tie: the d3 = 0 predecessor, the all-zero path
        # -128 is its own negative in int8: on a scrambled position it stays negative where -127
        # would turn positive.  With -128 on every scrambled position the block is the type-4 block
        # that holds -128 there, and no longer the codeword
        soft = R.soft_class("clean", tx, rng, kind)
        soft[scr == 1] = -128
        soft4 = np.where(scr == 1, -128, soft).astype(np.int8)
        got = E.Receiver.decode_block(soft, kind, scr)
        want = E.Receiver.decode_block(soft4, kind, np.zeros(K, np.uint8))
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and not got[1]
        bits, ok = E.Receiver.decode_block(R.soft_class("inverted", tx, rng, kind), kind, scr)
        assert not ok


def _gauss_blocks():
    """(block kind, soft block, cell or BSCH init, type-1) of every Gaussian-class block of the
    GPU test's Viterbi batches."""
    out = []
    for seed in VITERBI_SEEDS:
        b = R.viterbi_batch(seed, 64, seed - VITERBI_SEEDS[0])
        for ch, blocks in enumerate(b["blocks"]):
            for start, bk, kind, fields, cls, t1, tx in blocks:
                if cls == "gauss":
                    out.append((seed, kind, R.block_soft(b["soft"][ch], start, fields),
                                3 if kind == 2 else int(b["cells"][ch]), t1))
    return out


def test_viterbi_batch_covers_classes_and_alignments():
    seen, align = set(), set()
    for seed in VITERBI_SEEDS:
        b = R.viterbi_batch(seed, 64, seed - VITERBI_SEEDS[0])
        smax = b["hard"].shape[1]
        assert b["soft"].shape[1] == 2 * smax and smax <= 2050 and smax % 4 == seed - VITERBI_SEEDS[0]
        for ch, blocks in enumerate(b["blocks"]):
            for start, bk, kind, fields, cls, t1, tx in blocks:
                seen.add((kind, cls))
                for o, n in fields:   # the segment's byte alignment in the soft-bit buffer
                    align.add((kind, o, (ch * 2 * smax + start + o) % 4))
        last = b["blocks"][-1][-1][0]
        assert last + 510 == 2 * (int(b["nsym"][-1]) - 1)   # the last burst ends the last row
    assert seen == {(k, c) for k in (0, 1, 2) for c in R.SOFT_CLASSES}
    assert align == {(k, o, a) for k, o in ((0, 14), (0, 282), (1, 14), (1, 282), (2, 94)) for a in range(4)}


def test_gauss_class_share_and_likelihood():
    """Per block kind the oracle's CRC-good share of the Gaussian class lies in [0.25, 0.75] on the
    GPU test's seeds, and every CRC-good decode is at least as likely as what was transmitted."""
    blocks = _gauss_blocks()
    for seed in VITERBI_SEEDS:
        for kind in (0, 1, 2):
            sel = [b for b in blocks if b[0] == seed and b[1] == kind]
            good = 0
            for _, _, soft, init, t1 in sel:
                bits, ok = E.Receiver.decode_block(soft, kind, E.scramble_seq(init, E.KIND_PARAMS[kind][0]))
                good += ok
                if ok:
                    got = S.codeword_metric(soft, S.type2(bits), kind, init)
                    sent = S.codeword_metric(soft, S.type2(t1), kind, init)
                    assert got >= sent, (seed, kind, got, sent)
            print("seed", seed, "kind", kind, "CRC-good", good, "of", len(sel))
            assert len(sel) >= 8 and 0.25 <= good / len(sel) <= 0.75, (seed, kind, good, len(sel))
