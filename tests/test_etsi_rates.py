"""The ETSI receiver over the whole plan space, on the CPU: the plans of the rate table
(tests/_etsi_rates.py), the oracle's channel filter against a float64 restatement that shares no code
with it, and the history a streaming window re-reads at every integer-kHz rate that has a plan.

tests/test_gpu_etsi_rates.py holds the kernels to the oracle at the same rates.
"""
import numpy as np
import pytest

import etsi as E

import _etsi_rates as R


def test_rate_table_plans():
    """Each table rate gets the plan the table states, from the product's designer and the oracle's.
    A designer change that moves a rate to another plan shows here as lost coverage."""
    from tetraear.signal.etsi import rate_design
    for fs, (q1, L1, up, down, Lp, win) in R.RATES.items():
        assert rate_design(fs) == (q1, L1, up, down, Lp), fs
        d = E.design(fs)
        assert (d["q1"], d["L1"], d["up"], d["down"], d["Lp"]) == (q1, L1, up, down, Lp), fs
        assert len(d["h1"]) == L1 and len(d["hp"]) == Lp and (Lp - 1) // up + 2 == win, fs


def test_rate_table_spans_the_plan_space():
    plans = list(R.RATES.values())
    assert {p[0] for p in plans} == set(range(1, 14))                      # every q1
    assert any(p[2] == p[3] == 1 for p in plans)                           # no resampling
    assert max(p[1] for p in plans) > 52 and max(p[4] for p in plans) > 4000
    assert max(p[5] for p in plans) == 252                                 # the widest window the designer makes
    assert any((p[0] * p[3]) % 2 for p in plans)                           # an odd window period
    # the GPU test's input lengths give the stage-1 counts they are chosen for, at most 20 000 samples
    for fs, (q1, L1, up, down, Lp, win) in R.RATES.items():
        S1 = R.RT1 - win
        want = R.chanfilt_m1(win)
        assert want[:5] == [S1, S1 + 1, 512, 2 * S1, 2 * S1 + 1] and want[5] > 2 * S1 and want[5] % S1, fs
        for n, m in zip(R.chanfilt_lengths(q1, L1, win), want):
            m1, m2 = R.plan_lengths(q1, L1, up, down, Lp, n)
            assert n % 2 == 0 and n <= 20000 and m2 > 0, (fs, n)
            assert m1 == m or (q1 == 1 and m % 2 and m1 == m + 1), (fs, n, m1, m)   # q1 = 1: M1 = N is even


@pytest.mark.parametrize("fs", list(R.RATES))
def test_oracle_chanfilt_vs_float64_restatement(fs):
    """eo_chanfilt on 4 ms of modulated signal against upfirdn in float64: the same length
    (tetra_etsi_lengths' formula) and both components within the a-priori rounding bound of the
    float32 fmaf chains.  An index convention off by one (n = Lp - 1 + down m, kmin, kmax, the stage-1
    alignment) misses the bound by orders of magnitude."""
    rx = E.Receiver(fs)
    d = rx.d
    n = 2 * int(round(0.004 * fs / 2))
    x = R.signal(E, fs, n, seed=fs // 1000)
    worst = R.check_against_f64(rx.chanfilt(x), x, d["h1"], d["hp"], d["q1"], d["up"], d["down"], fs)
    print(f"{fs}: worst error {worst:.3f} of the bound")


def test_float64_restatement_catches_a_misplaced_index():
    """The bound is tight enough to mean something: the oracle's outputs shifted by one 72 kHz sample,
    or computed from the input shifted by one sample, are far outside it."""
    fs = 1_000_000
    rx = E.Receiver(fs)
    d = rx.d
    x = R.signal(E, fs, 4000, seed=5)
    y = rx.chanfilt(x)
    for bad in (np.concatenate([y[1:], y[-1:]]), rx.chanfilt(np.concatenate([x[1:], x[:1]]))):
        with pytest.raises(AssertionError):
            R.check_against_f64(bad, x, d["h1"], d["hp"], d["q1"], d["up"], d["down"], fs)


def _plannable():
    from tetraear.signal.etsi import rate_design
    out = []
    for khz in range(72, 5001):
        try:
            rate_design(1000 * khz)
        except ValueError:
            continue
        out.append(1000 * khz)
    return out


def test_stream_history_covers_every_plannable_rate():
    """tetra_etsi_stream_window (host code, no GPU) over every integer-kHz rate from 72 kHz to 5 MSps
    that has a plan and three chunk patterns: the window never starts further before the chunk than
    EtsiStream keeps for that plan (stream_history).  With a constant 4096 samples kept, 68 of the
    1331 rates needed more (2.75 MSps: 4286, 4.953 MSps: 6004 on these patterns) and EtsiStream.demod
    raised on them."""
    from tetraear.signal.etsi import stream_history
    rates = _plannable()
    assert len(rates) == 1331
    patterns = R.chunk_patterns()
    short, over4096, worst = [], [], (0, 0)
    for fs in rates:
        plan = R.bare_plan(fs)
        need = R.history_needed(plan, patterns)
        keep = stream_history(plan)
        if need > keep:
            short.append((fs, need, keep))
        if need > 4096:
            over4096.append((fs, need))
        worst = max(worst, (need, fs))
        assert keep <= need + 2 * plan.q1 * plan.down, (fs, need, keep)   # a bound, not a guess: within a period
    print("rates needing more than 4096 samples:", over4096)
    assert not short, short
    assert worst[1] == 4_953_000 and len(over4096) == 68, (worst, len(over4096))


def test_stream_history_is_what_the_stream_keeps():
    from tetraear.signal.etsi import EtsiStream, stream_history, etsi_plan
    for fs in (2.4e6, 2.75e6, 4.953e6):
        assert EtsiStream(fs, 1).hist_len == stream_history(etsi_plan(fs))
    assert stream_history(etsi_plan(2.4e6)) == 1447 and stream_history(etsi_plan(4.953e6)) == 6046
