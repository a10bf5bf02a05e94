"""CPU checks of the loss-of-lock monitor's rule and constants (tests/_etsi_lock_model.py, the numpy
restatement of tetra_etsi_lock and of EtsiStream(lock=True, redo=True) over oracle/etsi.py Stream): the
state machine on hand-made records, the three conditions the committed constants were chosen for
 on a reduced set, and the reason for the feature -- a 66-sample slip pins the carried
loop at its clamp for good, and one re-acquisition cures it.
"""
import os
import re

import numpy as np
import pytest

import _etsi_lock_model as M

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J, B, R, F, D, S = M.F_JUDGED, M.F_BAD, M.F_RAILED, M.F_FRESH, M.F_DROPPED, M.F_SEARCHING


def _state(**kw):
    st = np.zeros(1, M.LOCK_STATE)
    for k, v in kw.items():
        st[k] = v
    return st


def _judge(st, smin=90, smax=100, n=200, weak=0, delta=0.1, **kw):
    rec, clear = M.judge(smin, smax, n, weak, delta, st[0], **{**dict(num=1, den=2, nmin=64, patience=1), **kw})
    return int(rec[M.R_FLAGS]), clear


def _fields(st):
    return tuple(int(st[k][0]) for k in ("searching", "bad_run", "relocks", "chunks"))


def test_header_and_binding_carry_the_model_constants():
    txt = open(os.path.join(REPO, "include", "tetra_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define TETRA_ETSI_LOCK_(\w+)_DEFAULT (\d+)", txt)}
    assert got == dict(NUM=M.NUM, DEN=M.DEN, WEAK=M.WEAK, NMIN=M.NMIN, PATIENCE=M.PATIENCE)
    assert txt.count("a stated choice, backed by the table of §5.28") == 5
    from tetraear import _hip
    assert (_hip.ETSI_LOCK_NUM_DEFAULT, _hip.ETSI_LOCK_DEN_DEFAULT, _hip.ETSI_LOCK_WEAK_DEFAULT,
            _hip.ETSI_LOCK_NMIN_DEFAULT, _hip.ETSI_LOCK_PATIENCE_DEFAULT) == (M.NUM, M.DEN, M.WEAK, M.NMIN, M.PATIENCE)
    assert _hip.ETSI_LOCK_STATE == M.LOCK_STATE and _hip.ETSI_LOCK_STATE.itemsize == 32


def test_first_chunk_is_fresh_and_a_good_one_locks():
    st = _state()
    assert _judge(st) == (J | F, False) and _fields(st) == (0, 0, 0, 1)
    assert _judge(st) == (J, False) and _fields(st) == (0, 0, 0, 2)


@pytest.mark.parametrize("patience", [1, 2])
def test_good_then_bad(patience):
    st = _state(chunks=5)
    for k in range(1, patience):
        assert _judge(st, smin=40, patience=patience) == (J | B, False) and _fields(st) == (0, k, 0, 5 + k)
    assert _judge(st, smin=40, patience=patience) == (J | B | D | S, True)
    assert _fields(st) == (1, 0, 1, 5 + patience)
    # a good chunk in between clears the run
    st = _state(chunks=5, bad_run=patience - 1)
    assert _judge(st, patience=patience) == (J, False) and _fields(st) == (0, 0, 0, 6)


def test_bad_and_fresh_keeps_searching():
    st = _state()
    for k in range(3):
        assert _judge(st, smin=40, patience=2) == (J | B | F | S, True) and _fields(st) == (1, 0, 0, k + 1)
    assert _judge(st, patience=2) == (J | F, False) and _fields(st) == (0, 0, 0, 4)


def test_unjudged_changes_nothing():
    st = _state(chunks=3, bad_run=1, relocks=2)
    assert _judge(st, smin=0, smax=0, n=63, weak=63, delta=1.5, patience=2) == (R, False)
    assert _fields(st) == (0, 1, 2, 4)
    st = _state(searching=1, chunks=3)
    assert _judge(st, n=10) == (F | S, False) and _fields(st) == (1, 0, 0, 4)
    st = _state()   # the all-zero state reads as searching, and stays so until a judged chunk
    assert _judge(st, n=0) == (F | S, False) and _fields(st) == (1, 0, 0, 1)
    assert _judge(st) == (J | F, False) and _fields(st) == (0, 0, 0, 2)


def test_every_leg_alone_is_bad():
    for kw, extra in ((dict(delta=1.5), R), (dict(delta=-1.5), R), (dict(weak=101), 0), (dict(smin=0, smax=0), 0),
                      (dict(smin=49), 0)):
        st = _state(chunks=1)
        assert _judge(st, **kw) == (J | B | D | S | extra, True), kw
    for kw in (dict(delta=1.4999999), dict(weak=100), dict(smin=50), dict(delta=float("nan"))):
        st = _state(chunks=1)
        assert _judge(st, **kw) == (J, False), kw


def test_sums_read_the_dibits_and_nothing_else():
    row = np.full(40, 127, np.int8)
    row[:12] = [-128, 3, 5, -7, 0, 0, 7, -7, 8, 0, -127, 127]
    assert M.sums(row, 7, 8) == (3 + 0 + 127, 128 + 8 + 127, 6, 3)
    assert M.sums(row, 7, 0) == (3 + 5 + 0 + 7 + 0 + 127, 128 + 7 + 0 + 7 + 8 + 127, 6, 0)
    assert M.sums(row, 0, 8) == (0, 0, 0, 0) and M.sums(row, 30, 8, ostride=6)[2] == 6


# ------------------------------------------------------------------------------ the constants' three conditions

RATES = [(2.4e6, 131072), (2.0e6, 109226)]


def _chunks(x, chunk):
    return [x[i:i + chunk] for i in range(0, len(x) - chunk + 1, chunk)]


@pytest.mark.parametrize("fs,chunk", RATES)
def test_no_locked_chunk_at_10_db_or_better_is_bad(fs, chunk):
    rng = np.random.default_rng(501)
    for snr in (None, 15.0, 10.0):
        ls = M.LockedStream(fs, lock=True, redo=True)
        out = [ls.push(c) for c in _chunks(M.capture(rng, 20 * chunk, fs, snr, t0=0.37, cfo=210.0), chunk)]
        bal = [M.balance(o["soft"], M.WEAK) for o in out]
        print(fs, snr, "balance %.3f..%.3f" % (min(bal), max(bal)))
        assert len(out) == 20 and not any(o["rec"][M.R_FLAGS] & B for o in out), (fs, snr)
        assert not any(o["dropped"] for o in out) and [o["fresh"] for o in out] == [True] + [False] * 19


@pytest.mark.parametrize("fs,chunk", RATES)
def test_every_noise_chunk_after_signal_is_bad(fs, chunk):
    rng = np.random.default_rng(502)
    n = 0
    for sigma in (0.02, 0.2, 2.0):
        x = np.concatenate([M.capture(rng, 2 * chunk, fs, 15.0), M.noise(rng, 7 * chunk, sigma)])
        ls = M.LockedStream(fs, lock=True, consts=dict(patience=1 << 30))   # never re-acquired: carried throughout
        out = [ls.push(c) for c in _chunks(x, chunk)]
        assert all(o["rec"][M.R_FLAGS] & B for o in out[2:]), (fs, sigma)
        n += len(out) - 2
    assert n >= 20


def _slip_runs(seed, fs=2.4e6, chunk=131072, drop=66, **kw):
    rng = np.random.default_rng(seed)
    x = M.slipped(M.capture(rng, 8 * chunk + drop, fs, 12.0, t0=0.55, cfo=-130.0), 2 * chunk, drop)
    ls = M.LockedStream(fs, **kw)
    return [ls.push(c) for c in _chunks(x, chunk)]


def test_the_66_sample_slip_is_dropped_by_the_chunk_after_it():
    """66 samples are half a symbol at 2.4 MSps (0.495): the slip the loop cannot track out.  (At 2.0 MSps
    they are 0.594 of a symbol and the loop often settles on the neighbouring symbol instead: DESIGN.md
    §5.28 lists that rate's count.)"""
    n = 0
    for seed in (601, 602, 603):
        out = _slip_runs(seed, lock=True, redo=True)
        first = [k for k, o in enumerate(out) if o["dropped"]]
        assert first and first[0] in (2, 3), (seed, first)
        n += len(out)
    assert n >= 20


def test_a_slip_pins_the_carried_loop_and_one_reacquisition_cures_it():
    """The reason for the feature.  Locked range: the balances of the same kind of capture at 12 dB without a
    slip on the carried oracle, widened below by its own width.  With the monitor and redo every chunk after
    the chunk of the slip lies in it and |delta| stays under the clamp; on the carried stream delta is pinned at
    the clamp and the balance stays under the range -- this half must keep failing the range for as long as a
    carried loop cannot re-acquire."""
    rng = np.random.default_rng(77)
    ref = M.LockedStream(2.4e6, lock=False)
    locked = [M.balance(ref.push(c)["soft"], M.WEAK) for c in _chunks(M.capture(rng, 12 * 131072, 2.4e6, 12.0), 131072)]
    lo = min(locked) - (max(locked) - min(locked))
    on = _slip_runs(601, lock=True, redo=True)
    off = _slip_runs(601, lock=False)
    b_on = [M.balance(o["soft"], M.WEAK) for o in on]
    b_off = [M.balance(o["soft"], M.WEAK) for o in off]
    d_on = [abs(float(o["track"]["delta"][0])) for o in on]
    d_off = [abs(float(o["track"]["delta"][0])) for o in off]
    print("locked %.3f..%.3f bound %.3f" % (min(locked), max(locked), lo))
    print("monitor", np.round(b_on, 3), np.round(d_on, 3))
    print("carried", np.round(b_off, 3), np.round(d_off, 3))
    k = [i for i, o in enumerate(on) if o["dropped"]][0]
    assert k in (2, 3)
    assert all(b >= lo for b in b_on[k + 1:]) and all(d < 1.5 for d in d_on[k:])
    assert sum(o["dropped"] for o in on) == 1 and int(on[-1]["state"]["relocks"][0]) == 1
    assert all(d == 1.5 for d in d_off[4:]) and all(b < lo for b in b_off[3:])
