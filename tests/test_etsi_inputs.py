"""The rows of tests/_etsi_inputs.py on the CPU oracle alone: they mean what
tests/test_gpu_etsi_inputs.py assumes, and the receiver is scale-exact over the window it documents.

Scale-exact: the input times 2^k gives the same dibits, soft bits, symbol count and diagnostics, and
the symbols times 2^k, bit for bit.  Before the CFO norm was taken on a power-of-two-normalised Z the
oracle held that only for k in [-11, +4]: at k = +5 (floats left in int16 units are far above that)
Zr^2 + Zi^2 overflowed, the rotation became (0, -0) and every dibit and soft bit read 0.
"""
import numpy as np
import pytest

import etsi as E
import _etsi_inputs as I


@pytest.fixture(scope="module")
def rx():
    return E.Receiver()


def _demod(rx, x):
    with np.errstate(all="ignore"):   # the top rungs overflow on purpose
        y = rx.chanfilt(x)
        return (y,) + rx.timing(y)


@pytest.fixture(scope="module")
def ladder(rx):
    """{k: (y, sym, soft, hard, diag)} of the ladder rows."""
    return {k: _demod(rx, r) for k, r in zip(I.LADDER, I.ladder_rows())}


def _scale_exact(ref, got, k):
    return (len(got[1]) == len(ref[1]) and np.array_equal(got[3], ref[3]) and np.array_equal(got[2], ref[2])
            and np.array_equal(got[4], ref[4]) and np.array_equal(got[1], I.scale(ref[1], k)))


def test_scale_exact_window(rx, ladder):
    """Every integer k of WINDOW = [-16, +10] (the ladder's rungs inside it included) is scale-exact."""
    ref = ladder[0]
    assert len(ref[1]) == 141
    exact = {k: _scale_exact(ref, _demod(rx, I.scale(I.base(), k)), k) for k in range(-24, 17)}
    lo = min(k for k in exact if all(exact[j] for j in range(k, 1)))
    hi = max(k for k in exact if all(exact[j] for j in range(0, k + 1)))
    print("scale-exact window measured: [%d, %d]" % (lo, hi))
    bad = [k for k in range(I.WINDOW[0], I.WINDOW[1] + 1) if not exact[k]]
    assert not bad, bad
    for k in I.LADDER:
        if I.WINDOW[0] <= k <= I.WINDOW[1]:
            assert _scale_exact(ref, ladder[k], k), k


def test_ladder_outside_the_window(ladder):
    """What is lost outside the window, rung by rung: never a wrong dibit while any signal is left,
    never a rotation of (0, -0) or NaN."""
    ref = ladder[0]
    for k, (y, sym, soft, hard, diag) in ladder.items():
        rot = diag[2:4]
        assert np.all(np.isfinite(rot)) and abs(np.hypot(*rot.astype(np.float64)) - 1) < 1e-6, (k, rot)
        if k >= 58:   # |y|^2 overflows: inf - inf in the Oerder-Meyr sums, no timing phase, no symbols
            assert len(sym) == 0 and np.isnan(diag[0]), k
            continue
        assert len(sym) == len(ref[1]), k
        if k <= -100:   # |y|^2 and d underflow to 0: the output of a silent channel
            assert not hard.any() and not soft.any() and tuple(rot) == (1.0, 0.0), k
            continue
        assert np.array_equal(hard, ref[3]), k          # the k = 0 dibits
        if k >= 13 or k <= -40:   # the d^4 sums overflow / underflow: no CFO estimate, identity rotation
            assert tuple(rot) == (1.0, 0.0), k
        else:
            assert np.allclose(rot, ref[4][2:4], rtol=0, atol=1e-6), (k, rot)
        if k >= 29 or k <= -41:   # |d|^2 overflows / underflows: no soft scale
            assert not soft.any(), k
        else:
            assert np.array_equal(soft, ref[2]) if -18 <= k <= 12 else soft.any(), k   # the rotation's bits
    assert np.all(np.isfinite(ladder[57][1].view(np.float32)))   # +57: symbols finite, +58: |y|^2 is not


def _subnormal(v):
    v = np.abs(np.asarray(v, np.float32))
    return int(np.count_nonzero((v > 0) & (v < np.float32(2.0 ** -126))))


def test_subnormals_are_present_where_claimed(ladder):
    """The rungs that claim subnormal arithmetic have subnormal, nonzero values in it (and the ones
    that claim a flush have zeros): y at -130, |y|^2 and d_j at -70, the d^4 terms at -19 / -18."""
    with np.errstate(all="ignore"):
        def parts(k):
            y, sym = ladder[k][0], ladder[k][1]
            yf = y.view(np.float32).reshape(-1, 2)
            p = yf[:, 0] * yf[:, 0] + yf[:, 1] * yf[:, 1]
            d = (sym[1:] * np.conj(sym[:-1])).astype(np.complex64)
            d2 = (d * d).astype(np.complex64)
            return yf, p, d.view(np.float32), (d2 * d2).astype(np.complex64).view(np.float32)
        yf, p, d, d4 = parts(-130)
        assert _subnormal(yf) > len(yf) and _subnormal(I.ladder_rows()[I.LADDER.index(-130)].view(np.float32)) > 0
        yf, p, d, d4 = parts(-120)   # y normal, the products of small taps and samples underflow
        assert _subnormal(yf) < 0.02 * yf.size and np.count_nonzero(yf) > 0.99 * yf.size
        h = np.abs(E.design()["hp"])
        assert np.count_nonzero(h * np.float32(2.0 ** -121) < np.float32(2.0 ** -126)) > 50
        yf, p, d, d4 = parts(-100)
        assert _subnormal(yf) == 0 and not p.any()
        yf, p, d, d4 = parts(-70)
        assert _subnormal(p) > 0.9 * len(p)
        assert _subnormal(d) > 0.5 * d.size and np.count_nonzero(d) > 0.9 * d.size
        yf, p, d, d4 = parts(-64)   # d_j normal again, |d_j|^2 flushed: no soft scale
        assert _subnormal(d) < 0.05 * d.size and np.count_nonzero(d) > 0.9 * d.size and not (d * d).any()
        yf, p, d, d4 = parts(-19)
        assert _subnormal(d4) > 0.5 * d4.size and np.count_nonzero(d4) > 0.9 * d4.size
        yf, p, d, d4 = parts(-18)   # the first subnormal terms: too few to move the rotation
        assert 0 < _subnormal(d4) < 0.2 * d4.size
        yf, p, d, d4 = parts(-12)
        assert _subnormal(d4) == 0


def test_class_known_answers(rx):
    out = {n: _demod(rx, r) for n, r in zip(I.CLASSES, I.class_rows())}
    for n in ("zeros", "neg_zeros"):
        y, sym, soft, hard, diag = out[n]
        assert len(sym) == 141 and not hard.any() and not soft.any() and tuple(diag[2:4]) == (1.0, 0.0), n
        assert not y.view(np.float32).any()
    assert np.all(np.signbit(I.class_rows()[I.CLASSES.index("neg_zeros")].view(np.float32)))
    soft = out["impulse"][2]
    assert soft.max() == 127 and soft.min() == -127
    y, sym, soft, hard, diag = out["lsb_noise"]
    assert np.count_nonzero(soft) > len(soft) // 2 and set(hard.tolist()) == {0, 1, 2, 3}
    y, sym, soft, hard, diag = out["square"]
    assert set(hard.tolist()) == {0, 1, 2, 3}
    # tones: one dibit value throughout (a constant phase step); the stopband tone leaves about 3e-6
    for n in ("dc", "sc16_min", "tone_0", "tone_3k", "tone_4k5", "tone_200k"):
        assert len(set(out[n][3].tolist())) == 1, n
    a = np.abs(out["tone_200k"][0][100:-100])
    assert 1e-7 < a.max() < 1e-5, a.max()
    # half a row of signal: its dibits are the base row's there, silence decides 0
    ref = _demod(rx, I.base())
    assert np.array_equal(out["base_silence"][3][5:60], ref[3][5:60]) and not out["base_silence"][3][80:].any()
    assert np.array_equal(out["silence_base"][3][85:135], ref[3][85:135]) and not out["silence_base"][3][:60].any()


def test_sc16_rows_are_exact_and_what_they_say():
    q = I.sc16_rows()
    x = I.sc16_to_cf32(q)
    assert q.dtype == np.int16 and x.dtype == np.complex64
    cls = dict(zip(I.CLASSES, I.class_rows()))
    for n in ("zeros", "dc", "sc16_min", "lsb_noise", "square"):   # held exactly
        assert np.array_equal(x[I.SC16_CLASSES.index(n)], cls[n]), n
    assert (q[I.SC16_CLASSES.index("sc16_min")] == -32768).all()
    imp = q[I.SC16_CLASSES.index("impulse")]
    assert np.count_nonzero(imp) == 1 and imp.max() == 32767   # 1.0 clips to full scale
    sq = q[I.SC16_CLASSES.index("square")]
    assert set(np.unique(sq).tolist()) == {-32768, 32767}
    assert set(np.unique(q[I.SC16_CLASSES.index("lsb_noise")]).tolist()) == {-1, 0, 1}
    weak = q[I.SC16_CLASSES.index("base_2^-11")]
    assert np.median(np.abs(weak)) <= 16 and np.count_nonzero(weak) > weak.size // 2   # a few LSB
    # the weak row still demodulates to mostly the base dibits
    rx = E.Receiver()
    h0 = rx.demod(I.base())[2]
    h = rx.demod(x[I.SC16_CLASSES.index("base_2^-6")])[2]
    assert np.mean(h == h0) > 0.95


def test_built72_rows(rx):
    rows = dict(zip(I.BUILT72, I.built72_rows()))
    A = E.Receiver.om_quarters(rows["const"])
    assert A[0] == A[2] and A[1] == A[3] and A[0] > 0          # X exactly 0: pat2(0, 0)
    sym, soft, hard, diag = rx.timing(rows["const"])
    assert len(sym) == 161 and diag[0] == 0 and not hard.any()
    A = E.Receiver.om_quarters(rows["class1"])
    assert A[1] > 0 and A[0] == 0 and A[2] == 0 and A[3] == 0
    assert len(rx.timing(rows["class1"])[0]) == 161
    # on-sample rows: the symbols are the samples placed
    for n in ("axis_ties", "half_even"):
        sym, soft, hard, diag = rx.timing(rows[n])
        assert len(sym) == 161 and np.array_equal(sym, rows[n][4::4]), n
        assert diag[0] == 0 and np.signbit(diag[0]) and diag[1] == 0 and tuple(diag[2:4]) == (1.0, 0.0), n
    sym, soft, hard, diag = rx.timing(rows["axis_ties"])
    d = (sym[1:] * np.conj(sym[:-1])).astype(np.complex64).view(np.float32).reshape(-1, 2)
    s = sym.view(np.float32).reshape(-1, 2)
    dr = s[1:, 0] * s[:-1, 0] + s[1:, 1] * s[:-1, 1]           # exact: small integers, signed zeros as fmaf gives
    di = s[1:, 1] * s[:-1, 0] + -(s[1:, 0] * s[:-1, 1])
    ties = (dr == 0) | (di == 0)
    assert ties.sum() >= 50 and np.all((dr != 0) | (di != 0))
    zeros = np.where(dr == 0, dr, di)[ties]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()   # +0 and -0 ties
    assert np.array_equal(np.abs(d[:, 0]), np.abs(dr))
    assert not soft[0::2][di == 0].any() and not soft[1::2][dr == 0].any()
    assert not (hard[di == 0] & 2).any() and not (hard[dr == 0] & 1).any()   # a zero of either sign decides 0
    sym, soft, hard, diag = rx.timing(rows["half_even"])
    a = np.abs(soft.astype(np.int32))
    assert set(a.tolist()) == set(I.HALF_EVEN_SOFT)    # 61.5 -> 62, 22.5 -> 22 (half-away: 23), 82, 12
    assert np.count_nonzero(a == 22) >= 30 and np.count_nonzero(a == 62) >= 30
    # signal in the middle block only: symbols of exact zeros before and after it
    sym, soft, hard, diag = rx.timing(rows["w_zero_blocks"])
    assert len(sym) == 161 and not sym[:64].any() and sym[70:130].all() and not sym[140:].any()


def test_stream_chunks(rx):
    """E.Stream over the chunk sequence: the windows' filter outputs are the whole capture's (what the
    oracle's own tests promise of a Stream), the first chunk is the chunk on its own, and the loop
    state stays finite through the silent, weak, two-sample, loud and noise-only chunks."""
    for chunks, conv in ((I.stream_chunks(), lambda c: c), (I.stream_chunks_sc16(), I.sc16_to_cf32)):
        xs = [conv(c) for c in chunks]
        yfull = rx.chanfilt(np.concatenate(xs))
        st = E.Stream(2.4e6, cell_init=I.CELL)
        done = 0
        for i, x in enumerate(xs):
            r = st.push(x)
            y0 = 3 * r["window"][0] // 100
            assert np.array_equal(r["y"], yfull[y0:y0 + len(r["y"])]), i
            if i == 0:
                so, sbo, ho, _ = rx.demod(x)
                assert np.array_equal(r["symbols"], so) and np.array_equal(r["soft"], sbo)
                assert np.array_equal(r["hard"], ho)
            else:
                assert y0 + r["yoff"] == done, i
            done = y0 + len(r["y"])
            t = r["track"][0]
            assert t["acquired"] == 1 and np.isfinite([t["base"], t["delta"], t["pr"], t["pi"]]).all(), i
            assert len(r["symbols"]) == (0 if len(x) == 2 else len(r["hard"]) + 1), i   # 2 samples: no output
        assert done == len(yfull)
        assert np.count_nonzero(r["soft"]) > len(r["soft"]) * 0.9   # the last chunk is signal again
