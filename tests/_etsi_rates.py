"""Rates that span the ETSI receiver's plan space, an fp64 restatement of its channel filter, and the
streaming-history sweep (helpers of tests/test_etsi_rates.py and tests/test_gpu_etsi_rates.py).

The GPU suite's other ETSI tests run the generic channel filter (k_chanfilt_g) at the reference GUI's
slider rates only (1.8-2.4 MSps: q1 in {7, 10, 11}, a stage-2 window of at most 104 taps).  RATES holds
one rate per region of the plan space the designer reaches: every q1 in 1..13, stage 1 absent (q1 = 1),
no resampling at all (1/1), the largest prototype and `up`, the widest stage-2 window, an odd window
period, and the rates whose streaming windows re-read the most input.
"""
import ctypes

import numpy as np
from scipy.signal import upfirdn

# fs (Hz): (q1, L1, up, down, Lp, stage-2 window = (Lp - 1) // up + 2)
RATES = {
    72_000: (1, 1, 1, 1, 33, 34),           # no resampling at all
    127_000: (1, 1, 72, 127, 4065, 58),     # largest prototype, largest up
    356_000: (1, 1, 18, 89, 2849, 160),     # q1 = 1 with a wide window
    704_000: (2, 10, 9, 44, 1409, 158),
    1_000_000: (5, 24, 9, 25, 801, 90),     # a rate the compat tests already use
    1_053_000: (3, 14, 8, 39, 1249, 158),
    1_408_000: (4, 20, 9, 44, 1409, 158),
    1_593_000: (6, 28, 16, 59, 1889, 120),
    1_900_000: (10, 48, 36, 95, 3041, 86),     # q1 = 10 off the canonical plan (a GUI slider rate)
    2_048_000: (8, 38, 9, 32, 1025, 115),
    2_750_000: (11, 52, 36, 125, 4001, 113),   # odd period (1375 -> 2750), history > 4096
    3_948_000: (7, 34, 6, 47, 1505, 252),      # widest designed window (design limit < 254)
    4_941_000: (9, 44, 8, 61, 1953, 246),
    4_968_000: (12, 58, 4, 23, 737, 186),
    4_953_000: (13, 62, 24, 127, 4065, 171),   # worst streaming history
    4_992_000: (13, 62, 3, 16, 513, 172),
}

RT1 = 512   # stage-1 outputs per tile of k_chanfilt_g; consecutive tiles are S1 = RT1 - window apart

U = 2.0 ** -24   # unit roundoff of float32


def plan_lengths(q1, L1, up, down, Lp, n):
    """tetra_etsi_lengths' formula: (M1, M2) of n input samples."""
    m1 = (n - L1) // q1 + 1 if n >= L1 else 0
    num = up * m1 - 1 - (Lp - 1)
    return m1, (num // down + 1 if num >= 0 else 0)


def chanfilt_m1(win):
    """Stage-1 output counts that put k_chanfilt_g's tile arithmetic at its edges for a stage-2 window
    of `win` taps: S1 (one tile exactly), S1 + 1 (a second tile of one stage-1 output), 512 (a full
    first tile), 2 S1, 2 S1 + 1, and a ragged value in the third tile."""
    S1 = RT1 - win
    return [S1, S1 + 1, RT1, 2 * S1, 2 * S1 + 1, 2 * S1 + S1 // 3 + 7]


def chanfilt_lengths(q1, L1, win):
    """The input lengths of chanfilt_m1: N = q1 (M1 - 1) + L1 rounded up to even (the extra sample
    adds a stage-1 output only when q1 = 1, where an odd M1 cannot be had)."""
    out = [q1 * (m1 - 1) + L1 for m1 in chanfilt_m1(win)]
    return [n + n % 2 for n in out]


def to_sc16(x):
    """complex -> ([..., 2] int16 on the SC16 grid, the complex64 samples the SC16 kernels compute on)."""
    q = np.stack([np.rint(x.real * 32768), np.rint(x.imag * 32768)], -1).clip(-32768, 32767).astype(np.int16)
    return q, (q[..., 0].astype(np.float32) / 32768 + 1j * (q[..., 1].astype(np.float32) / 32768)).astype(np.complex64)


def signal(E, fs, n, seed):
    """n samples of pi/4-DQPSK at fs with noise and a CFO (oracle/etsi.py modulate)."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, 2 * (int(n * 18000 / fs) + 16)).astype(np.uint8)
    return E.modulate(bits, n, fs=fs, t0=float(rng.uniform(4.0, 5.0)), phase0=float(rng.uniform(0, 6.28)),
                      cfo=float(rng.uniform(-600, 600)), snr_db=18.0, rng=rng)


def _components(x):
    x = np.asarray(x)
    return (x.real, x.imag) if np.iscomplexobj(x) else (x,)


def _stage(h, x, up, skip, step):
    """Both components of upfirdn(h, x, up, 1)[skip::step] in float64 (upfirdn on complex input would
    compute the same sums; per component keeps the absolute-value runs on the same code)."""
    return [upfirdn(np.asarray(h, np.float64), c.astype(np.float64), up, 1)[skip::step] for c in _components(x)]


def chanfilt_f64(x, h1, hp, q1, up, down):
    """The channel filter restated in float64 on the float32 taps, with the rounding bound of the
    float32 fmaf chains that compute it (oracle, kernel): (y complex128 [M2], bound float64 [M2], one
    bound for both components).

    Stage 1: x1[k] = sum_j h1[j] x[q1 k + j] = (x convolved with reversed h1)[L1 - 1 + q1 k].
    Stage 2: zero-stuff x1 by `up`, filter with hp, keep every `down`-th sample from Lp - 1 on.
    Bound, with u = 2^-24: a chain of n fmaf steps errs by at most n u sum|h||x| (gamma_n <= (n + 1) u
    here).  Stage 1: e1 = (L1 + 1) u sum|h1||x|.  Stage 2 sums at most nterm = (Lp - 1) // up + 2
    products of inputs that are each off by e1: (nterm + 1) u sum|hp||x1| + sum|hp| e1 (1 + (nterm + 1) u).
    The absolute sums are the same upfirdn runs on the absolute values."""
    h1, hp = np.asarray(h1, np.float32), np.asarray(hp, np.float32)
    L1, Lp = len(h1), len(hp)
    M1 = plan_lengths(q1, L1, up, down, Lp, len(x))[0]
    s1 = [c[L1 - 1:][::q1][:M1] for c in _stage(h1[::-1], x, 1, 0, 1)]
    a1 = [c[L1 - 1:][::q1][:M1] for c in _stage(np.abs(h1[::-1]), np.abs(x.real) + 1j * np.abs(x.imag), 1, 0, 1)]
    e1 = [(L1 + 1) * U * a for a in a1]
    y = _stage(hp, s1[0] + 1j * s1[1], up, Lp - 1, down)
    nterm = (Lp - 1) // up + 2
    ahp = np.abs(hp.astype(np.float64))
    bound = []
    for comp in range(2):
        a2 = upfirdn(ahp, np.abs(s1[comp]), up, 1)[Lp - 1::down]
        ee = upfirdn(ahp, e1[comp], up, 1)[Lp - 1::down]
        bound.append((nterm + 1) * U * a2 + ee * (1 + (nterm + 1) * U))
    return y[0] + 1j * y[1], np.stack(bound)


def check_against_f64(y32, x, h1, hp, q1, up, down, what):
    """y32 (float32 fmaf chains on x) against the float64 restatement: the restatement's length cut to
    tetra_etsi_lengths' M2, both components within the a-priori bound elementwise.  Returns the worst
    error as a fraction of the bound."""
    yr, bound = chanfilt_f64(x, h1, hp, q1, up, down)
    M2 = plan_lengths(q1, len(h1), up, down, len(hp), len(x))[1]
    assert 0 < M2 <= len(yr), (what, M2, len(yr))
    assert len(y32) == M2, (what, len(y32), M2)
    y64 = np.asarray(y32).astype(np.complex128)
    err = np.stack([np.abs(y64.real - yr.real[:M2]), np.abs(y64.imag - yr.imag[:M2])])
    b = bound[:, :M2]
    assert np.all(b > 0), what
    worst = float(np.max(err / b))
    assert np.all(err <= b), (what, worst, int(np.argmax(np.max(err / b, axis=0))))
    return worst


# ------------------------------------------------------------------------------ streaming history

def bare_plan(fs):
    """An EtsiPlan with the design's integers only (the window arithmetic reads no taps)."""
    from tetraear import _hip
    from tetraear.signal.etsi import rate_design
    p = _hip.EtsiPlan()
    p.q1, p.L1, p.up, p.down, p.Lp = rate_design(fs)
    return p


def chunk_patterns():
    rng = np.random.default_rng(4096)
    return [[131072] * 6, [2] * 3000 + [40000], [2 * int(v) for v in rng.integers(1, 30000, 40)]]


def history_needed(plan, patterns):
    """The largest x_total - s over the chunk patterns, from the product's own host function."""
    from tetraear import _hip
    fn = _hip.lib().tetra_etsi_stream_window
    s, W, yoff, ynext = (ctypes.c_int64() for _ in range(4))
    refs = [ctypes.byref(v) for v in (s, W, yoff, ynext)]
    worst = 0
    for sizes in patterns:
        x_total = y_done = 0
        for n in sizes:
            assert fn(plan, x_total, y_done, n, *refs) == 0
            worst = max(worst, x_total - s.value)
            x_total += n
            y_done = ynext.value
    return worst
