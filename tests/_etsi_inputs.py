"""Input rows for the ETSI demod built on the CPU: weak, loud and non-TETRA (TEST INFRASTRUCTURE).

Every other ETSI test feeds the demod a synthetic downlink at amplitude about 0.5.  The rows here
cover what a real batch also holds -- idle channels, tones, captures not scaled to +-1 -- and the
arithmetic between "no signal" and "nominal signal": subnormal products and sums, sqrtf and
divisions of subnormals, overflow to inf and inf - inf = NaN inside the timing stage.  All rows
come from oracle/etsi.py's transmitter with fixed seeds, so tests/test_etsi_inputs.py (oracle only:
proves the rows mean what is claimed) and tests/test_gpu_etsi_inputs.py (kernels against the
oracle, bit for bit) see the same bytes.  No input sample is inf or NaN.

  base      a burst stream (SB, NDB, NDB(p), NDB ...) at amplitude 0.5, 300 Hz CFO, 14 dB Es/N0
  ladder    base x 2^k, exact in float32, k in LADDER; WINDOW is the range of k over which the
            receiver has to be scale-exact (same dibits, soft bits, diagnostics; symbols x 2^k)
  classes   rows that are not TETRA (CLASSES)
  sc16      the rows an int16 capture can hold exactly (SC16_CLASSES), as [N, 2] int16
  built72   72 kHz rows for the timing stage alone (BUILT72), M2B samples each
"""
import functools

import numpy as np

import etsi as E

NMAX = 134408        # the longest row any test cuts from base (3.9 bursts)
N_DEFAULT = 20000    # 141 symbols: two full Gardner blocks and a partial one
FS = 2.4e6
CELL = E.scramble_init(262, 1, 5)
BASE_KINDS = (E.BURST_SB, E.BURST_NDB_N, E.BURST_NDB_P, E.BURST_NDB_N, E.BURST_NDB_P)
# -130 (the samples and y subnormal) and -120 (y normal, the products of small taps and samples
# underflow inside both filter stages) stand below the regimes of the timing stage: they are there
# for the channel filter's fmaf chains and stage 2's MFMA
LADDER = (-130, -120, -100, -70, -64, -41, -40, -19, -18, -12, -11, -1, 0, 4, 5, 12, 13, 14, 28, 29, 57, 58, 60)
WINDOW = (-16, 10)   # the scale-exact window the receiver must cover (a condition, not a measurement)
CLASSES = ("zeros", "dc", "sc16_min", "tone_0", "tone_3k", "tone_4k5", "tone_200k", "lsb_noise", "square",
           "impulse", "base_silence", "silence_base", "neg_zeros")
SC16_CLASSES = ("zeros", "dc", "sc16_min", "lsb_noise", "square", "impulse", "tone_0", "tone_3k", "tone_4k5",
                "tone_200k", "base_0.5", "base_2^-6", "base_2^-11")
M2B = 648            # built 72 kHz rows: 161 on-sample symbols = 160 dibits
BUILT72 = ("const", "class1", "axis_ties", "half_even", "w_zero_blocks")


def _ro(a):
    a.setflags(write=False)
    return a


def scale(x, k):
    """x * 2^k, exact in float32 (ldexp on the parts; no sample of these rows overflows, and only the
    k = -130 rung's are subnormal and so rounded)."""
    v = np.ascontiguousarray(x, np.complex64).view(np.float32)
    with np.errstate(over="raise"):
        return np.ldexp(v, np.int32(k)).astype(np.float32).view(np.complex64)


def c64(re, im):
    """complex64 from float32 parts, signed zeros kept (re + 1j * im would lose them)."""
    out = np.empty(np.shape(re) + (2,), np.float32)
    out[..., 0] = re
    out[..., 1] = im
    return out.view(np.complex64)[..., 0]


@functools.lru_cache(maxsize=None)
def base_long(fs=FS):
    """(samples [NMAX] c64, jobs): the burst stream every signal row is cut from, sampled at fs.  The
    first burst starts 12 symbols in, past the channel filter's start-up, so a row of NMAX samples at
    2.4 MSps holds three whole bursts."""
    rng = np.random.default_rng(20261019)
    bits, jobs = E.burst_stream(rng, len(BASE_KINDS), E.scramble_seq(CELL, 432), kinds=list(BASE_KINDS))
    x = E.modulate(bits, NMAX, fs=fs, t0=-12.0, cfo=300.0, snr_db=14.0, rng=rng, amp=0.5)
    return _ro(x), jobs


def base(N=N_DEFAULT, start=0, fs=FS):
    return base_long(fs)[0][start:start + N]


def planted_payloads():
    """The type-1 payloads of base's bursts: {tuple(bits padded to 268)}."""
    return {tuple(np.pad(t1, (0, 268 - len(t1)))) for _, jobs in base_long()[1] for _, t1 in jobs}


@functools.lru_cache(maxsize=None)
def ladder_rows(N=N_DEFAULT, fs=FS):
    """[len(LADDER), N] c64: base x 2^k."""
    return _ro(np.stack([scale(base(N, fs=fs), k) for k in LADDER]))


def _tone(f, N, amp=0.5, ph=0.7):
    return (amp * np.exp(1j * (ph + 2 * np.pi * f * np.arange(N) / FS))).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def class_rows(N=N_DEFAULT):
    """[len(CLASSES), N] c64, in the order of CLASSES."""
    rng = np.random.default_rng(77)
    b = base(N)
    h = (N // 4) * 2
    z = np.zeros(N, np.complex64)
    sq = c64(np.where(rng.integers(0, 2, N) == 1, 32767, -32768).astype(np.float32) / np.float32(32768),
             np.where(rng.integers(0, 2, N) == 1, 32767, -32768).astype(np.float32) / np.float32(32768))
    lsb = c64(rng.integers(-1, 2, N).astype(np.float32) / np.float32(32768),
              rng.integers(-1, 2, N).astype(np.float32) / np.float32(32768))
    imp = z.copy()
    imp[N // 2] = 1.0
    rows = dict(zeros=z, dc=np.full(N, 0.25 + 0.125j, np.complex64), sc16_min=np.full(N, -1.0 - 1.0j, np.complex64),
                tone_0=_tone(0.0, N), tone_3k=_tone(3000.0, N), tone_4k5=_tone(4500.0, N),
                tone_200k=_tone(200e3, N), lsb_noise=lsb, square=sq, impulse=imp,
                base_silence=np.concatenate([b[:h], z[h:]]), silence_base=np.concatenate([z[:h], b[h:]]),
                neg_zeros=c64(np.full(N, -0.0, np.float32), np.full(N, -0.0, np.float32)))
    return _ro(np.stack([rows[n] for n in CLASSES]))


def to_sc16(x):
    """complex rows -> [..., 2] int16, rounded and clipped as a capture would be."""
    x = np.asarray(x)
    return np.stack([np.rint(x.real.astype(np.float64) * 32768), np.rint(x.imag.astype(np.float64) * 32768)],
                    -1).clip(-32768, 32767).astype(np.int16)


def sc16_to_cf32(q):
    """The samples the SC16 kernels compute on: int16 / 32768, exact."""
    return c64(q[..., 0].astype(np.float32) / np.float32(32768), q[..., 1].astype(np.float32) / np.float32(32768))


@functools.lru_cache(maxsize=None)
def sc16_rows(N=N_DEFAULT):
    """[len(SC16_CLASSES), N, 2] int16, in the order of SC16_CLASSES (tones and base rounded to int16;
    base at 2^-11 is a few LSB)."""
    cls = dict(zip(CLASSES, class_rows(N)))
    rows = {n: cls[n] for n in SC16_CLASSES if n in cls}
    rows["base_0.5"] = base(N)
    rows["base_2^-6"] = scale(base(N), -6)
    rows["base_2^-11"] = scale(base(N), -11)
    return _ro(np.stack([to_sc16(rows[n]) for n in SC16_CLASSES]))


# ------------------------------------------------------------------------------ 72 kHz rows
# A row with samples in class 0 mod 4 only has Oerder-Meyr X = (A0, 0): base = -0.0, kstart = 1 and the
# loop samples y at t = 4 (1 + l) exactly (cubic weights 0, 1, 0, 0; the Gardner error is 0 because the
# mid samples are), so symbol j IS y[4 (1 + j)] and d_j = s_j conj(s_{j-1}) can be placed to the bit.

def _on_sample(sym):
    """M2B-sample row whose symbols are sym (161 of them; parts as float32 [n, 2], signed zeros kept)."""
    assert len(sym) == (M2B - 3 - 4) // 4 + 1
    y = np.zeros((M2B, 2), np.float32)
    y[4:4 + 4 * len(sym):4] = sym
    return y.view(np.complex64)[:, 0]


_UNITS = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.float32)


def _axis_ties(rng):
    """Symbols u u g u u g ...: u a unit on an axis (its zero part +0 or -0 at random), g = (+-1, +-1).
    u-u steps give d_j exactly on an axis (d^4 = +1, with +0 and -0 in the other part), u-g and g-u
    steps d_j = (+-1, +-1) (d^4 = -4): Z is a negative real with a zero of either sign beside it, the
    rotation (1, +-0), and every axis d_j is a tie in one of its two decisions.  (The cubic's zero
    weights turn a -0.0 part of y into +0 in the symbol; the -0 ties come from d_j's products.)"""
    n = (M2B - 3 - 4) // 4 + 1
    s = np.zeros((n, 2), np.float32)
    for j in range(n):
        if j % 3 == 2:
            s[j] = rng.choice([-1.0, 1.0], 2)
        else:
            s[j] = _UNITS[rng.integers(4)]
            s[j][s[j] == 0] = rng.choice([-0.0, 0.0], 1)
    return s


def _mul(a, b, conj_b=False):
    bi = -b[1] if conj_b else b[1]
    return np.array([a[0] * b[0] - a[1] * bi, a[0] * bi + a[1] * b[0]], np.float32)


def _half_even(rng):
    """Symbols u g u g ... u: u a unit on an axis, g in turn an axis-swapped / sign variant of
    41 (3, 4) = (123, 164) and of 3 (8, 15) = (24, 45).  Every d_j is a variant of its g, |d| is 205 or
    51 in equal numbers -- mean |d| = 128 exactly, the soft scale 64 / 128 -- and d^4 has a negative
    real part for both ((3 + 4i)^4 = -527 - 336i, (8 + 15i)^4 = -31679 - 77280i), so with the imaginary
    parts cancelling the rotation is the identity and the soft bits are 61.5, 82, 12 and 22.5 before
    rounding: 62 and 22 under round-half-even, 62 and 23 under round-half-away."""
    n = (M2B - 3 - 4) // 4 + 1
    s = np.zeros((n, 2), np.float32)
    fam = [(123.0, 164.0), (24.0, 45.0)]
    for j in range(n):
        if j % 2 == 0:
            s[j] = _UNITS[rng.integers(4)]
        else:
            a, b = fam[(j // 2) % 2]
            if rng.integers(2):
                a, b = b, a
            s[j] = (a * rng.choice([-1.0, 1.0]), b * rng.choice([-1.0, 1.0]))
    return s


HALF_EVEN_SOFT = (12, 22, 62, 82)   # |soft bit| values of the half_even row


@functools.lru_cache(maxsize=None)
def built72_rows():
    """[len(BUILT72), M2B] c64, in the order of BUILT72."""
    rx = E.Receiver()
    const = np.full(M2B, 0.3 + 0.1j, np.complex64)
    rng = np.random.default_rng(5)
    class1 = np.zeros(M2B, np.complex64)
    class1[1::4] = (rng.standard_normal(M2B // 4) + 1j * rng.standard_normal(M2B // 4)).astype(np.complex64) * 0.3
    axis = _on_sample(_axis_ties(np.random.default_rng(6)))
    # the half_even row: the first seed whose imaginary 4th-power sums cancel to the rotation (1, +-0)
    # in the oracle's summation order (the terms are +-v pairs, but f32 sums of them need not be 0)
    for seed in range(200):
        half = _on_sample(_half_even(np.random.default_rng(1000 + seed)))
        _, sb, _, diag = rx.timing(half)
        if diag[2] == 1.0 and diag[3] == 0.0 and set(np.abs(sb.astype(np.int32)).tolist()) == set(HALF_EVEN_SOFT):
            break
    else:
        raise AssertionError("no half_even row found")
    y = rx.chanfilt(base(NMAX // 4))
    wz = np.zeros(M2B, np.complex64)
    wz[280:540] = y[280:540]   # blocks 0 and 2 of the Gardner loop see zeros only (W == 0)
    rows = dict(const=const, class1=class1, axis_ties=axis, half_even=half, w_zero_blocks=wz)
    return _ro(np.stack([rows[n] for n in BUILT72]))


# ------------------------------------------------------------------------------ streaming
STREAM_CF32 = ("base0", "zeros", "base1 x 2^-18", "zeros(2)", "base2 x 2^12", "lsb_noise", "base3")
# SC16 cannot hold base x 2^-18 or x 2^12: their nearest int16 analogues stand in (a few LSB, full scale)
STREAM_SC16 = ("base0", "zeros", "base1 x 2^-11", "zeros(2)", "square", "lsb_noise", "base3")


@functools.lru_cache(maxsize=None)
def stream_chunks():
    """Chunks of one capture for E.Stream / EtsiStream: consecutive N_DEFAULT-sample pieces of base with
    silence, a weak, a loud and a noise-only stretch between them."""
    N = N_DEFAULT
    cls = dict(zip(CLASSES, class_rows(N)))
    b = [base(N, i * N) for i in range(4)]
    return [b[0], cls["zeros"], _ro(scale(b[1], -18)), _ro(np.zeros(2, np.complex64)), _ro(scale(b[2], 12)),
            cls["lsb_noise"], b[3]]


@functools.lru_cache(maxsize=None)
def stream_chunks_sc16():
    N = N_DEFAULT
    cls = dict(zip(CLASSES, class_rows(N)))
    b = [base(N, i * N) for i in range(4)]
    rows = [b[0], cls["zeros"], scale(b[1], -11), np.zeros(2, np.complex64), cls["square"], cls["lsb_noise"], b[3]]
    return [_ro(to_sc16(r)) for r in rows]
