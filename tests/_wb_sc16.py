"""Helpers of the wideband SC16 tests: a complex64 capture quantised to the radio's int16 pairs, and
the complex64 capture those pairs stand for (the SC16 specification is "cf32 of x / 32768")."""
import numpy as np


def shift_of(x):
    """The smallest k >= 0 with max(|re|, |im|) * 2^-k * 32768 <= 32767."""
    v = np.ascontiguousarray(x, np.complex64).view(np.float32)
    peak = float(np.abs(v).max()) if v.size else 0.0
    k = 0
    while peak * 2.0 ** -k * 32768.0 > 32767.0:
        k += 1
    return k


def q16(x, bits=16):
    """[Nw] complex -> [Nw, 2] int16: scaled by the exact power of two 2^-k (shift_of) into full scale
    of a `bits`-bit converter (16: +-32767; 12: +-2047, the BladeRF ADC), rounded."""
    v = np.ascontiguousarray(x, np.complex64).view(np.float32).reshape(-1, 2)
    full = float(1 << (bits - 1))
    q = np.rint(v.astype(np.float64) * (full * 2.0 ** -shift_of(x)))
    assert np.abs(q).max(initial=0.0) <= full - 1
    return q.astype(np.int16)


def twin(q):
    """[Nw, 2] int16 -> [Nw] complex64, each component / 32768 (exact in float32)."""
    q = np.asarray(q)
    return (q.astype(np.float32) / np.float32(32768)).view(np.complex64)[:, 0].copy()


def canon(o):
    """Frames (dicts of numbers, lists and numpy arrays) as plain Python, for ==."""
    if isinstance(o, dict):
        return {k: canon(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [canon(v) for v in o]
    if isinstance(o, np.ndarray):
        return o.tolist()
    if isinstance(o, np.generic):
        return o.item()
    return o
