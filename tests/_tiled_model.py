"""CPU model of the exact time-tiled compat decimator (include/tetra_hip.h, TETRA_COMPAT_TILED).

scipy.signal.decimate(x, q) on complex64 is sosfiltfilt of cheby1(8, 0.05, 0.8/q): one forward and
one backward `sosfilt` over the odd extension ext[0, L), L = N + 54.  Here each pass is cut into
tiles [kT, min((k+1)T, L)).  Tile k is run *speculatively* from an all-zero state W samples early
(from the pass's exact start state when that reaches sample 0); the state it has just before sample
kT (S_k) is compared, as 32-bit patterns, with the state the resolved tile k-1 ended in (E*_{k-1}).
Equal: the tile's outputs and end state are the sequential run's.  Not equal: the tile is rerun from
E*_{k-1}.  Either way every output is scipy's, bit for bit; W only decides how often a rerun happens.

A stream is one real component of one row (the SOS coefficients are real, so the real and
imaginary parts never mix); checks and reruns are counted per stream, as the GPU kernels do.
This file is the specification the built-in tile and warm-up lengths were chosen with
(tools/compat_tile_sweep.py).
"""
import numpy as np
from scipy import signal as _ss

TILE, WARM = 8192, 16384   # the built-in defaults (csrc/compat_tiled.hip: TL_TILE, TL_WARM)
PAD = 27                   # sosfiltfilt's default padlen for 4 sections


def _odd_ext(x, n):
    return np.concatenate((2 * x[0:1] - x[n:0:-1], x, 2 * x[-1:] - x[-2:-(n + 2):-1]))


def _same_bits(a, b):
    """Per component: are the 8 state words of a and b equal as uint32 patterns? -> (re, im)."""
    a = np.ascontiguousarray(a, np.complex64).view(np.uint32).reshape(-1, 2)
    b = np.ascontiguousarray(b, np.complex64).view(np.uint32).reshape(-1, 2)
    return bool((a[:, 0] == b[:, 0]).all()), bool((a[:, 1] == b[:, 1]).all())


def tiled_pass(sos, zi, seq, tile, warm):
    """One sosfilt pass over `seq` (complex64) from state zi * seq[0], time-tiled.
    Returns (output, tiles checked, tiles rerun), the counts summed over the two components."""
    L = len(seq)
    out = np.empty(L, np.complex64)
    K = -(-L // tile)
    z0 = (zi * seq[0]).astype(np.complex64)
    zero = np.zeros_like(z0)
    checked = rerun = 0
    e_true = None
    for k in range(K):
        lo, hi = k * tile, min((k + 1) * tile, L)
        a = max(0, lo - warm)
        z = z0 if a == 0 else zero
        if lo > a:
            _, z = _ss.sosfilt(sos, seq[a:lo], zi=z)
        s_k = z
        y, e_k = _ss.sosfilt(sos, seq[lo:hi], zi=s_k)
        if k > 0:   # a tile that started at sample 0 ran from the exact state: it always matches
            ok = _same_bits(s_k, e_true)
            checked += 2
            rerun += 2 - sum(ok)
            if not all(ok):   # the rerun from the true state is right for both components
                y, e_k = _ss.sosfilt(sos, seq[lo:hi], zi=e_true)
        out[lo:hi] = y
        e_true = e_k
    return out, checked, rerun


def decimate_tiled(x, q, tile=TILE, warm=WARM):
    """scipy.signal.decimate(x, q) for a 1-D complex64 x through the tiled scheme.
    Returns (y, stats): stats = [forward checked, forward rerun, backward checked, backward rerun]."""
    x = np.ascontiguousarray(x, np.complex64)
    if len(x) <= PAD:
        raise ValueError("The length of the input vector x must be greater than padlen, which is 27.")
    sos = np.asarray(_ss.cheby1(8, 0.05, 0.8 / q, output="sos"), dtype=np.complex64)
    zi = _ss.sosfilt_zi(sos)
    ext = _odd_ext(x, PAD)
    f, fc, fr = tiled_pass(sos, zi, ext, tile, warm)
    b, bc, br = tiled_pass(sos, zi, np.ascontiguousarray(f[::-1]), tile, warm)
    return np.ascontiguousarray(b[::-1][PAD:-PAD][::q]), [fc, fr, bc, br]
