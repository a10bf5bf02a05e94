"""The exact time-tiled compat decimator (TETRA_COMPAT_TILED, csrc/compat_tiled.hip) on the GPU:
bit-identical to the sequential kernels for every shape, decimation factor, tile geometry and kind
of row -- whether its tiles verify (noisy rows at the built-in lengths) or are rerun (a warm-up far
too short, noiseless rows) -- and through process() / process_batch().
"""
import ctypes

import numpy as np
import pytest

from conftest import iq_to_c64

pytestmark = pytest.mark.gpu

TILE, WARM = 8192, 16384   # the built-in lengths (tests/_tiled_model.py)
NS = (28, 29, 1000, 8191, 8193, 40001, 131072)
QS = (7, 8, 9, 10)
KINDS = ("noise", "sc16", "zeros", "constant", "burst")
CMAX, NMAX = 64, 131072


@pytest.fixture(scope="module")
def hip():
    from tetraear import _hip
    c = _hip.ctx()
    assert c.arch().startswith("gfx950")
    return c


@pytest.fixture(scope="module")
def noise():
    """[64, 131072] complex64 white noise, made once; every test slices it and leaves it unchanged."""
    rng = np.random.default_rng(20260)
    x = np.empty((CMAX, NMAX), np.complex64)
    x.real = 0.25 * rng.standard_normal((CMAX, NMAX), np.float32)
    x.imag = 0.25 * rng.standard_normal((CMAX, NMAX), np.float32)
    x.setflags(write=False)
    return x


def _rows(noise, C, N, shift=0, kinds=KINDS):
    """A [C, N] batch whose row c is of kind kinds[(c + shift) % len(kinds)]."""
    x = np.array(noise[:C, :N])
    for c in range(C):
        kind = kinds[(c + shift) % len(kinds)]
        if kind == "sc16":
            x[c] = (np.round(x[c].real * 32768) / 32768 + 1j * (np.round(x[c].imag * 32768) / 32768)).astype(np.complex64)
        elif kind == "zeros":
            x[c] = 0
        elif kind == "constant":
            x[c] = 0.25 + 0.125j
        elif kind == "burst":
            x[c, max(1, N // 8):] = 0
    return np.ascontiguousarray(x)


def _plan(q, N):
    from tetraear import _hip
    from tetraear.signal.processor import compat_plan
    plan, m, _ = compat_plan(q * 240000.0, N, _hip.TETRA_CF32, decimator="tiled")
    assert plan.q == q
    return plan, m


def _stats(hip):
    st = (ctypes.c_int32 * 4)()
    hip.check(hip.lib.tetra_compat_tile_stats(hip.handle, st), "tetra_compat_tile_stats")
    return [int(v) for v in st]


def _both(hip, x, q):
    """(tetra_decimate_tiled, tetra_decimate) of the batch x as uint32 bit patterns, and the stats."""
    from tetraear import _hip
    C, N = x.shape
    plan, m = _plan(q, N)
    got = np.full((C, m), np.nan, np.complex64)
    want = np.full((C, m), np.nan, np.complex64)
    hip.check(hip.lib.tetra_decimate_tiled(hip.handle, plan, _hip.ptr(x), _hip.TETRA_CF32, C, N, _hip.ptr(got)),
              "tetra_decimate_tiled")
    st = _stats(hip)
    hip.check(hip.lib.tetra_decimate(hip.handle, plan, _hip.ptr(x), _hip.TETRA_CF32, C, N, _hip.ptr(want)),
              "tetra_decimate")
    return got.view(np.uint32), want.view(np.uint32), st


@pytest.mark.parametrize("tiles", ((0, 0), (512, 64), (512, 512)))
@pytest.mark.parametrize("C", (1, 3, 64))
def test_decimate_tiled_equals_sequential(hip, noise, C, tiles):
    """tetra_decimate_tiled == tetra_decimate bit for bit: odd lengths, fewer than two tiles (the
    sequential kernels run: all counters 0), a ragged last tile, every q, all five kinds of row.
    With a 64-sample warm-up no noisy tile verifies, so the rerun path demonstrably ran in both
    passes; an all-zero batch is the one input that cannot rerun (both trajectories are exactly 0)."""
    T = tiles[0] or TILE
    hip.check(hip.lib.tetra_compat_set_tiles(hip.handle, *tiles), "tetra_compat_set_tiles")
    try:
        for qi, q in enumerate(QS):
            for ni, N in enumerate(NS):
                # C = 1 has one row per call: give every kind its own call; else rotate the kinds
                for shift in (range(len(KINDS)) if C == 1 else (qi + ni,)):
                    x = _rows(noise, C, N, shift)
                    got, want, st = _both(hip, x, q)
                    assert np.array_equal(got, want), (C, N, q, tiles, shift, st, int((got != want).sum()))
                    K = -(-(N + 54) // T)
                    if N <= T:
                        assert st == [0, 0, 0, 0], (C, N, q, tiles, st)
                        continue
                    assert st[0] == st[2] == (K - 1) * 2 * C, (C, N, q, tiles, st)
                    assert 0 <= st[1] <= st[0] and 0 <= st[3] <= st[2]
                    only_zeros = C == 1 and KINDS[shift % len(KINDS)] == "zeros"
                    if tiles == (512, 64) and not only_zeros:
                        assert st[1] > 0 and st[3] > 0, (C, N, q, tiles, shift, st)
    finally:
        hip.check(hip.lib.tetra_compat_set_tiles(hip.handle, 0, 0), "tetra_compat_set_tiles")


@pytest.mark.parametrize("C", (1, 3, 64))
def test_default_tiles_verify_on_noise(hip, noise, C):
    """At the built-in lengths on 131072-sample noise rows (plain and SC16-quantised) every tile but
    the first is checked and at most 1 in 10 is rerun (a condition, not a measurement: the CPU model
    reruns none) -- the mode must not owe its exactness to falling back."""
    for q in QS:
        x = _rows(noise, C, NMAX, q, kinds=("noise", "sc16"))
        got, want, st = _both(hip, x, q)
        assert np.array_equal(got, want), (C, q, st)
        K = -(-(NMAX + 54) // TILE)
        print(f"C={C} q={q}: checked/rerun fwd {st[0]}/{st[1]} bwd {st[2]}/{st[3]}")
        assert st[0] == st[2] == (K - 1) * 2 * C, (C, q, st)
        assert 10 * st[1] <= st[0] and 10 * st[3] <= st[2], (C, q, st)


def test_set_tiles_validates(hip):
    for bad in ((32, 64), (64, 32), (100, 64), (512, 96), (0, 64), (512, 0), (-64, 64)):
        assert hip.lib.tetra_compat_set_tiles(hip.handle, *bad) != 0, bad
    hip.check(hip.lib.tetra_compat_set_tiles(hip.handle, 64, 64), "tetra_compat_set_tiles")
    hip.check(hip.lib.tetra_compat_set_tiles(hip.handle, 0, 0), "tetra_compat_set_tiles")


def test_process_tiled_matches_golden_and_sequential(hip, g1):
    """process() with decimator="tiled" on every g1_demod.npz case: the reference's hard symbols,
    and .symbols identical (values and dtype) to the sequential form's of the same call."""
    from tetraear.signal import SignalProcessor
    z, meta = g1
    ran = 0
    for i, m in enumerate(meta):
        x = iq_to_c64(z[f"c{i}_iq"])
        pt = SignalProcessor(m["fs"], decimator="tiled")
        ht = pt.process(x, m["freq_offset"])
        ran += sum(pt.tile_stats.values()) > 0
        ps = SignalProcessor(m["fs"], decimator="sequential")
        hs = ps.process(x, m["freq_offset"])
        assert np.array_equal(ht, z[f"c{i}_hard"]), (i, m)
        assert np.array_equal(ht, hs), (i, m)
        assert pt.symbols.dtype == ps.symbols.dtype and np.array_equal(pt.symbols, ps.symbols), (i, m)
    assert ran > 0, "no g1 case reached the tiled kernels"


def test_process_batch_tiled(hip, noise):
    """process_batch: 64 channels tiled == sequential bit for bit; 65 channels run the sequential
    kernels (the same results, all counters zero)."""
    from tetraear.signal import SignalProcessor
    N = 40001
    for C in (64, 65):
        x = np.concatenate([_rows(noise, 64, N, 1), _rows(noise, 1, N, 0)])[:C]
        fo = np.where(np.arange(C) % 3 == 0, 0.0, 1171.875 * (np.arange(C) % 7 - 3))
        pt = SignalProcessor(2.4e6, decimator="tiled")
        ht, st_, nt = pt.process_batch(x, fo)
        stats = pt.tile_stats
        hs, ss, ns = SignalProcessor(2.4e6, decimator="sequential").process_batch(x, fo)
        assert np.array_equal(nt, ns)
        for c in range(C):
            n = int(ns[c])
            assert np.array_equal(ht[c, :max(0, n - 1)], hs[c, :max(0, n - 1)]), (C, c)
            assert np.array_equal(st_[c, :n].view(np.uint64), ss[c, :n].view(np.uint64)), (C, c)
        if C == 64:
            K = -(-(N + 54) // TILE)
            assert stats["fwd_checked"] == stats["bwd_checked"] == (K - 1) * 2 * C, stats
        else:
            assert set(stats.values()) == {0}, stats


def test_seeded_sweep_tiled_vs_sequential(hip, noise):
    """20 seeded random (C <= 64, N in [28, 40000], q, tile, warm, kinds) cases, the tiled entry point
    against the sequential one: the cross-form check of a new entry point."""
    rng = np.random.default_rng(99)
    try:
        for case in range(20):
            C = int(rng.integers(1, 65))
            N = int(rng.integers(28, 40001))
            q = int(rng.choice(QS))
            tile = 64 * int(rng.integers(1, 65))
            warm = 64 * int(rng.integers(1, 129))
            shift = int(rng.integers(0, 5))
            hip.check(hip.lib.tetra_compat_set_tiles(hip.handle, tile, warm), "tetra_compat_set_tiles")
            got, want, st = _both(hip, _rows(noise, C, N, shift), q)
            assert np.array_equal(got, want), (case, C, N, q, tile, warm, shift, st)
            if N > tile:
                assert st[0] == st[2] == (-(-(N + 54) // tile) - 1) * 2 * C, (case, st)
            else:
                assert st == [0, 0, 0, 0]
    finally:
        hip.check(hip.lib.tetra_compat_set_tiles(hip.handle, 0, 0), "tetra_compat_set_tiles")
