"""The exact time-tiled compat decimator on the CPU: its numpy/scipy model (tests/_tiled_model.py)
against scipy.signal.decimate, the rerun rate at the built-in tile lengths, and the host-only form
selection of the product (tetra_compat_forms).  The GPU kernels are held to the sequential kernels
bit for bit in tests/test_gpu_tiled.py.
"""
import os
import sys

import numpy as np
import pytest
from scipy import signal

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _signals  # noqa: E402
import _tiled_model as model  # noqa: E402

NS = (28, 1000, 8193, 131072)
TILES = ((model.TILE, model.WARM), (512, 64), (1024, 1024))
ROWS = _signals.SWEEP_FAMILIES + ("constant", "zeros", "burst")
RATE = {7: 1.8e6, 10: 2.4e6}


def _row(name, n, fs):
    rng = np.random.default_rng(2024)
    if name in _signals.SWEEP_FAMILIES:
        return _signals.family(name, rng, n, fs)[0]
    if name == "constant":
        return np.full(n, 0.25 + 0.125j, np.complex64)
    if name == "zeros":
        return np.zeros(n, np.complex64)
    x = np.zeros(n, np.complex64)   # a burst followed by exact zeros
    m = max(1, n // 8)
    x[:m] = _signals.family("noise", rng, m, fs)[0]
    return x


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


@pytest.mark.parametrize("q", (7, 10))
@pytest.mark.parametrize("name", ROWS)
def test_model_equals_scipy_decimate(name, q):
    """Bit-identical to scipy for every row, tile geometry and length.  Noiseless rows (no rounding
    noise to merge the warm-started trajectory into the sequential one) must get there through
    reruns: asserted wherever a tile starts from the zero state, i.e. (K - 1) T > W.  The all-zero
    row is the exception by construction: both trajectories are exactly zero, so nothing reruns."""
    for n in NS:
        x = _row(name, n, RATE[q])
        want = signal.decimate(x, q)
        assert want.dtype == np.complex64
        for tile, warm in TILES:
            got, st = model.decimate_tiled(x, q, tile, warm)
            assert got.dtype == np.complex64 and got.shape == want.shape
            assert np.array_equal(_bits(got), _bits(want)), (name, q, n, tile, warm, st)
            K = -(-(n + 2 * model.PAD) // tile)
            assert st[0] == st[2] == 2 * (K - 1)
            if name in ("constant", "burst") and (K - 1) * tile > warm:
                assert st[1] > 0 and st[3] > 0, (name, q, n, tile, warm, st)
            if name == "zeros":
                assert st[1] == 0 and st[3] == 0


def test_default_tiles_rarely_rerun():
    """At the built-in lengths, over the GUI's call pattern (sweep_chunks seeds 0-3 x 10 chunks,
    q = 10), at most 2 % of the checked tiles rerun -- a mode that always fell back would be exact
    and pointless.  (tools/compat_tile_sweep.py: 0 reruns at every q in 7..10.)"""
    checked = rerun = 0
    for seed in range(4):
        for _, fam, _, x, _ in _signals.sweep_chunks(seed, 10):
            _, st = model.decimate_tiled(x, 10)
            checked += st[0] + st[2]
            rerun += st[1] + st[3]
    print(f"{rerun} of {checked} checked tiles rerun")
    assert checked == 4 * 10 * 2 * 2 * 16
    assert rerun <= 0.02 * checked


def _forms(fs, N, C=1, decimator=None, fmt=None):
    from tetraear import _hip
    from tetraear.signal.processor import SignalProcessor, compat_forms, compat_plan
    dec = SignalProcessor(fs, mode="compat", decimator=decimator).decimator
    plan, _, _ = compat_plan(fs, N, _hip.TETRA_CF32 if fmt is None else fmt, decimator=dec)
    return compat_forms(plan, C, N)


def test_form_selection(monkeypatch):
    """Host-only: where decimator="tiled" runs the tiled kernels, and that nothing else does."""
    from tetraear import _hip
    monkeypatch.delenv("TETRAEAR_COMPAT_DECIMATOR", raising=False)
    rates = (1.8e6, 1.9e6, 2.0e6, 2.1e6, 2.2e6, 2.3e6, 2.4e6)
    for fs in rates:
        for C in (1, 64):
            f = _forms(fs, 131072, C, "tiled")
            assert f["decimate"] == "tiled" and f["filtfilt"] == "sequential", (fs, C, f)
        assert _forms(fs, 131072, 65, "tiled")["decimate"] == "sequential"
        assert _forms(fs, 131072, 1, "tiled", _hip.TETRA_CF64)["decimate"] == "sequential"
        for N in (28, 1000, model.TILE):
            assert _forms(fs, N, 1, "tiled")["decimate"] == "sequential", (fs, N)
        assert _forms(fs, model.TILE + 1, 1, "tiled")["decimate"] == "tiled"
        for C in (1, 64, 65):   # built with no argument: sequential everywhere
            f = _forms(fs, 131072, C)
            assert f["decimate"] == "sequential" and f["filtfilt"] == "sequential", (fs, C, f)
    assert _forms(3.2e6, 131072, 1, "tiled")["decimate"] == "sequential"   # q = 13: outside 7..10
    assert _forms(2.4e6, 131072, 1, "blocked")["decimate"] == "blocked"
    monkeypatch.setenv("TETRAEAR_COMPAT_DECIMATOR", "tiled")
    assert _forms(2.4e6, 131072)["decimate"] == "tiled"
    assert _forms(2.4e6, 131072, decimator="sequential")["decimate"] == "sequential"
