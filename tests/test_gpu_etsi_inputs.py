"""The ETSI demod on weak, loud and non-TETRA input (tests/_etsi_inputs.py) against the CPU oracle.

No tolerance anywhere: every array is compared with np.array_equal, the diagnostics with
equal_nan=True (NaN where the oracle has NaN, the same value elsewhere).  All rows of a class set go
through one launch per entry point, so a degenerate channel (silence, a tone, subnormal or
overflowing arithmetic, no timing phase at all) also must not disturb its neighbours.
tests/test_etsi_inputs.py proves on the oracle alone what the rows hold.

The top rungs (k >= 57) put inf and NaN into the timing stage.  Every loop of the paths under test
ends with them: the Gardner loop's `valid` is false in every lane for a NaN position (nv = 0, break),
its addresses come from the position only, never from sample values; the CFO wave leaves on
PROG_DONE, stored unconditionally; k_timing's ring loads and the channel filters (k_chanfilt_r,
k_chanfilt, k_chanfilt_g) loop over integer ranges that do not depend on the samples.
"""
import ctypes
import functools

import numpy as np
import pytest

import etsi as E
import _etsi_inputs as I

pytestmark = pytest.mark.gpu

LENGTHS = [262144, 134408, 131072, 70002, 70001, 40000, 23408, 20000, 9001, 3000]   # test_demod_lengths_vs_oracle
FORMS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]                              # test_timing_forms_bit_exact
IN_WINDOW = [k for k in I.LADDER if I.WINDOW[0] <= k <= I.WINDOW[1]]


def _kernel(plan, fmt, N):
    """(name, static LDS bytes) of the channel-filter kernel the fused demod call takes at N: the LDS
    size tells the variants of one name apart (fused or not, cf32 or SC16)."""
    from tetraear import _hip
    c = _hip.ctx()
    name, lds = ctypes.create_string_buffer(64), ctypes.c_int64(0)
    c.check(c.lib.tetra_etsi_kernel_info(c.handle, plan, fmt, N, 1, name, 64, ctypes.byref(lds)), "kernel_info")
    return name.value.decode(), lds.value


def _kernel_lengths(fmt):
    """{kernel: the smallest N of LENGTHS that selects it} (odd lengths trimmed as demod_batch does)."""
    from tetraear.signal.etsi import etsi_plan
    plan = etsi_plan()
    reach = {}
    for N in sorted(n - n % 2 for n in LENGTHS):
        reach.setdefault(_kernel(plan, fmt, N), N)
    return reach


def _rows(N):
    """Ladder and class rows of N samples: (labels, [R, N] c64)."""
    return ([("k", k) for k in I.LADDER] + [("class", n) for n in I.CLASSES],
            np.concatenate([I.ladder_rows(N), I.class_rows(N)]))


@functools.lru_cache(maxsize=None)
def _oracle(N, fs=2.4e6):
    """The oracle on _rows(N): per row (y, sym, soft, hard, diag)."""
    rx = E.Receiver(fs)
    rows = _rows(N)[1] if fs == 2.4e6 else np.concatenate([I.ladder_rows(N, fs), I.class_rows(N)])
    out = []
    with np.errstate(all="ignore"):
        for r in rows:
            y = rx.chanfilt(r)
            out.append((y,) + rx.timing(y))
    return out


def _same(got, want, labels, what):
    """got = (hard, soft, sym, ns, diag) of a batch, want = per row (sym, soft, hard, diag)."""
    hard, soft, sym, ns, diag = got
    for r, (so, sbo, ho, dg) in enumerate(want):
        n, tag = int(ns[r]), (what, labels[r])
        assert n == len(so), tag
        assert np.array_equal(sym[r, :n], so), tag
        assert np.array_equal(soft[r, :2 * max(n - 1, 0)], sbo), tag
        assert np.array_equal(hard[r, :max(n - 1, 0)], ho), tag
        if diag is not None:
            assert np.array_equal(diag[r], dg, equal_nan=True), tag + (diag[r], dg)


def _demod(x, plan=None, fs=2.4e6):
    """tetra_demod_etsi_fmt on a batch (cf32 [C, N] or SC16 [C, N, 2]) with diagnostics."""
    from tetraear import _hip
    from tetraear.signal.etsi import EtsiReceiver, lengths
    if plan is None:
        rx = EtsiReceiver(fs)
        return rx.demod_batch(x) + (rx.diag,)
    fmt = _hip.TETRA_SC16 if x.dtype == np.int16 else _hip.TETRA_CF32
    C, N = x.shape[:2]
    _, _, sm = lengths(plan, N)
    sym, soft = np.zeros((C, sm), np.complex64), np.zeros((C, 2 * sm), np.int8)
    hard, ns, diag = np.zeros((C, sm), np.uint8), np.zeros(C, np.int32), np.zeros((C, 4), np.float32)
    c = _hip.ctx()
    c.check(c.lib.tetra_demod_etsi_fmt(c.handle, plan, _hip.ptr(np.ascontiguousarray(x)), fmt, C, N, _hip.ptr(sym),
                                       _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(ns), sm, _hip.ptr(diag)), "demod")
    return hard, soft, sym, ns, diag


@pytest.fixture(scope="module")
def demod_cf32():
    """(a): {N: outputs of the cf32 demod on _rows(N)} at N_DEFAULT and at the smallest length of
    LENGTHS for every kernel the list reaches."""
    from tetraear import _hip
    reach = _kernel_lengths(_hip.TETRA_CF32)
    out = {N: _demod(np.ascontiguousarray(_rows(N)[1])) for N in sorted(set(reach.values()) | {I.N_DEFAULT})}
    return reach, out


def test_demod_cf32_every_kernel(demod_cf32):
    from tetraear import _hip
    from tetraear.signal.etsi import etsi_plan
    reach, out = demod_cf32
    names = {k[0] for k in reach}
    assert names == {_kernel(etsi_plan(), _hip.TETRA_CF32, n - n % 2)[0] for n in LENGTHS}
    assert names == {"k_chanfilt_r", "k_chanfilt"} and len(reach) >= 2, reach
    assert max(reach.values()) == 134408   # past the LDS output buffer: the component path
    print("kernels covered (cf32):", {k: n for k, n in reach.items()})
    for N, got in out.items():
        _same(got, [w[1:] for w in _oracle(N)], _rows(N)[0], N)


def test_demod_sc16_every_kernel():
    """(b): the rows an int16 capture can hold, at every SC16 kernel LENGTHS reaches, against the
    oracle on the 1/32768-scaled samples."""
    from tetraear import _hip
    reach = _kernel_lengths(_hip.TETRA_SC16)
    assert {k[0] for k in reach} == {"k_chanfilt_r", "k_chanfilt"} and len(reach) >= 3, reach
    print("kernels covered (SC16):", {k: n for k, n in reach.items()})
    rx = E.Receiver()
    for N in sorted(set(reach.values()) | {I.N_DEFAULT}):
        q = np.ascontiguousarray(I.sc16_rows(N))
        want = [rx.demod(x) for x in I.sc16_to_cf32(q)]
        _same(_demod(q), want, I.SC16_CLASSES, ("sc16", N))


@pytest.fixture(scope="module")
def y72():
    """The channel filter alone (tetra_etsi_chanfilt_fmt, y in HBM) on the default rows: y equals the
    oracle's, and feeds the timing forms."""
    from tetraear import _hip
    from tetraear.signal.etsi import etsi_plan, lengths
    labels, x = _rows(I.N_DEFAULT)
    plan = etsi_plan()
    _, M2, _ = lengths(plan, I.N_DEFAULT)
    y = np.zeros((len(x), M2), np.complex64)
    c = _hip.ctx()
    c.check(c.lib.tetra_etsi_chanfilt_fmt(c.handle, plan, _hip.ptr(np.ascontiguousarray(x)), _hip.TETRA_CF32, len(x),
                                          I.N_DEFAULT, _hip.ptr(y)), "chanfilt_fmt")
    for r, w in enumerate(_oracle(I.N_DEFAULT)):
        assert np.array_equal(y[r], w[0]), labels[r]
    return y


def _timing(y):
    from tetraear import _hip
    from tetraear.signal.etsi import etsi_plan
    C, M2 = y.shape
    sm = M2 // 4 + 2
    sym, soft = np.zeros((C, sm), np.complex64), np.zeros((C, 2 * sm), np.int8)
    hard, ns, diag = np.zeros((C, sm), np.uint8), np.zeros(C, np.int32), np.zeros((C, 4), np.float32)
    c = _hip.ctx()
    c.check(c.lib.tetra_etsi_timing(c.handle, etsi_plan(), _hip.ptr(np.ascontiguousarray(y)), C, M2, _hip.ptr(sym),
                                    _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(ns), sm, _hip.ptr(diag)), "timing")
    return hard, soft, sym, ns, diag


@pytest.mark.parametrize("ring,lean", FORMS)
def test_timing_forms(y72, ring, lean, monkeypatch):
    """(c): every k_timing form on the filter outputs of the rows and on the built 72 kHz rows."""
    monkeypatch.setenv("TETRA_TIMING_RING", str(ring))
    monkeypatch.setenv("TETRA_TIMING_LEAN", str(lean))
    _same(_timing(y72), [w[1:] for w in _oracle(I.N_DEFAULT)], _rows(I.N_DEFAULT)[0], ("y72", ring, lean))
    rx = E.Receiver()
    b = I.built72_rows()
    _same(_timing(b), [rx.timing(r) for r in b], I.BUILT72, ("built72", ring, lean))


@pytest.mark.parametrize("fs,force", [(1.8e6, False), (2.4e6, True)])
def test_generic_rate_kernel(fs, force):
    """(d): k_chanfilt_g + k_timing, at 1.8 MSps and on the canonical plan with TETRA_ETSI_FORCE_GENERIC."""
    from tetraear import _hip
    from tetraear.signal.etsi import etsi_plan
    plan = etsi_plan(fs, force_generic=force)
    assert _kernel(plan, _hip.TETRA_CF32, I.N_DEFAULT)[0] == "k_chanfilt_g"
    x = np.concatenate([I.ladder_rows(I.N_DEFAULT, fs), I.class_rows(I.N_DEFAULT)])
    _same(_demod(np.ascontiguousarray(x), plan), [w[1:] for w in _oracle(I.N_DEFAULT, fs)], _rows(I.N_DEFAULT)[0],
          ("generic", fs))


@pytest.mark.parametrize("fmt", ["cf32", "sc16"])
def test_stream_chunks(fmt):
    """(e): EtsiStream.demod against E.Stream chunk by chunk -- signal, silence, a weak chunk, a
    two-sample chunk, a loud chunk, noise, signal -- the carried loop state and every output.  (SC16
    cannot hold base x 2^-18 or x 2^12: a few-LSB chunk and a full-scale square wave stand in.)"""
    from tetraear.signal.etsi import EtsiStream
    chunks = I.stream_chunks() if fmt == "cf32" else I.stream_chunks_sc16()
    st, orc = EtsiStream(2.4e6, 1), E.Stream(2.4e6, cell_init=I.CELL)
    for i, ch in enumerate(chunks):
        hard, soft, sym, ns = st.demod(np.ascontiguousarray(ch)[None])
        r = orc.push(ch if fmt == "cf32" else I.sc16_to_cf32(ch))
        n = int(ns[0])
        assert n == len(r["symbols"]), i
        assert np.array_equal(sym[0, :n], r["symbols"]), i
        assert np.array_equal(soft[0, :2 * max(n - 1, 0)], r["soft"]), i
        assert np.array_equal(hard[0, :max(n - 1, 0)], r["hard"]), i
        assert np.array_equal(st.diag[0], r["diag"], equal_nan=True), i
        t, w = st.track[0], r["track"][0]
        assert (t["base"], t["delta"], t["prev_re"], t["prev_im"], t["acquired"]) == \
            (w["base"], w["delta"], w["pr"], w["pi"], w["acquired"]), i


def test_timing_chunks_with_partials():
    """(f): tetra_etsi_timing_chunks with the resampler's group partials, at the smallest geometry of
    test_timing_chunks_geometries_bit_exact: rows that hold silence, a 2^-40 stretch and a nominal
    stretch side by side, so the overlapping chunks straddle them."""
    from tetraear import _hip
    from tetraear.signal.etsi import etsi_plan
    rowlen, nchunk, stride, length, U = 100, 2, 40, 60, 36
    y = E.Receiver().chanfilt(I.base())[200:300]
    z, weak = np.zeros(100, np.complex64), I.scale(y, -40)
    rows = np.ascontiguousarray(np.stack([np.concatenate([z[:40], weak[40:]]), np.concatenate([weak[:40], y[40:]]),
                                          np.concatenate([y[:50], z[50:]])]))
    ngrp = -(-rowlen // U)
    om = np.stack([E.Receiver.om_group_partials(r, U) for r in rows]).astype(np.float32)
    C, sm = 3 * nchunk, length // 4 + 2
    sym, soft = np.zeros((C, sm), np.complex64), np.zeros((C, 2 * sm), np.int8)
    hard, ns, diag = np.zeros((C, sm), np.uint8), np.zeros(C, np.int32), np.zeros((C, 4), np.float32)
    c = _hip.ctx()
    c.check(c.lib.tetra_etsi_timing_chunks(c.handle, etsi_plan(), _hip.ptr(rows), 3, rowlen, nchunk, stride, length,
                                           _hip.ptr(om), ngrp, U, _hip.ptr(sym), _hip.ptr(soft), _hip.ptr(hard),
                                           _hip.ptr(ns), sm, _hip.ptr(diag)), "timing_chunks")
    ora, want, labels = E.Receiver(), [], []
    for r in range(3):
        for ci in range(nchunk):
            s0 = ci * stride
            L = min(length, rowlen - s0)
            want.append(ora.timing(rows[r, s0:s0 + L], om=E.Receiver.om_grouped(rows[r], s0, L, U, om[r])))
            labels.append((r, ci))
    _same((hard, soft, sym, ns, diag), want, labels, "chunks")


def test_lower_mac_on_the_rows(demod_cf32):
    """(g): EtsiLowerMac.decode_batch on the demod's outputs against the oracle's lower MAC: no bursts
    on the silent, tone and all-zero-dibit rows, the planted bursts CRC-good on every rung inside the
    window (the longest rows hold three whole bursts, five blocks)."""
    from tetraear.core.etsi import EtsiLowerMac
    N = 134408
    hard, soft, sym, ns, _ = demod_cf32[1][N]
    labels = _rows(N)[0]
    res = EtsiLowerMac().decode_batch(soft, hard, ns, np.full(len(ns), I.CELL, np.uint32))
    rx, sent = E.Receiver(), I.planted_payloads()
    for r, lab in enumerate(labels):
        n = max(int(ns[r]), 1)
        want = rx.lower_mac(soft[r, :2 * (n - 1)], hard[r, :n - 1], I.CELL)
        got = res[r]
        assert [(f["position"], f["burst_kind"]) for f in got] == [(s, k) for s, k, _ in want], lab
        for f, (_, _, dec) in zip(got, want):
            assert len(f["blocks"]) == len(dec), lab
            for b, (kind, bits, ok) in zip(f["blocks"], dec):
                assert b["crc_ok"] == ok and np.array_equal(b["bits"], bits), lab
        if lab[0] == "k" and I.WINDOW[0] <= lab[1] <= I.WINDOW[1]:
            blocks = [b for f in got for b in f["blocks"]]
            assert len(got) == 3 and len(blocks) == 5 and all(b["crc_ok"] for b in blocks), lab
            assert all(tuple(np.pad(b["bits"], (0, 268 - len(b["bits"])))) in sent for b in blocks), lab
        if lab[0] == "class" and lab[1] not in ("base_silence", "silence_base"):
            assert got == [], lab
        if not hard[r, :n - 1].any():
            assert got == [], lab


def test_scale_metamorphic(demod_cf32):
    """(h): independent of the oracle -- on the GPU's own outputs the rungs inside the window equal
    the k = 0 row, with the symbols scaled exactly."""
    for N, (hard, soft, sym, ns, diag) in demod_cf32[1].items():
        r0 = I.LADDER.index(0)
        n = int(ns[r0])
        assert n > 10
        for k in IN_WINDOW:
            r = I.LADDER.index(k)
            assert int(ns[r]) == n, (N, k)
            assert np.array_equal(hard[r, :n - 1], hard[r0, :n - 1]), (N, k)
            assert np.array_equal(soft[r, :2 * (n - 1)], soft[r0, :2 * (n - 1)]), (N, k)
            assert np.array_equal(diag[r], diag[r0]), (N, k)
            assert np.array_equal(sym[r, :n], I.scale(sym[r0, :n], k)), (N, k)
