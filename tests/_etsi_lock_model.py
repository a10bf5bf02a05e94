"""numpy restatement of the loss-of-lock monitor (tetra_etsi_lock, include/tetra_hip.h) and of the
receiver around it (tetraear.signal.etsi.EtsiStream(lock=True, redo=...)), driven over oracle/etsi.py
Stream the way the receiver drives the library.  TEST INFRASTRUCTURE: the GPU tests hold the kernel and
EtsiStream against it bit for bit, tests/test_etsi_lock_model.py pins the rule, and `python
tests/_etsi_lock_model.py` prints the table of DESIGN.md §5.28 the committed constants were read from.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(os.path.dirname(_HERE), "oracle"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import etsi as E   # noqa: E402

# the committed constants (include/tetra_hip.h TETRA_ETSI_LOCK_*_DEFAULT; tests/test_etsi_lock_model.py
# checks the header says the same)
NUM, DEN, WEAK, NMIN, PATIENCE = 1, 2, 8, 64, 1
LOCK_STATE = np.dtype([("searching", "<i4"), ("bad_run", "<i4"), ("relocks", "<i4"), ("chunks", "<i4"),
                       ("reserved", "<i4", (4,))])
F_JUDGED, F_BAD, F_RAILED, F_FRESH, F_DROPPED, F_SEARCHING = 1, 2, 4, 8, 16, 32
R_SMIN, R_SMAX, R_N, R_WEAK, R_FLAGS, R_BAD_RUN, R_RELOCKS = range(7)


def sums(row, nsym, weak, ostride=None):
    """(SMIN, SMAX, N, WEAK) of one row of soft bits: N = max(nsym - 1, 0) dibits (at most ostride)."""
    n = max(int(nsym) - 1, 0)
    if ostride is not None:
        n = min(n, int(ostride))
    s = np.abs(np.asarray(row[:2 * n], np.int8).astype(np.int64)).reshape(n, 2)
    hi, lo = s.max(axis=1), s.min(axis=1)
    strong = hi >= weak
    return int(lo[strong].sum()), int(hi[strong].sum()), n, int(n - strong.sum())


def judge(smin, smax, n, nweak, delta, state, num=NUM, den=DEN, nmin=NMIN, patience=PATIENCE):
    """The rule on one channel's sums: state (a LOCK_STATE record) is updated in place; returns
    (rec [8] int32, clear): clear = the channel's track.acquired is to be set to 0."""
    if not (state["searching"] or state["bad_run"] or state["relocks"] or state["chunks"]):
        state["searching"] = 1   # an all-zero state reads as searching: the first chunk acquires
    fresh = bool(state["searching"])
    railed = bool(np.abs(np.float32(delta)) >= np.float32(1.5))
    judged = n >= nmin
    bad = judged and (2 * nweak > n or smax == 0 or int(smin) * int(den) < int(num) * int(smax) or railed)
    dropped = clear = False
    state["chunks"] += 1
    if judged and not bad:
        state["searching"], state["bad_run"] = 0, 0
    elif judged and fresh:
        state["searching"] = 1
        clear = True
    elif judged:
        state["bad_run"] += 1
        if state["bad_run"] >= patience:
            dropped = clear = True
            state["searching"], state["bad_run"] = 1, 0
            state["relocks"] += 1
    flags = (F_JUDGED * judged | F_BAD * bool(bad) | F_RAILED * railed | F_FRESH * fresh | F_DROPPED * dropped
             | F_SEARCHING * bool(state["searching"]))
    return np.array([smin, smax, n, nweak, flags, state["bad_run"], state["relocks"], 0], np.int32), clear


def lock(softbits, nsym, ostride, track, state, num=NUM, den=DEN, weak=WEAK, nmin=NMIN, patience=PATIENCE):
    """tetra_etsi_lock over C rows (softbits flat or [C, 2 ostride]; track and state updated in place):
    rec [C, 8]."""
    sb = np.asarray(softbits, np.int8).reshape(-1)
    C = len(nsym)
    rec = np.zeros((C, 8), np.int32)
    for c in range(C):
        row = sb[2 * ostride * c:2 * ostride * (c + 1)]
        r, clear = judge(*sums(row, nsym[c], weak, ostride), track["delta"][c], state[c:c + 1][0], num, den, nmin,
                         patience)
        rec[c] = r
        if clear:
            track["acquired"][c] = 0
    return rec


def balance(soft, weak=0):
    """SMIN / SMAX of a chunk's soft bits (weak = 0: over every dibit) -- the lock metric as a ratio."""
    smin, smax, _, _ = sums(soft, len(soft) // 2 + 1, weak)
    return smin / smax if smax else 0.0


class LockedStream:
    """One channel of EtsiStream(lock=..., redo=...) on the oracle: oracle Stream's window arithmetic,
    channel filter and carried timing loop (its lower MAC is not run), the monitor after every chunk,
    and with redo the timing repeated from the track as it stood before the call with acquired = 0
    when the chunk dropped the channel."""

    def __init__(self, fs=E.FS_NOMINAL, lock=True, redo=False, consts=None):
        self.st = E.Stream(fs)
        self.on, self.redo = lock, redo
        self.k = dict(num=NUM, den=DEN, weak=WEAK, nmin=NMIN, patience=PATIENCE)
        self.k.update(consts or {})
        self.state = np.zeros(1, LOCK_STATE)

    def _timing(self, y, yoff):
        sym, soft, hard, diag = self.st.rx.timing_stream(y, yoff, self.st.trk[0:1])
        return dict(symbols=sym, soft=soft, hard=hard, diag=diag)

    def push(self, x):
        st = self.st
        x = np.asarray(x, np.complex64)
        s, W, yoff, y_start = st.window(len(x))
        st.buf = np.concatenate([st.buf, x])
        st.x_total += len(x)
        y = st.rx.chanfilt(st.buf[s:st.x_total])
        _, m_hi = E.stream_lengths(st.rx.d, st.x_total)
        trk0, state0 = st.trk.copy(), self.state.copy()
        out = self._timing(y, yoff)
        out["fresh"] = not trk0["acquired"][0]
        out["dropped"] = False
        if self.on:
            ns = np.array([len(out["symbols"])], np.int32)
            rec = lock(out["soft"], ns, max(len(out["soft"]) // 2, 1), st.trk, self.state, **self.k)
            out["dropped"] = bool(rec[0, R_FLAGS] & F_DROPPED)
            if out["dropped"] and self.redo:
                st.trk[:] = trk0
                st.trk["acquired"] = 0
                self.state["chunks"] = state0["chunks"]
                out.update(self._timing(y, yoff))
                out["fresh"] = True
                ns = np.array([len(out["symbols"])], np.int32)
                rec = lock(out["soft"], ns, max(len(out["soft"]) // 2, 1), st.trk, self.state, **self.k)
            out["rec"] = rec[0]
        st.y_done = max(m_hi, st.y_done)
        out["track"], out["state"] = st.trk.copy(), self.state.copy()
        return out


# ------------------------------------------------------------------------------ signals

def capture(rng, n, fs=E.FS_NOMINAL, snr_db=None, t0=0.3, cfo=120.0, cell=None, amp=0.5):
    """n samples of a continuous downlink (burst_stream + modulate) of a random cell."""
    scr = E.scramble_seq(E.scramble_init(*(cell or (int(rng.integers(200, 800)), int(rng.integers(0, 1000)),
                                                    int(rng.integers(0, 64))))), 432)
    nb = int(n * E.SYMBOL_RATE / fs / 255) + 3
    bits, _ = E.burst_stream(rng, nb, scr)
    return E.modulate(bits, n, fs=fs, t0=t0, phase0=float(rng.uniform(0, 6.28)), cfo=cfo, snr_db=snr_db, rng=rng,
                      amp=amp)


def noise(rng, n, sigma=0.35):
    return (sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def slipped(x, at, drop):
    """The capture with `drop` samples missing at sample `at` (an SDR sample drop at a chunk seam)."""
    return np.concatenate([x[:at], x[at + drop:]])


# ------------------------------------------------------------------------------ the GPU tests' stream

def three_channels(seed=11, chunk=32768, nchunk=6, fs=E.FS_NOMINAL):
    """[3, nchunk * chunk] complex64 at 12 dB Es/N0: channel 0 one continuous downlink; channel 1 the
    same kind with 66 samples missing before chunk 3; channel 2 a downlink for two chunks, one chunk of
    noise, then another cell's downlink at another symbol time and carrier offset."""
    rng = np.random.default_rng(seed)
    n = nchunk * chunk
    a = capture(rng, n, fs, 12.0, t0=0.21, cfo=140.0)
    b = slipped(capture(rng, n + 66, fs, 12.0, t0=0.67, cfo=-90.0), 3 * chunk, 66)
    c = np.concatenate([capture(rng, 2 * chunk, fs, 12.0, t0=0.4, cfo=60.0), noise(rng, chunk, 0.02),
                        capture(rng, n - 3 * chunk, fs, 12.0, t0=0.93, cfo=-250.0)])
    return np.stack([a, b, c]).astype(np.complex64)


def run_model(iq, chunk, fs=E.FS_NOMINAL, **kw):
    """Per chunk per channel the LockedStream outputs of iq [C, n] cut into chunks of `chunk` samples."""
    ls = [LockedStream(fs, **kw) for _ in range(iq.shape[0])]
    return [[ls[c].push(iq[c, at:at + chunk]) for c in range(iq.shape[0])]
            for at in range(0, iq.shape[1] - chunk + 1, chunk)]


# ------------------------------------------------------------------------------ the measurement of §5.28

def _crc_good(fs, chunks, lockargs):
    """CRC-good blocks of a capture decoded through the oracle lower MAC, the monitor's fresh rows
    starting a new chain (the carried tail dropped, the cell kept)."""
    ls = LockedStream(fs, **lockargs)
    lm = E.LmacStream(ls.st.rx, None)
    good = 0
    for k, x in enumerate(chunks):
        o = ls.push(x)
        if o["fresh"] and k:
            lm.tail_hard, lm.tail_soft, lm.phase = np.zeros(0, np.uint8), np.zeros(0, np.int8), 0
        good += sum(ok for _, _, dec in lm.push(o["hard"], o["soft"])["bursts"] for _, _, ok in dec)
    return good


def measure(fs, nchunk, chunk, seed, out=print):
    """The table of DESIGN.md §5.28 for one rate: nchunk chunks of `chunk` samples per condition."""
    rng = np.random.default_rng(seed)
    n = nchunk * chunk
    res = {}

    def run(x, **kw):
        ls = LockedStream(fs, **kw)
        return [ls.push(x[i:i + chunk]) for i in range(0, len(x) - chunk + 1, chunk)]

    SEG = 20   # chunks per capture: a condition is nchunk / SEG independent captures
    for name, snr in (("clean", None), ("15 dB", 15.0), ("10 dB", 10.0), ("8 dB", 8.0), ("6 dB", 6.0)):
        bal, weak, bad, tot, crc = [], [], 0, 0, [0, 0, 0]
        for _ in range(-(-nchunk // SEG)):
            x = capture(rng, SEG * chunk, fs, snr, t0=float(rng.uniform(0, 1)), cfo=float(rng.uniform(-600, 600)))
            o = run(x, lock=True, redo=False, consts=dict(patience=1 << 30))
            bal += [balance(v["soft"], WEAK) for v in o]
            weak += [v["rec"][R_WEAK] / max(v["rec"][R_N], 1) for v in o]
            bad += sum(bool(v["rec"][R_FLAGS] & F_BAD) for v in o)
            tot += len(o)
            if snr is not None and snr <= 8.0:
                cks = [x[i:i + chunk] for i in range(0, len(x) - chunk + 1, chunk)]
                crc[0] += _crc_good(fs, cks, dict(lock=False))
                crc[1] += _crc_good(fs, cks, dict(lock=True, redo=True, consts=dict(patience=1)))
                crc[2] += _crc_good(fs, cks, dict(lock=True, redo=True, consts=dict(patience=2)))
        res[name] = dict(min=min(bal), max=max(bal), bad=bad, n=tot, weak=max(weak), crc=crc)
        out(f"{fs / 1e6:.3f} MSps locked {name:6s}: balance {min(bal):.3f}..{max(bal):.3f} weak share <= "
            f"{max(weak):.3f} bad {bad}/{tot}")
        if snr is not None and snr <= 8.0:
            out(f"    CRC-good blocks: monitor off {crc[0]}, patience 1 {crc[1]}, patience 2 {crc[2]}")
    # noise only, every chunk demodulated fresh
    bal, bad = [], 0
    for i in range(nchunk):
        ls = LockedStream(fs, lock=True)
        v = ls.push(noise(rng, chunk))
        bal.append(balance(v["soft"], WEAK))
        bad += bool(v["rec"][R_FLAGS] & F_BAD)
    res["noise fresh"] = dict(min=min(bal), max=max(bal), bad=bad, n=nchunk)
    out(f"{fs / 1e6:.3f} MSps noise fresh  : balance {min(bal):.3f}..{max(bal):.3f} bad {bad}/{nchunk}")
    # noise after signal on a carried stream (the monitor never clears acquired: patience huge)
    bad = tot = 0
    wk = []
    for i in range(nchunk // 4):
        x = np.concatenate([capture(rng, 2 * chunk, fs, 15.0), noise(rng, 2 * chunk, (0.02, 0.2, 2.0)[i % 3])])
        o = run(x, lock=True, consts=dict(patience=1 << 30))
        for v in o[2:]:
            tot += 1
            bad += bool(v["rec"][R_FLAGS] & F_BAD)
            wk.append(v["rec"][R_WEAK] / max(v["rec"][R_N], 1))
    res["noise after signal"] = dict(bad=bad, n=tot, weak=min(wk))
    out(f"{fs / 1e6:.3f} MSps noise after signal: weak share >= {min(wk):.3f} bad {bad}/{tot}")
    # slips: the chunk of the slip and the chunks after it, carried against monitor + redo
    for drop in (34, 66, 100, 400):
        late = by = 0
        runs = max(nchunk // 6, 4)
        pinned = 0
        after_c, after_m = [], []
        for i in range(runs):
            x = slipped(capture(rng, 6 * chunk + drop, fs, 12.0), 2 * chunk, drop)
            oc = run(x, lock=False)
            om = run(x, lock=True, redo=True)
            d = [k for k, v in enumerate(om) if v["dropped"]]
            by += bool(d) and d[0] <= 3
            late += not (bool(d) and d[0] <= 3)
            pinned += abs(float(oc[5]["track"]["delta"][0])) >= 1.5
            after_c += [balance(v["soft"], WEAK) for v in oc[3:]]
            after_m += [balance(v["soft"], WEAK) for v in om[(d[0] if d else 3):][1:]]
        res[f"slip {drop}"] = dict(dropped_by_next=by, runs=runs, pinned=pinned, carried=min(after_c),
                                   monitor=min(after_m) if after_m else None)
        out(f"{fs / 1e6:.3f} MSps slip {drop:3d} at 12 dB: dropped by the chunk after it {by}/{runs}; carried loop pinned "
            f"{pinned}/{runs}, balance after >= {min(after_c):.3f}; with monitor + redo >= "
            f"{min(after_m) if after_m else float('nan'):.3f}")
    return res


if __name__ == "__main__":
    nch = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    measure(2.4e6, nch, 131072, seed=2801)
    measure(2.0e6, nch, 109226, seed=2802)
