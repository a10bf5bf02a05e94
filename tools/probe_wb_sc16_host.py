#!/usr/bin/env python3
"""Host-resident wideband path, SC16 against complex64: one 10 M-sample piece (0.5 s
at 20 MSps) from host memory through WidebandStream.decode -- as int16 as captured, and as complex64
including the conversion a caller needed before the channeliser took SC16 -- then the channeliser
alone, with every output row copied back and with 16 outputs per carrier (the input copy and the
analysis left).  Wall clock per call, the first call of each form dropped.
usage: python tools/probe_wb_sc16_host.py"""
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # the repository
sys.path[:0] = [os.path.join(R, "tetraear-bladerf_amd"), os.path.join(R, "tests")]
import numpy as np  # noqa: E402
from tetraear.signal import wideband as WB  # noqa: E402
from _wb_sc16 import q16  # noqa: E402

REPS = 9


def as_cf32(q):   # signal/etsi.py's _sc16_to_cf32
    return (q[:, 0].astype(np.float32) + 1j * q[:, 1].astype(np.float32)).astype(np.complex64) / np.float32(32768)


def as_cf32_fast(q):   # one float32 pass
    return (q.astype(np.float32) * np.float32(1 / 32768)).view(np.complex64)[:, 0]


def report(name, ts, extra=""):
    print(f"{name}: median {statistics.median(ts[1:]):.4f} s, min {min(ts[1:]):.4f} "
          f"(runs {[round(t, 4) for t in ts]}) {extra}", flush=True)


def main():
    x, cells = WB.synth_wideband(10_000_000, seed=3, snr_db=30.0)[:2]
    q = q16(x)
    del x
    for name, conv in (("WidebandStream.decode, int16 as captured", lambda q: q),
                       ("WidebandStream.decode, complex64 incl. astype (etsi._sc16_to_cf32 form)", as_cf32),
                       ("WidebandStream.decode, complex64 incl. one float32 pass", as_cf32_fast)):
        ts, tc, nf = [], [], 0
        for rep in range(REPS):
            st = WB.WidebandStream(cells)
            t0 = time.perf_counter()
            p = conv(q)
            t1 = time.perf_counter()
            fr = st.decode(p)
            t2 = time.perf_counter()
            ts.append(t2 - t0)
            tc.append(t1 - t0)
            nf = sum(len(f) for f in fr)
            del p, fr
        report(name, ts, f"conversion median {statistics.median(tc[1:]):.4f} s, frames {nf}")
    rx = WB.WidebandReceiver()
    c64 = as_cf32_fast(q).copy()
    for keep in (None, 16):
        for name, p in (("int16", q), ("complex64", c64)):
            ts = []
            for rep in range(REPS):
                t0 = time.perf_counter()
                rx.channelize(p, keep)
                ts.append(time.perf_counter() - t0)
            report(f"channelize from the host, n_keep={keep}, {name}", ts)


if __name__ == "__main__":
    main()
