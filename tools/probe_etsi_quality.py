#!/usr/bin/env python3
"""Stage times of the streaming ETSI step with tetra_etsi_mac and tetra_etsi_link_quality behind the
lower MAC (tetra_profile's HIP events, one context, the stages one after another): etsi_quality
against etsi_viterbi, etsi_traceback and etsi_mac of the same run.
usage: probe_etsi_quality.py [channels] [steps]  """
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tetraear-bladerf_amd"), REPO]


def read_profile(c):
    names = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 64)()
    n = ctypes.c_int(0)
    c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    raw = names.raw.split(b"\0")
    return {raw[i].decode(): (ms[i], int(cnt[i])) for i in range(n.value)}


def main():
    import torch
    from tetraear import _hip
    from tetraear.signal.etsi import BenchStep
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    N = 131072
    dev = torch.device("cuda", 0)
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    st = BenchStep(c, C, N, 2.4e6, 1, dev, cells="acquire", chunks=steps + 2)
    tdma = torch.zeros((C, 3), dtype=torch.int64, device=dev)
    slots = torch.zeros((C, _hip.ETSI_MAXB, _hip.SLOT_FIELDS), dtype=torch.int32, device=dev)
    npdu = torch.zeros((C, _hip.ETSI_MAXJ), dtype=torch.int32, device=dev)
    pdus = torch.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.PDU_FIELDS), dtype=torch.int32, device=dev)
    bq = torch.full((C, _hip.ETSI_MAXB, _hip.LQ_FIELDS), -9, dtype=torch.int32, device=dev)
    kq = torch.full((C, _hip.ETSI_MAXJ, _hip.LQ_FIELDS), -9, dtype=torch.int32, device=dev)

    def step():
        bq.fill_(-9)   # what a step does not write must still read -9 after it
        kq.fill_(-9)
        st()
        _, soft, hard, nsym = st.bufs[(st.kchunk - 1) & 1]   # the rows the lower MAC read: the tails went to the others
        outs = [_hip.ptr(t) for t in (st.nburst, st.bursts, st.nblock, st.blocks, st.type1)]
        c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(nsym), C, *outs, _hip.ptr(tdma), _hip.ptr(slots), _hip.ptr(npdu),
                                     _hip.ptr(pdus)), "etsi_mac")
        c.check(c.lib.tetra_etsi_link_quality(c.handle, _hip.ptr(soft), _hip.ptr(hard), C, st.stride,
                                              2 * _hip.ETSI_RESERVE, 1, _hip.ptr(st.cell_state), *outs, _hip.ptr(bq),
                                              _hip.ptr(kq)), "etsi_link_quality")

    for _ in range(2):
        step()
    torch.cuda.synchronize(dev)
    c.check(c.lib.tetra_profile(c.handle, 1), "profile")
    read_profile(c)
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    prof = read_profile(c)
    c.check(c.lib.tetra_profile(c.handle, 0), "profile")
    print("tetra_profile, C = %d channels x %d samples per step, streaming lower MAC with cell acquisition, "
          "%d timed steps" % (C, N, steps))
    for name in ("etsi_demod", "etsi_sync", "etsi_acquire", "etsi_viterbi", "etsi_traceback", "etsi_mac", "etsi_quality"):
        if name in prof:
            print("  %-18s %6.3f ms per step  (%d launches)" % (name, prof[name][0] / steps, prof[name][1]))
    live_b = torch.arange(_hip.ETSI_MAXB, device=dev)[None, :] < st.nburst[:, None]
    live_k = torch.arange(_hip.ETSI_MAXJ, device=dev)[None, :] < st.nblock[:, None]
    good = live_k & (st.blocks[:, :, 1] != 0)
    assert bool((kq[live_k & ~good] == torch.tensor([-1, 0, 0, 0], device=dev, dtype=torch.int32)).all())
    assert bool((kq[good] >= 0).all()) and bool((bq[live_b] >= 0).all())
    assert bool((kq[~live_k] == -9).all()) and bool((bq[~live_b] == -9).all())
    g = kq[good].to(torch.int64)
    nerr, nbits = int(g[:, _hip.LQ_NERR].sum()), int((g[:, _hip.LQ_WSUM] > -1).sum())
    K = torch.tensor([432, 216, 120], device=dev)[st.blocks[:, :, 0][good].long()]
    scored = int((K - g[:, _hip.LQ_NZERO]).sum())
    b = bq[live_b].to(torch.int64)
    print("last step: bursts %d, blocks %d (CRC-good %d), channel errors %d in %d scored bits (BER %.2e), "
          "blocks with errors %d" % (int(live_b.sum()), int(live_k.sum()), nbits, nerr, scored, nerr / max(scored, 1),
                                     int((g[:, _hip.LQ_NERR] > 0).sum())))
    print("last step: training errors %d, head/tail errors %d, saturated soft bits %d of %d"
          % (int(b[:, _hip.BQ_TERR].sum()), int(b[:, _hip.BQ_HERR].sum()), int(b[:, _hip.BQ_NSAT].sum()), 510 * len(b)))


if __name__ == "__main__":
    main()
