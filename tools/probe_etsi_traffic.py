#!/usr/bin/env python3
"""Stage times of the streaming ETSI step with tetra_etsi_mac, tetra_etsi_link_quality and
tetra_etsi_traffic behind the lower MAC (tetra_profile's HIP events, one context, the stages one after
another): etsi_traffic against etsi_quality of the same run.  The synthesised captures hold no traffic,
so the step runs twice: as they are (every burst CONTROL or NONE: the cost of classifying), and with the
lower MAC given a wrong cell for every channel, so that every normal burst is FULL or LOST (the most
that can be exported).
usage: probe_etsi_traffic.py [channels] [steps]  """
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tetraear-bladerf_amd"), REPO]

STAGES = ("etsi_demod", "etsi_sync", "etsi_acquire", "etsi_viterbi", "etsi_traceback", "etsi_mac", "etsi_quality",
          "etsi_traffic")


def read_profile(c):
    names = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 64)()
    n = ctypes.c_int(0)
    c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    raw = names.raw.split(b"\0")
    return {raw[i].decode(): (ms[i], int(cnt[i])) for i in range(n.value)}


def run(C, steps, wrong_cell):
    import torch
    from tetraear import _hip
    from tetraear.signal.etsi import BenchStep
    N = 131072
    dev = torch.device("cuda", 0)
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    st = BenchStep(c, C, N, 2.4e6, 1, dev, cells="given" if wrong_cell else "acquire", chunks=steps + 2)
    if wrong_cell:   # the context's cell table with another colour code in every channel
        used = st.cells ^ (0x15 << 2)
        c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(used), C), "set_cells")
        c.synchronize()
    else:
        used = st.cell_state
    tdma = torch.zeros((C, 3), dtype=torch.int64, device=dev)
    slots = torch.zeros((C, _hip.ETSI_MAXB, _hip.SLOT_FIELDS), dtype=torch.int32, device=dev)
    npdu = torch.zeros((C, _hip.ETSI_MAXJ), dtype=torch.int32, device=dev)
    pdus = torch.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.PDU_FIELDS), dtype=torch.int32, device=dev)
    bq = torch.full((C, _hip.ETSI_MAXB, _hip.LQ_FIELDS), -9, dtype=torch.int32, device=dev)
    kq = torch.full((C, _hip.ETSI_MAXJ, _hip.LQ_FIELDS), -9, dtype=torch.int32, device=dev)
    tq = torch.full((C, _hip.ETSI_MAXB, _hip.TQ_FIELDS), -9, dtype=torch.int32, device=dev)
    tch = torch.full((C, _hip.ETSI_MAXB, _hip.TCH_BITS), 0x5A, dtype=torch.int8, device=dev)

    def step():
        tq.fill_(-9)   # what a step does not write must still read -9 / 0x5A after it
        tch.fill_(0x5A)
        st()
        _, soft, hard, nsym = st.bufs[(st.kchunk - 1) & 1]   # the rows the lower MAC read: the tails went to the others
        outs = [_hip.ptr(t) for t in (st.nburst, st.bursts, st.nblock, st.blocks, st.type1)]
        c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(nsym), C, *outs, _hip.ptr(tdma), _hip.ptr(slots), _hip.ptr(npdu),
                                     _hip.ptr(pdus)), "etsi_mac")
        c.check(c.lib.tetra_etsi_link_quality(c.handle, _hip.ptr(soft), _hip.ptr(hard), C, st.stride,
                                              2 * _hip.ETSI_RESERVE, 1, _hip.ptr(used), *outs, _hip.ptr(bq),
                                              _hip.ptr(kq)), "etsi_link_quality")
        c.check(c.lib.tetra_etsi_traffic(c.handle, _hip.ptr(soft), C, st.stride, 2 * _hip.ETSI_RESERVE, 1,
                                         _hip.ptr(used), *outs[:4], _hip.ptr(slots), None, _hip.ptr(tq), _hip.ptr(tch)),
                "etsi_traffic")

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
    print("tetra_profile, C = %d channels x %d samples per step, streaming lower MAC %s, %d timed steps"
          % (C, N, "with a wrong cell in every channel" if wrong_cell else "with cell acquisition", steps))
    for name in STAGES:
        if name in prof:
            print("  %-18s %6.3f ms per step  (%d launches)" % (name, prof[name][0] / steps, prof[name][1]))
    live = torch.arange(_hip.ETSI_MAXB, device=dev)[None, :] < st.nburst[:, None]
    assert bool((tq[~live] == -9).all()) and bool((tq[live][:, 0] >= 0).all())
    cls = tq[live][:, _hip.TQ_CLASS]
    count = [int((cls == k).sum()) for k in range(5)]
    nbits = int(tq[live][:, _hip.TQ_NBITS].sum())
    print("last step: bursts %d -- NONE %d, CONTROL %d, FULL %d, HALF %d, LOST %d; %d soft bits exported"
          % (int(live.sum()), *count, nbits))
    exported = ((tq[:, :, _hip.TQ_CLASS] == _hip.TCH_FULL) | (tq[:, :, _hip.TQ_CLASS] == _hip.TCH_HALF)) & live
    assert bool((tch[~exported] == 0x5A).all())
    del st
    torch.cuda.empty_cache()


def main():
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    for wrong_cell in (False, True):
        run(C, steps, wrong_cell)


if __name__ == "__main__":
    main()
