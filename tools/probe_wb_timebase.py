#!/usr/bin/env python3
"""Stage times of the wideband step with TETRA_WB_MAC=timebase (tetra_profile's HIP events, one
context, the stages one after another): etsi_mac_groups against etsi_mac on the same rows and against
the lower MAC's stages.  usage: probe_wb_timebase.py [wideband samples] [steps]  """
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tetraear-bladerf_amd"), REPO]
os.environ["TETRA_WB_MAC"] = "timebase"


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
    from tetraear.signal.wideband import BenchStep
    Nw = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dev = torch.device("cuda", 0)
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    st = BenchStep(c, Nw, seed=1, device=dev)
    # tetra_etsi_mac on the same rows: one timebase per row, its outputs thrown away
    tdma = torch.zeros((st.C, 3), dtype=torch.int64, device=dev)
    slots, npdu, pdus = torch.zeros_like(st.slots), torch.zeros_like(st.npdu), torch.zeros_like(st.pdus)

    def rows_mac():
        tdma.zero_()
        c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(st.nsym), st.C, _hip.ptr(st.nburst), _hip.ptr(st.bursts),
                                     _hip.ptr(st.nblock), _hip.ptr(st.blocks), _hip.ptr(st.type1), _hip.ptr(tdma),
                                     _hip.ptr(slots), _hip.ptr(npdu), _hip.ptr(pdus)), "etsi_mac")

    for _ in range(3):
        st()
        rows_mac()
    torch.cuda.synchronize(dev)
    c.check(c.lib.tetra_profile(c.handle, 1), "profile")
    read_profile(c)
    for _ in range(steps):
        st()
        rows_mac()
    torch.cuda.synchronize(dev)
    prof = read_profile(c)
    c.check(c.lib.tetra_profile(c.handle, 0), "profile")
    assert torch.equal(npdu, st.npdu) and torch.equal(pdus, st.pdus)   # the same PDU walk
    print(json.dumps({"wideband_samples": Nw, "rows": st.C, "rows_per_group": st.nchunk, "steps": steps,
                      "stage_ms_per_step": {k: round(ms / steps, 4) for k, (ms, n) in sorted(prof.items())},
                      "launches_per_step": {k: n / steps for k, (ms, n) in sorted(prof.items())},
                      "quality": st.quality()}))


if __name__ == "__main__":
    main()
