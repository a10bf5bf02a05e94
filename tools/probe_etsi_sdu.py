#!/usr/bin/env python3
"""Stage times of the streaming ETSI step with tetra_etsi_mac and tetra_etsi_sdu behind the lower MAC
(tetra_profile's HIP events, one context, the stages one after another): etsi_sdu against etsi_mac and
etsi_traceback of the same run.  The step runs twice: on the synthesised captures as they are (random
payloads: few fragments, the cost of looking), and with fragment chains planted.  tetra_synth_etsi takes
no payloads, so the chains are planted in the records the lower MAC left, on the device: every CRC-good
SCH/F block becomes a MAC-RESOURCE with L = 63, a MAC-FRAG or a MAC-END by its burst's place on the
stream's slot grid (chains of six fragments, four slots apart, on all four timeslots), and tetra_etsi_mac
and tetra_etsi_sdu run on those built records.
usage: probe_etsi_sdu.py [channels] [steps]  """
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tetraear-bladerf_amd"), REPO]

STAGES = ("etsi_demod", "etsi_sync", "etsi_acquire", "etsi_viterbi", "etsi_traceback", "etsi_mac", "etsi_sdu")
CHAIN = 6   # fragments per planted chain
MAXD = 4


def read_profile(c):
    names = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 64)()
    n = ctypes.c_int(0)
    c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    raw = names.raw.split(b"\0")
    return {raw[i].decode(): (ms[i], int(cnt[i])) for i in range(n.value)}


def templates(torch, dev):
    """[3, 268] type-1 bytes: a MAC-RESOURCE (L = 63, SSI), a MAC-FRAG, a MAC-END (L = 63), full blocks."""
    g = torch.Generator().manual_seed(7)

    def bits(head):
        return torch.cat([torch.tensor(head, dtype=torch.uint8), torch.randint(0, 2, (268 - len(head),), generator=g,
                                                                               dtype=torch.uint8)])
    first = [0, 0, 0, 0, 0, 0, 0] + [1] * 6 + [0, 0, 1] + [1, 0] * 12 + [0, 0, 0]
    last = [0, 1, 1, 0, 0] + [1] * 6 + [0, 0]
    return torch.stack([bits(first), bits([0, 1, 0, 0]), bits(last)]).to(dev)


def run(C, steps, plant):
    import torch
    from tetraear import _hip
    from tetraear.signal.etsi import BenchStep
    N = 131072
    dev = torch.device("cuda", 0)
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    st = BenchStep(c, C, N, 2.4e6, 1, dev, cells="acquire", chunks=steps + 2)
    tdma = torch.zeros((C, 3), dtype=torch.int64, device=dev)
    slots = torch.zeros((C, _hip.ETSI_MAXB, _hip.SLOT_FIELDS), dtype=torch.int32, device=dev)
    npdu = torch.zeros((C, _hip.ETSI_MAXJ), dtype=torch.int32, device=dev)
    pdus = torch.zeros((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.PDU_FIELDS), dtype=torch.int32, device=dev)
    sdu = torch.full((C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.SDU_FIELDS), -9, dtype=torch.int32, device=dev)
    sdu_data = torch.zeros((C, _hip.ETSI_MAXJ, _hip.SDU_ROW), dtype=torch.uint8, device=dev)
    frag = torch.zeros((C, _hip.ETSI_FRAG.itemsize), dtype=torch.uint8, device=dev)
    ndone = torch.zeros(C, dtype=torch.int32, device=dev)
    done = torch.zeros((C, MAXD, _hip.DONE_FIELDS), dtype=torch.int32, device=dev)
    done_data = torch.zeros((C, MAXD, _hip.SDU_MAXBYTES), dtype=torch.uint8, device=dev)
    tmpl = templates(torch, dev)
    total = {"done": 0}

    def plant_chains():
        """Every CRC-good SCH/F block gets the fragment its burst's slot calls for."""
        bit0 = frag[:, :8].contiguous().view(torch.int64)[:, 0]
        j = torch.arange(_hip.ETSI_MAXJ, device=dev)[None, :]
        good = (j < st.nblock[:, None]) & (st.blocks[:, :, 0] == 0) & (st.blocks[:, :, 1] != 0)
        b = st.blocks[:, :, 2].clamp(0, _hip.ETSI_MAXB - 1).long()
        start = torch.gather(st.bursts[:, :, 0].long(), 1, b)
        slot = torch.div(bit0[:, None] + start + 255, 510, rounding_mode="floor")
        place = torch.div(slot, 4, rounding_mode="floor") % CHAIN
        which = (place != 0).long() + (place == CHAIN - 1).long()   # 0 first, 1 middle, 2 last
        st.type1[good] = tmpl[which[good]]

    def step():
        st()
        nsym = st.bufs[(st.kchunk - 1) & 1][3]
        if plant:
            plant_chains()
        outs = [_hip.ptr(t) for t in (st.nburst, st.bursts, st.nblock, st.blocks, st.type1)]
        c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(nsym), C, *outs, _hip.ptr(tdma), _hip.ptr(slots), _hip.ptr(npdu),
                                     _hip.ptr(pdus)), "etsi_mac")
        c.check(c.lib.tetra_etsi_sdu(c.handle, _hip.ptr(nsym), C, 1, 0, 0, _hip.TDMA_EXPIRE, *outs, _hip.ptr(npdu),
                                     _hip.ptr(pdus), None, _hip.ptr(sdu), _hip.ptr(sdu_data), _hip.ptr(frag), MAXD,
                                     _hip.ptr(ndone), _hip.ptr(done), _hip.ptr(done_data)), "etsi_sdu")
        total["done"] += int(ndone.sum())

    for _ in range(2):
        step()
    torch.cuda.synchronize(dev)
    c.check(c.lib.tetra_profile(c.handle, 1), "profile")
    read_profile(c)
    total["done"] = 0
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    prof = read_profile(c)
    c.check(c.lib.tetra_profile(c.handle, 0), "profile")
    print("tetra_profile, C = %d channels x %d samples per step, streaming lower MAC with cell acquisition, %s, %d timed "
          "steps" % (C, N, "fragment chains planted in the records" if plant else "the synthesised payloads", steps))
    for name in STAGES:
        if name in prof:
            print("  %-18s %6.3f ms per step  (%d launches)" % (name, prof[name][0] / steps, prof[name][1]))
    import numpy as np
    fr = frag.cpu().numpy().view(_hip.ETSI_FRAG).reshape(C)
    j = torch.arange(_hip.ETSI_MAXJ, device=dev)[None, :]
    live = (j < st.nblock[:, None]) & (npdu > 0)
    roles = sdu[live][:, :, _hip.SDU_ROLE]
    rec = torch.arange(_hip.ETSI_MAXPDU, device=dev)[None, :] < npdu[live].clamp(max=_hip.ETSI_MAXPDU)[:, None]
    print("last step: blocks with PDUs %d, records %d, with ROLE != 0 %d; completed in the timed steps %d; since the "
          "start: dropped %d, orphans %d; chains active now %d"
          % (int(live.sum()), int(rec.sum()), int(((roles != 0) & rec).sum()), total["done"], int(fr["dropped"].sum()),
             int(fr["orphans"].sum()), int(np.count_nonzero(fr["chain"]["active"]))))
    del st
    torch.cuda.empty_cache()


def main():
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    for plant in (False, True):
        run(C, steps, plant)


if __name__ == "__main__":
    main()
