#!/usr/bin/env python3
"""Stage times of the streaming ETSI step with tetra_etsi_mac, tetra_etsi_sdu and tetra_etsi_assign behind
the lower MAC (tetra_profile's HIP events, one context, the stages one after another): etsi_assign against
etsi_sdu of the same run, which walks the same records with the same early exit.  The step runs twice: on
the synthesised captures as they are (random payloads: the few channel allocations random bits happen to
spell, the cost of looking), and with allocations planted.  tetra_synth_etsi takes no payloads, so they are
planted in the records the lower MAC left, on the device: on one channel in PLANT_EVERY, every CRC-good SCH/F
block of a burst whose slot count is a multiple of 16 becomes a MAC-RESOURCE whose channel allocation names
the channel's own carrier and timeslots 2 and 3, and tetra_etsi_mac, tetra_etsi_sdu and tetra_etsi_assign run
on those built records.  Every channel has a key of its own (band 4 upwards, carrier number c mod 4000).
usage: probe_etsi_assign.py [channels] [steps]  """
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tetraear-bladerf_amd"), REPO]

STAGES = ("etsi_demod", "etsi_sync", "etsi_acquire", "etsi_viterbi", "etsi_traceback", "etsi_mac", "etsi_sdu", "etsi_assign")
PLANT_EVERY = 8   # one channel in eight announces
MAXD, MAXE = 4, 8
CARRIER_AT = 40 + 3 + 10   # the carrier number's first bit: header and SSI, three flags, the ten head bits


def read_profile(c):
    names = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 64)()
    n = ctypes.c_int(0)
    c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    raw = names.raw.split(b"\0")
    return {raw[i].decode(): (ms[i], int(cnt[i])) for i in range(n.value)}


def templates(torch, dev, C):
    """[C, 268] type-1 bytes: a MAC-RESOURCE of nine octets (SSI, no power control, no slot granting, a channel
    allocation of timeslots 2 and 3, downlink, carrier number c mod 4000, not extended, monitoring pattern 3, a
    TM-SDU of four bits), then a null PDU."""
    g = torch.Generator().manual_seed(7)
    head = [0, 0, 0, 0, 0, 0, 0] + [0, 0, 1, 0, 0, 1] + [0, 0, 1] + [1, 0] * 12          # L = 9, address type 1, the SSI
    head += [0, 0, 1] + [0, 0] + [0, 1, 1, 0] + [0, 1] + [0, 0] + [0] * 12 + [0] + [1, 1] + [1, 0, 1, 1]
    head += [0] * 7 + [0, 0, 0, 0, 1, 0] + [0, 0, 0]                                     # the null PDU
    row = torch.cat([torch.tensor(head, dtype=torch.uint8), torch.randint(0, 2, (268 - len(head),), generator=g,
                                                                           dtype=torch.uint8)])
    t = row[None, :].repeat(C, 1)
    n = torch.arange(C) % 4000
    for i in range(12):
        t[:, CARRIER_AT + i] = ((n >> (11 - i)) & 1).to(torch.uint8)
    return t.to(dev)


def run(C, steps, plant):
    import numpy as np
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
    ch = torch.arange(C, device=dev)
    keys = (64000 + (ch // 4000) * 16000 + 4 * (ch % 4000)).to(torch.int32)
    state = torch.zeros((C, _hip.ETSI_ASSIGN.itemsize), dtype=torch.uint8, device=dev)
    nev = torch.zeros(C, dtype=torch.int32, device=dev)
    ev = torch.full((C, MAXE, _hip.AE_FIELDS), -9, dtype=torch.int32, device=dev)
    ta = torch.full((C, _hip.ETSI_MAXB, _hip.TA_FIELDS), -9, dtype=torch.int32, device=dev)
    tmpl = templates(torch, dev, C) if plant else None
    total = {"events": 0}

    def plant_allocations():
        bit0 = state[:, :8].contiguous().view(torch.int64)[:, 0]
        j = torch.arange(_hip.ETSI_MAXJ, device=dev)[None, :]
        good = (j < st.nblock[:, None]) & (st.blocks[:, :, 0] == 0) & (st.blocks[:, :, 1] != 0)
        b = st.blocks[:, :, 2].clamp(0, _hip.ETSI_MAXB - 1).long()
        start = torch.gather(st.bursts[:, :, 0].long(), 1, b)
        slot = torch.div(bit0[:, None] + start + 255, 510, rounding_mode="floor")
        good &= (slot % 16 == 0) & (ch[:, None] % PLANT_EVERY == 0)
        st.type1[good] = tmpl[ch[:, None].expand_as(good)[good]]

    def step():
        ta.fill_(-9)
        st()
        nsym = st.bufs[(st.kchunk - 1) & 1][3]
        if plant:
            plant_allocations()
        outs = [_hip.ptr(t) for t in (st.nburst, st.bursts, st.nblock, st.blocks, st.type1)]
        c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(nsym), C, *outs, _hip.ptr(tdma), _hip.ptr(slots), _hip.ptr(npdu),
                                     _hip.ptr(pdus)), "etsi_mac")
        c.check(c.lib.tetra_etsi_sdu(c.handle, _hip.ptr(nsym), C, 1, 0, 0, _hip.TDMA_EXPIRE, *outs, _hip.ptr(npdu),
                                     _hip.ptr(pdus), None, _hip.ptr(sdu), _hip.ptr(sdu_data), _hip.ptr(frag), MAXD,
                                     _hip.ptr(ndone), _hip.ptr(done), _hip.ptr(done_data)), "etsi_sdu")
        c.check(c.lib.tetra_etsi_assign(c.handle, _hip.ptr(nsym), C, 1, 0, 0, _hip.ASSIGN_HOLD_DEFAULT,
                                        _hip.ASSIGN_IDLE_DEFAULT, 0, *outs[:4], _hip.ptr(npdu), _hip.ptr(pdus), None,
                                        _hip.ptr(slots), None, _hip.ptr(sdu), MAXD, _hip.ptr(ndone), _hip.ptr(done),
                                        _hip.ptr(keys), _hip.ptr(state), MAXE, _hip.ptr(nev), _hip.ptr(ev), _hip.ptr(ta)),
                "etsi_assign")
        total["events"] += int(nev.sum())

    for _ in range(2):
        step()
    torch.cuda.synchronize(dev)
    c.check(c.lib.tetra_profile(c.handle, 1), "profile")
    read_profile(c)
    total["events"] = 0
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    prof = read_profile(c)
    c.check(c.lib.tetra_profile(c.handle, 0), "profile")
    print("tetra_profile, C = %d channels x %d samples per step, streaming lower MAC with cell acquisition, %s, %d timed "
          "steps" % (C, N, "allocations planted in the records of one channel in %d" % PLANT_EVERY if plant
                     else "the synthesised payloads", steps))
    for name in STAGES:
        if name in prof:
            print("  %-18s %6.3f ms per step  (%d launches)" % (name, prof[name][0] / steps, prof[name][1]))
    sa = state.cpu().numpy().view(_hip.ETSI_ASSIGN).reshape(C)
    live = torch.arange(_hip.ETSI_MAXB, device=dev)[None, :] < st.nburst[:, None]
    assert bool((ta[~live] == -9).all()) and bool((ta[live][:, 0] >= -1).all())
    states = ta[live][:, _hip.TA_STATE]
    print("last step: bursts %d -- assigned %d, free %d, not followed %d; channels that heard an allocation %d; events in "
          "the timed steps %d; since the start: entries active now %d on %d channels, expired %d, released %d"
          % (int(live.sum()), int((states == 1).sum()), int((states == 0).sum()), int((states == -1).sum()),
             int((nev > 0).sum()), total["events"], int(np.count_nonzero(sa["slot"]["active"])),
             int(np.count_nonzero(sa["slot"]["active"].any(axis=1))), int(sa["expired"].sum()), int(sa["released"].sum())))
    del st
    torch.cuda.empty_cache()


def main():
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    for plant in (False, True):
        run(C, steps, plant)


if __name__ == "__main__":
    main()
