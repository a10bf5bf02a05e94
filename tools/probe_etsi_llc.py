#!/usr/bin/env python3
"""Stage times of the streaming ETSI step with tetra_etsi_mac, tetra_etsi_sdu and tetra_etsi_llc behind the
lower MAC (tetra_profile's HIP events, one context, the stages one after another): etsi_llc against
etsi_sdu of the same run, three repeats of the timed steps a run.  The step runs on two inputs: the
synthesised captures as they are (random payloads: few whole SDUs read as LLC PDUs, next to no message
completes -- the cost of looking), and with LLC PDUs planted.  tetra_synth_etsi takes no payloads, so
they are planted in the blocks the lower MAC left, on the device, as tools/probe_etsi_sdu.py plants its
chains: every CRC-good SCH/F block becomes one of the six fragments of a 1536-bit BL-DATA + FCS by its
burst's place on the stream's slot grid (four slots apart, on all four timeslots), every CRC-good SCH/HD
block a whole BL-UDATA + FCS of 77 bits, and tetra_etsi_mac, tetra_etsi_sdu and tetra_etsi_llc run on those.
The capture holds steps + 2 chunks; the repeats run on past its end, where the stream starts again.
usage: probe_etsi_llc.py [channels] [steps] [repeats]  """
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tetraear-bladerf_amd"), REPO]

STAGES = ("etsi_demod", "etsi_traceback", "etsi_mac", "etsi_sdu", "etsi_llc")
CHAIN = 6   # fragments per planted message
MAXD = 4
FIRST_CAP, MID_CAP, LAST_CAP = 268 - 43, 268 - 4, 268 - 13


def read_profile(c):
    names = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 64)()
    n = ctypes.c_int(0)
    c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    raw = names.raw.split(b"\0")
    return {raw[i].decode(): (ms[i], int(cnt[i])) for i in range(n.value)}


def bits_of(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def with_fcs(bits):
    """The bits and their frame check sequence (include/tetra_hip.h, tetra_etsi_llc)."""
    r = 0xFFFFFFFF
    for b in bits:
        t = (r >> 31) ^ b
        r = (r << 1) & 0xFFFFFFFF
        if t:
            r ^= 0x04C11DB7
    return bits + bits_of(r ^ 0xFFFFFFFF, 32)


def templates(torch, dev):
    """[CHAIN, 268] type-1 bytes -- a MAC-RESOURCE (L = 63, SSI), MAC-FRAGs, a MAC-END (L = 63), full blocks
    that carry one BL-DATA + FCS between them -- and [124]: a MAC-RESOURCE of 15 octets around a whole
    BL-UDATA + FCS, CMCE D-SDS-DATA in front."""
    g = torch.Generator().manual_seed(7)

    def rand(n):
        return torch.randint(0, 2, (n,), generator=g, dtype=torch.uint8).tolist()
    total = FIRST_CAP + (CHAIN - 2) * MID_CAP + LAST_CAP
    msg = with_fcs(bits_of(5, 4) + [1] + bits_of(2, 3) + bits_of(15, 5) + rand(total - 5 - 8 - 32))
    ssi = [1, 0] * 12
    heads = [[0] * 7 + [1] * 6 + [0, 0, 1] + ssi + [0, 0, 0]] + [[0, 1, 0, 0]] * (CHAIN - 2) + [[0, 1, 1, 0, 0] + [1] * 6 + [0, 0]]
    rows, at = [], 0
    for h in heads:
        rows.append(h + msg[at:at + 268 - len(h)])
        at += 268 - len(h)
    assert at == len(msg) == total
    whole = [0] * 7 + bits_of(15, 6) + [0, 0, 1] + ssi + [0, 0, 0] + \
        with_fcs(bits_of(6, 4) + bits_of(2, 3) + bits_of(15, 5) + rand(33)) + rand(4)
    assert len(whole) == 124
    return torch.tensor(rows, dtype=torch.uint8).to(dev), torch.tensor(whole, dtype=torch.uint8).to(dev)


def run(C, steps, repeats, plant):
    import torch
    from tetraear import _hip
    from tetraear.signal.etsi import BenchStep
    N = 131072
    dev = torch.device("cuda", 0)
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    st = BenchStep(c, C, N, 2.4e6, 1, dev, cells="acquire", chunks=steps + 2)
    MAXJ, MAXPDU = _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU
    tdma = torch.zeros((C, 3), dtype=torch.int64, device=dev)
    slots = torch.zeros((C, _hip.ETSI_MAXB, _hip.SLOT_FIELDS), dtype=torch.int32, device=dev)
    npdu = torch.zeros((C, MAXJ), dtype=torch.int32, device=dev)
    pdus = torch.zeros((C, MAXJ, MAXPDU, _hip.PDU_FIELDS), dtype=torch.int32, device=dev)
    sdu = torch.full((C, MAXJ, MAXPDU, _hip.SDU_FIELDS), -9, dtype=torch.int32, device=dev)
    sdu_data = torch.zeros((C, MAXJ, _hip.SDU_ROW), dtype=torch.uint8, device=dev)
    frag = torch.zeros((C, _hip.ETSI_FRAG.itemsize), dtype=torch.uint8, device=dev)
    ndone = torch.zeros(C, dtype=torch.int32, device=dev)
    done = torch.zeros((C, MAXD, _hip.DONE_FIELDS), dtype=torch.int32, device=dev)
    done_data = torch.zeros((C, MAXD, _hip.SDU_MAXBYTES), dtype=torch.uint8, device=dev)
    llc = torch.full((C, MAXJ, MAXPDU, _hip.LLC_FIELDS), -9, dtype=torch.int32, device=dev)
    tl = torch.zeros((C, MAXJ, _hip.SDU_ROW), dtype=torch.uint8, device=dev)
    llc_done = torch.full((C, MAXD, _hip.LLC_FIELDS), -9, dtype=torch.int32, device=dev)
    tl_done = torch.zeros((C, MAXD, _hip.SDU_MAXBYTES), dtype=torch.uint8, device=dev)
    tmpl, whole = templates(torch, dev)
    total = {"done": 0, "early": 0, "groups": 0, "good": 0, "bad": 0}

    def plant_pdus():
        """Every CRC-good SCH/F block gets the fragment its burst's slot calls for, every SCH/HD block the
        whole PDU."""
        bit0 = frag[:, :8].contiguous().view(torch.int64)[:, 0]
        j = torch.arange(MAXJ, device=dev)[None, :]
        live = (j < st.nblock[:, None]) & (st.blocks[:, :, 1] != 0)
        good = live & (st.blocks[:, :, 0] == 0)
        b = st.blocks[:, :, 2].clamp(0, _hip.ETSI_MAXB - 1).long()
        start = torch.gather(st.bursts[:, :, 0].long(), 1, b)
        slot = torch.div(bit0[:, None] + start + 255, 510, rounding_mode="floor")
        place = torch.div(slot, 4, rounding_mode="floor") % CHAIN
        st.type1[good] = tmpl[place[good]]
        half = live & (st.blocks[:, :, 0] == 1)
        t1 = st.type1
        t1[:, :, :124] = torch.where(half[:, :, None], whole[None, None, :], t1[:, :, :124])

    def step(count):
        st()
        nsym = st.bufs[(st.kchunk - 1) & 1][3]
        if plant:
            plant_pdus()
        outs = [_hip.ptr(t) for t in (st.nburst, st.bursts, st.nblock, st.blocks, st.type1)]
        c.check(c.lib.tetra_etsi_mac(c.handle, _hip.ptr(nsym), C, *outs, _hip.ptr(tdma), _hip.ptr(slots), _hip.ptr(npdu),
                                     _hip.ptr(pdus)), "etsi_mac")
        c.check(c.lib.tetra_etsi_sdu(c.handle, _hip.ptr(nsym), C, 1, 0, 0, _hip.TDMA_EXPIRE, *outs, _hip.ptr(npdu),
                                     _hip.ptr(pdus), None, _hip.ptr(sdu), _hip.ptr(sdu_data), _hip.ptr(frag), MAXD,
                                     _hip.ptr(ndone), _hip.ptr(done), _hip.ptr(done_data)), "etsi_sdu")
        c.check(c.lib.tetra_etsi_llc(c.handle, C, 1, _hip.ptr(st.nblock), _hip.ptr(st.blocks), _hip.ptr(npdu),
                                     _hip.ptr(pdus), _hip.ptr(sdu), _hip.ptr(sdu_data), MAXD, _hip.ptr(ndone),
                                     _hip.ptr(done), _hip.ptr(done_data), _hip.ptr(llc), _hip.ptr(tl), _hip.ptr(llc_done),
                                     _hip.ptr(tl_done)), "etsi_llc")
        if count:   # outside the stages' events; the profile sums device time between them only
            n = ndone.clamp(0, MAXD)
            rec = torch.arange(MAXD, device=dev)[None, :] < n[:, None]
            total["done"] += int(ndone.sum())
            total["early"] += int((ndone <= 0).sum())
            total["groups"] += C
            total["good"] += int(((llc_done[:, :, _hip.LLC_FCS] == _hip.FCS_GOOD) & rec).sum())
            total["bad"] += int(((llc_done[:, :, _hip.LLC_FCS] == _hip.FCS_BAD) & rec).sum())

    for _ in range(2):
        step(False)
    torch.cuda.synchronize(dev)
    print("tetra_profile, C = %d channels x %d samples per step, streaming lower MAC with cell acquisition, %s, %d "
          "repeats of %d timed steps" % (C, N, "LLC PDUs planted in the blocks" if plant else "the synthesised payloads",
                                         repeats, steps))
    for rep in range(repeats):
        c.check(c.lib.tetra_profile(c.handle, 1), "profile")
        read_profile(c)
        for _ in range(steps):
            step(True)
        torch.cuda.synchronize(dev)
        prof = read_profile(c)
        c.check(c.lib.tetra_profile(c.handle, 0), "profile")
        print("  repeat %d: " % (rep + 1) + "  ".join("%s %.3f" % (name, prof[name][0] / steps) for name in STAGES if name in prof)
              + "  ms per step")
    j = torch.arange(MAXJ, device=dev)[None, :]
    live = (j < st.nblock[:, None]) & (npdu > 0) & (st.blocks[:, :, 1] != 0)
    rec = torch.arange(MAXPDU, device=dev)[None, :] < npdu[live].clamp(max=MAXPDU)[:, None]
    status = llc[live][:, :, _hip.LLC_STATUS]
    fcs = llc[live][:, :, _hip.LLC_FCS]
    counts = [int(((status == s) & rec).sum()) for s in range(5)]
    print("last step: blocks with PDUs %d, records %d: LLC ok %d, none %d, malformed %d, encrypted %d, unsupported %d; "
          "whole SDUs with a good FCS %d, a bad one %d" % (int(live.sum()), int(rec.sum()), *counts,
                                                          int(((fcs == _hip.FCS_GOOD) & rec & (status == 0)).sum()),
                                                          int(((fcs == _hip.FCS_BAD) & rec & (status == 0)).sum())))
    print("timed steps: messages completed %d (FCS good %d, bad %d, among the first %d a channel); the done kernel left "
          "after one load in %d of %d groups (%.1f %%)" % (total["done"], total["good"], total["bad"], MAXD, total["early"],
                                                           total["groups"], 100.0 * total["early"] / max(total["groups"], 1)))
    del st
    torch.cuda.empty_cache()


def main():
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    for plant in (False, True):
        run(C, steps, repeats, plant)


if __name__ == "__main__":
    main()
