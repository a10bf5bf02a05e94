"""tetra_etsi_traffic restated in numpy (TEST INFRASTRUCTURE).

The records of include/tetra_hip.h: every burst of a lower-MAC call gets a class from the block
records (and, when given, the MAC call's slots and keep), and a FULL or HALF burst's block fields
come out descrambled with the cell's sequence (oracle/etsi.py scramble_seq).  All integers: the
kernel is held to this model bit for bit.  Row builders on top of tests/_lmac_rows.py follow.
"""
import numpy as np

import etsi as E
import _etsi_quality_model as Q

MAXB, MAXJ, NF, NBITS_MAX = 8, 16, 4, 432
CLASS, NBITS, WSUM, NZERO = range(4)
NONE, CONTROL, FULL, HALF, LOST = range(5)
SLOT_FN = 1
POISON, POISON8 = -777, 0x5A


def field_offsets(cls):
    """Bits from the burst's start to the exported positions of a FULL / HALF slot."""
    if cls == HALF:
        return 282 + np.arange(216)
    i = np.arange(432)
    return np.where(i < 216, 14 + i, 282 + (i - 216))


def descramble(s, q):
    """tch_i = q_i ? (s_i == -128 ? 127 : -s_i) : s_i."""
    s = np.asarray(s, np.int64)
    return np.where(np.asarray(q) == 1, np.where(s == -128, 127, -s), s).astype(np.int8)


def classify(kind, b, nk, blocks):
    """Rules e and f: the class of valid burst b of kind 0 / 1 from the row's first nk block records."""
    def good(idx):
        return any(int(r[0]) == kind and int(r[1]) != 0 and int(r[2]) == b and int(r[3]) == idx for r in blocks[:nk])
    if kind == 0:
        return CONTROL if good(0) else FULL
    g0, g1 = good(0), good(1)
    return CONTROL if g0 and g1 else HALF if g0 else LOST


def traffic(soft, origin, G, cell_init, nburst, bursts, nblock, blocks, slots=None, keep=None, tq=None, tch=None):
    """soft [C, 2 stride] int8 and a lower-MAC call's outputs -> (tq [C, 8, 4] int32, tch [C, 8, 432] int8);
    what the call does not write keeps tq / tch as passed (POISON / POISON8 when None)."""
    C, stride = soft.shape[0], soft.shape[1] // 2
    assert G >= 1 and C % G == 0 and len(cell_init) == C // G and origin >= 0
    tq = np.full((C, MAXB, NF), POISON, np.int32) if tq is None else tq.copy()
    tch = np.full((C, MAXB, NBITS_MAX), POISON8, np.int8) if tch is None else tch.copy()
    for c in range(C):
        nb, nk = min(max(int(nburst[c]), 0), MAXB), min(max(int(nblock[c]), 0), MAXJ)
        scr = E.scramble_seq(int(cell_init[c // G]), 432)
        for b in range(nb):
            start, kind = int(bursts[c, b, 0]), int(bursts[c, b, 1])
            if not Q.burst_valid(start, kind, origin, stride):
                tq[c, b] = -1
                continue
            if keep is not None and int(keep[c, b]) == 0:
                cls = NONE
            elif kind == 2:
                cls = NONE
            elif slots is not None and int(slots[c, b, SLOT_FN]) == 18:
                cls = CONTROL
            else:
                cls = classify(kind, b, nk, blocks[c])
            if cls not in (FULL, HALF):
                tq[c, b] = [cls, 0, 0, 0]
                continue
            off = field_offsets(cls)
            t = descramble(soft[c, origin + start + off], scr[:len(off)])
            tch[c, b, :len(off)] = t
            tq[c, b] = [cls, len(off), int(np.abs(t.astype(np.int64)).sum()), int((t == 0).sum())]
    return tq, tch


def call(soft, origin, G, cell_init, o, slots=None, keep=None, tq=None, tch=None, device=False, ctx=None, tch_offset=0,
         stride=None):
    """tetra_etsi_traffic on host arrays, or on device copies of them: (rc, tq, tch).  o: the lower-MAC
    call's outputs as _lmac_rows.lmac_outputs; tq / tch: what the outputs hold before.  tch_offset
    (device): the tch base lies that many bytes past an allocation's start."""
    from tetraear import _hip
    c = ctx if ctx is not None else _hip.ctx()
    C = soft.shape[0]
    stride = soft.shape[1] // 2 if stride is None else stride
    tq = np.full((C, MAXB, NF), POISON, np.int32) if tq is None else tq.copy()
    tch = np.full((C, MAXB, NBITS_MAX), POISON8, np.int8) if tch is None else tch.copy()
    ci = None if cell_init is None else np.ascontiguousarray(cell_init, np.uint32).view(np.int32)
    args = [soft, ci, o["nburst"], o["bursts"], o["nblock"], o["blocks"],
            None if slots is None else np.ascontiguousarray(slots, np.int32),
            None if keep is None else np.ascontiguousarray(keep, np.int32), tq, tch]
    if device:
        import torch
        dev = torch.device("cuda", 0)
        args = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray)
                else a.t for a in args]   # (an object with .t and .shape: rows already on the device)
        if tch_offset:
            buf = torch.full((tch.size + 16,), POISON8, dtype=torch.int8, device=dev)
            buf[tch_offset:tch_offset + tch.size] = args[9].reshape(-1)
            args[9] = buf[tch_offset:tch_offset + tch.size]
        torch.cuda.synchronize(dev)
    p = [_hip.ptr(a) for a in args]
    rc = c.lib.tetra_etsi_traffic(c.handle, p[0], C, stride, origin, G, *p[1:])
    if device:
        c.synchronize()
        tq, tch = args[8].cpu().numpy(), args[9].cpu().numpy().reshape(tch.shape)
        if tch_offset:
            edge = buf.cpu().numpy()
            assert (edge[:tch_offset] == POISON8).all() and (edge[tch_offset + tch.size:] == POISON8).all()
    return rc, tq, tch


# ------------------------------------------------------------------------------ built bursts

def traffic_burst(kind, t4, scr, rng=None):
    """oracle/etsi.py make_burst of a normal burst with the traffic fields overwritten: kind 0 (training
    sequence n) holds t4 ^ scr in its two block fields (a full slot); kind 1 (training sequence p) keeps
    a coded SCH/HD in its first field (the stolen half) and holds t4[:216] ^ scr[:216] in its second.
    Returns (bits, [(block kind, type-1)] of the blocks that still decode)."""
    rng = np.random.default_rng(0) if rng is None else rng
    t4, scr = np.asarray(t4, np.uint8), np.asarray(scr, np.uint8)
    bits, jobs = E.make_burst(kind, rng, scr)
    bits = bits.copy()
    if kind == 0:
        x = t4[:432] ^ scr[:432]
        bits[14:230], bits[282:498] = x[:216], x[216:]
        return bits, []
    assert kind == 1
    bits[282:498] = t4[:216] ^ scr[:216]
    return bits, jobs[:1]


def signs(tch):
    """The bits a descrambled soft row decides for: positive means 0."""
    return (np.asarray(tch) < 0).astype(np.uint8)
