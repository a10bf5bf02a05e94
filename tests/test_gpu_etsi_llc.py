"""tetra_etsi_llc (k_llc_whole, k_llc_done) on the GPU against tests/_etsi_llc_model.py: the call runs on
host arrays built directly -- rows from _etsi_sdu_model.build_rows with that model's Part A as the SDU
records, done records written by hand -- and every output array is compared whole.  The outputs are filled
with a sentinel before the call, so what the call leaves alone shows.

  * whole SDUs: C in {1, 5, 64} with G = 1 and C = 6 with G = 3; blocks of 1..4 PDUs at different BYTE
    offsets; TL-SDUs of 0, 1, 2, 3, 7, 8, 9 bits and the longest a 268-bit block takes; every type; rows
    without blocks, CRC-bad blocks, fragments, encrypted PDUs and whatever _etsi_sdu_cases.random_burst makes;
  * done records: ndone in {0, 1, maxd, maxd + 3}; messages of 36, 37, 40 and 4096 bits and every length
    within 9 bits of 512, 1024 and 2048; one corrupted bit in the first, a middle and the last segment of
    the wave's split; ENC != 0; maxd = 0 with NULL arrays;
  * invalid arguments; device pointers against the host-pointer call;
  * end to end through EtsiLowerMac(mac=True, sdu=True, llc=True) on built rows: a whole BL-UDATA + FCS, a
    three-fragment BL-DATA + FCS, and the same chain with one payload bit flipped in the middle fragment.
  * the wideband surface: WidebandReceiver.decode and WidebandStream(sdu=True, llc=True) on a seven-slot
    capture built as the SDU tests build theirs, one carrier with a two-fragment BL-DATA + FCS.
tests/test_etsi_llc_model.py checks the model itself on the CPU.
"""
import functools

import numpy as np
import pytest

import etsi as E
import _lmac_rows as R
import _etsi_mac_model as M
import _etsi_sdu_cases as K
import _etsi_sdu_model as S
import _etsi_llc_model as L

pytestmark = pytest.mark.gpu

INVALID = -1   # TETRA_E_INVALID
SENT32, SENT8 = -555, 0xA5
TL_LENGTHS = (0, 1, 2, 3, 7, 8, 9)
SDU_CAP = 268 - 43   # a MAC-RESOURCE with an SSI alone in an SCH/F block


# ------------------------------------------------------------------------------ inputs built directly

def resource(sdu_bits, room, enc=0, ssi=0x00ABCD):
    """A MAC-RESOURCE (address type 1, no optional element) around a TM-SDU, padded to whole octets by fill
    bits, or cut at the block's end: (bits, bits used)."""
    used = 43 + len(sdu_bits)
    length = max(2, (used + 7) // 8)
    nbits = min(8 * length, room)
    assert used <= nbits
    return S.resource_pdu(length, 1, sdu_bits, nbits, ssi=ssi, fill=int(nbits != used), enc=enc), nbits


def catalogue(rng):
    """LLC PDUs of every type with every TL-SDU length of the list, and per type the longest one an SCH/F
    block takes, in a seeded order: [(SDU bits, enc)]."""
    out = []
    for t in range(16):
        for n in TL_LENGTHS + ((L.capacity(t, SDU_CAP),) if t < 8 else (SDU_CAP - 4,)):
            out.append((L.llc_pdu(t, K.payload(rng, n), nr=int(rng.integers(2)), ns=int(rng.integers(2))), 0))
    out.append((L.llc_pdu(6, K.payload(rng, 40), flip=20), 0))          # a bad FCS
    out.append((L.llc_pdu(5, K.payload(rng, 24)), 2))                   # encrypted
    out += [(K.payload(rng, n), 0) for n in (1, 2, 3)]                  # too short for a type
    out += [(M.bits_of(4, 4) + K.payload(rng, n), 0) for n in (1, 2, 33)]   # BL-ADATA + FCS below 6 + 32 bits
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def pack_blocks(rng, cat):
    """The catalogue as SCH/F blocks of 1..4 MAC-RESOURCEs, a null PDU behind them where there is room."""
    blocks, cur, room = [], [], 268
    want = int(rng.integers(1, 5))
    for sdu_bits, enc in cat:
        need = 8 * max(2, (43 + len(sdu_bits) + 7) // 8)
        if cur and (len(cur) == want or min(need, 268) > room):
            blocks.append(cur + ([M.null_pdu()] if room >= 16 else []))
            cur, room, want = [], 268, int(rng.integers(1, 5))
        pdu, nbits = resource(sdu_bits, room, enc, ssi=int(rng.integers(1, 1 << 24)))
        cur.append(pdu)
        room -= nbits
    blocks.append(cur + ([M.null_pdu()] if room >= 16 else []))
    return blocks


def whole_rows(rng, C):
    """C rows of up to MAXB bursts: the catalogue's blocks dealt round the rows, then other bursts -- CRC-bad
    blocks, fragments, broadcast, SYNC, anything -- and every fifth row (from row 3) left empty."""
    rows = [[] for _ in range(C)]
    live = [c for c in range(C) if C < 4 or c % 5 != 3]
    for i, blk in enumerate(pack_blocks(rng, catalogue(rng))):
        row = rows[live[i % len(live)]]
        if len(row) < S.MAXB - 2:
            row.append((len(row) * K.SLOT, 0, [blk]))
    for c in live:
        rows[c].append((len(rows[c]) * K.SLOT, 0, [None]))   # CRC-bad
        rows[c].append((len(rows[c]) * K.SLOT,) + K.random_burst(rng))
    return rows


def sdu_outputs(arrays):
    """What tetra_etsi_sdu's Part A leaves for these rows (the SDU model), in sentinel-filled arrays."""
    nburst, bursts, nblock, blocks, type1, npdu, pdus = arrays
    C = len(nblock)
    recs = S.part_a(nblock, blocks, type1, npdu, pdus)
    sdu = np.full((C, S.MAXJ, S.MAXPDU, S.SDU_FIELDS), -3, np.int32)
    sdu_data = np.full((C, S.MAXJ, S.SDU_ROW), 0x3C, np.uint8)
    empty = np.zeros((1, 1, S.DONE_FIELDS), np.int32), np.zeros((1, 1, S.SDU_MAXBYTES), np.uint8)
    sdu, sdu_data, _, _ = S.expected_arrays(recs, None, {}, sdu, sdu_data, *empty)
    return sdu, sdu_data


def done_message(rng, spec):
    """spec = (type, total bits[, flipped bit][, enc]) -> (done record, bytes)."""
    t, n = spec[0], spec[1]
    flip = spec[2] if len(spec) > 2 else None
    rec = rng.integers(0, 50, S.DONE_FIELDS).astype(np.int32)
    rec[S.D_ENC] = spec[3] if len(spec) > 3 else 0
    rec[S.D_NBITS] = n
    k = L.capacity(t, n) if t < 8 else n - 4
    bits = L.llc_pdu(t, K.payload(rng, k), nr=1, ns=1, flip=flip) if k >= 0 else (M.bits_of(t, 4) + K.payload(rng, n))[:n]
    assert len(bits) == n
    return rec, S.pack(bits)


def done_specs():
    specs = [(t, n) for n in (36, 37, 40, 4096) for t in (4, 5, 6, 7)]
    specs += [(4 + (n & 3), n) for c in (512, 1024, 2048) for n in range(c - 9, c + 10)]
    specs += [(1, 517), (2, 4096), (0, 6), (3, 5), (9, 300), (15, 4)]
    # the wave splits a message from its end, eight bytes a lane: of 2048 bits the first, a middle and the last
    # segment, the header, and the FCS itself
    specs += [(5, 2048, 10), (5, 2048, 1000), (5, 2048, 2010), (5, 2048, 2), (5, 2048, 2047), (6, 4096, 4), (6, 36, 35),
              (7, 61, 5)]
    specs += [(5, 300, None, 1), (6, 4096, None, 3), (5, 0), (5, 3)]
    return specs


def done_inputs(rng, NG, maxd):
    """ndone cycling 0, 1, maxd, maxd + 3 over the groups; the specs dealt to the recorded slots in order
    (round again when there are more slots than specs); everything else poison."""
    nd = max(maxd, 1)
    ndone = np.array([(0, 1, maxd, maxd + 3)[g % 4] for g in range(NG)], np.int32)
    done = rng.integers(-9999, 9999, (NG, nd, S.DONE_FIELDS)).astype(np.int32)
    done_data = rng.integers(0, 256, (NG, nd, S.SDU_MAXBYTES)).astype(np.uint8)
    specs, k = done_specs(), 0
    for g in range(NG):
        for i in range(min(int(ndone[g]), maxd)):
            rec, data = done_message(rng, specs[k % len(specs)])
            k += 1
            done[g, i] = rec
            done_data[g, i, :len(data)] = np.frombuffer(data, np.uint8)
    return ndone, done, done_data, k


@functools.lru_cache(maxsize=None)
def case(C, G, maxd):
    rng = np.random.default_rng(1000 * C + 10 * G + maxd)
    arrays = S.build_rows(rng, whole_rows(rng, C))
    sdu, sdu_data = sdu_outputs(arrays)
    ndone, done, done_data, nmsg = done_inputs(rng, C // G, maxd)
    ins = dict(C=C, G=G, maxd=maxd, nblock=arrays[2], blocks=arrays[3], npdu=arrays[5], pdus=arrays[6], sdu=sdu,
               sdu_data=sdu_data, ndone=ndone, done=done, done_data=done_data)
    model = L.run(G, arrays[2], arrays[3], arrays[5], arrays[6], sdu, sdu_data, maxd, ndone, done, done_data)
    for a in ins.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ins, model, nmsg


IN_NAMES = ("nblock", "blocks", "npdu", "pdus", "sdu", "sdu_data", "ndone", "done", "done_data")


def sentinel_outputs(C, G, maxd):
    nd = max(maxd, 1)
    return [np.full((C, S.MAXJ, S.MAXPDU, L.LLC_FIELDS), SENT32, np.int32), np.full((C, S.MAXJ, S.SDU_ROW), SENT8, np.uint8),
            np.full((C // G, nd, L.LLC_FIELDS), SENT32, np.int32), np.full((C // G, nd, S.SDU_MAXBYTES), SENT8, np.uint8)]


def call_llc(ins, outs, device=False):
    """tetra_etsi_llc on host arrays or (device) on torch tensors, sdu_data and done_data at odd addresses;
    outs are updated in place.  Returns the return code."""
    from tetraear import _hip
    c = _hip.ctx()
    args = [ins[k] for k in IN_NAMES] + list(outs)
    args = [None if a is None else np.ascontiguousarray(a) for a in args]
    if device:
        import torch
        dev = [None if a is None else torch.from_numpy(a.copy()).cuda() for a in args]
        for i in (5, 8):
            if dev[i] is not None:
                odd = torch.zeros(args[i].size + 1, dtype=torch.uint8, device="cuda")
                odd[1:] = dev[i].reshape(-1)
                dev[i] = odd[1:]
                assert dev[i].data_ptr() % 2 == 1
        p = [_hip.ptr(a) for a in dev]
    else:
        p = [_hip.ptr(a) for a in args]
    rc = c.lib.tetra_etsi_llc(c.handle, ins["C"], ins["G"], p[0], p[1], p[2], p[3], p[4], p[5], ins["maxd"], p[6], p[7],
                              p[8], p[9], p[10], p[11], p[12])
    if device:
        torch.cuda.synchronize()
        for host, d in zip(outs, dev[9:]):
            if host is not None:
                host[...] = d.cpu().numpy().reshape(host.shape)
    return rc


def check(C, G, maxd, device=False):
    ins, (a, b), _ = case(C, G, maxd)
    outs = sentinel_outputs(C, G, maxd)
    want = L.expected_arrays(a, b, *outs)
    assert call_llc(ins, outs, device) == 0
    for name, got, exp in zip(("llc", "tl", "llc_done", "tl_done"), outs, want):
        assert np.array_equal(got, exp), (C, G, name, np.argwhere(got != exp)[:4].tolist())
    return a, b, outs


# ------------------------------------------------------------------------------ against the model

@pytest.mark.parametrize("C,G", [(1, 1), (5, 1), (64, 1), (6, 3)])
def test_records_equal_the_model(C, G):
    a, b, outs = check(C, G, 4)
    if C == 64:   # the cases are all there: every type read, every TL-SDU length, every verdict
        ok = [r for r, _, _ in a.values() if r[L.STATUS] == L.OK]
        assert {r[L.TYPE] for r in ok} == set(range(8))
        assert {r[L.TYPE] for r, _, _ in a.values() if r[L.STATUS] == L.UNSUPPORTED} == set(range(8, 16))
        assert set(TL_LENGTHS) | {L.capacity(t, SDU_CAP) for t in range(8)} <= {r[L.NBITS] for r in ok}
        assert {r[L.STATUS] for r, _, _ in a.values()} == {L.OK, L.NONE, L.MALFORMED, L.ENCRYPTED, L.UNSUPPORTED}
        assert {r[L.FCS] for r in ok} == {L.FCS_NONE, L.FCS_GOOD, L.FCS_BAD}
        assert len({at for _, _, at in a.values()}) >= 4   # SDUs at different BYTE offsets
        assert case(C, G, 4)[2] >= len(done_specs())   # every done spec was dealt
        done = [r for r, _ in b.values()]
        assert {r[L.STATUS] for r in done} == {L.OK, L.NONE, L.MALFORMED, L.ENCRYPTED, L.UNSUPPORTED}
        assert sum(r[L.FCS] == L.FCS_BAD for r in done) >= 8 and sum(r[L.FCS] == L.FCS_GOOD for r in done) >= 60
        # untouched: records of rows without blocks, and everything past min(ndone, maxd)
        ins = case(C, G, 4)[0]
        assert (ins["nblock"] == 0).any() and (outs[0][ins["nblock"] == 0] == SENT32).all()
        assert (outs[2][ins["ndone"] == 0] == SENT32).all() and (outs[2][ins["ndone"] == 1, 1:] == SENT32).all()


def test_crc_bad_blocks_and_rows_without_blocks_stay_untouched():
    ins, (a, _), _ = case(5, 1, 4)
    outs = sentinel_outputs(5, 1, 4)
    assert call_llc(ins, outs) == 0
    bad = [(c, j) for c in range(5) for j in range(int(ins["nblock"][c])) if ins["blocks"][c, j, 1] == 0]
    assert bad and all((outs[0][c, j] == SENT32).all() and (outs[1][c, j] == SENT8).all() for c, j in bad)
    assert (outs[0][3] == SENT32).all() and ins["nblock"][3] == 0
    written = {(c, j) for c, j, _ in a}
    assert all((outs[0][c, j] == SENT32).all() for c in range(5) for j in range(S.MAXJ) if (c, j) not in written)


@pytest.mark.parametrize("maxd", [1, 7])
def test_done_counts_at_other_maxd(maxd):
    check(8, 1, maxd)


def test_maxd_zero_with_null_arrays():
    ins, (a, b), _ = case(5, 1, 0)
    assert not b
    outs = sentinel_outputs(5, 1, 0)
    want = L.expected_arrays(a, b, outs[0], outs[1], None, None)
    ins = dict(ins, done=None, done_data=None)
    outs[2] = outs[3] = None
    assert call_llc(ins, outs) == 0
    assert np.array_equal(outs[0], want[0]) and np.array_equal(outs[1], want[1])


def test_device_pointers_give_the_host_call_s_bytes():
    _, _, host = check(64, 1, 4)
    _, _, dev = check(64, 1, 4, device=True)
    assert all(np.array_equal(x, y) for x, y in zip(host, dev))
    check(6, 3, 4, device=True)


def test_invalid_arguments_write_nothing():
    good = case(6, 3, 4)[0]
    bad = [dict(good, G=0), dict(good, G=4), dict(good, G=65), dict(good, maxd=-1), dict(good, C=0),
           dict(good, C=(1 << 24) + 3)]
    bad += [dict(good, **{k: None}) for k in IN_NAMES]
    for ins in bad:
        outs = sentinel_outputs(6, 3, 4)
        assert call_llc(ins, outs) == INVALID, {k: v for k, v in ins.items() if not isinstance(v, np.ndarray)}
        assert all((o == s).all() for o, s in zip(outs, (SENT32, SENT8, SENT32, SENT8)))
    for j in range(4):   # a NULL output
        outs = sentinel_outputs(6, 3, 4)
        outs[j] = None
        assert call_llc(good, outs) == INVALID, j
        assert all(o is None or (o == s).all() for o, s in zip(outs, (SENT32, SENT8, SENT32, SENT8)))
    check(6, 3, 4)   # a good call after the refusals


# ------------------------------------------------------------------------------ through the public surface

CELL = (262, 1017, 33)


@functools.lru_cache(maxsize=None)
def planted():
    """One carrier's row of consecutive bursts on the slot grid (place_bursts: burst_stream's random gaps
    leave it, and a chain over several bursts needs it, as in the SDU tests): an SB on slot 0; on slot 1 a
    whole BL-UDATA + FCS whose TL-SDU opens with discriminator 2 (CMCE) and type 15; on slots 2, 6, 10 a
    BL-DATA + FCS in three fragments; on slots 3, 7, 11 the same message with one payload bit flipped in
    the middle fragment (the blocks are encoded from the flipped bits, so their CRC-16 passes).  Null PDUs
    elsewhere.  Returns (bits, the three TM-SDUs' bits)."""
    rng = np.random.default_rng(4242)
    init = E.scramble_init(*CELL)
    whole = L.llc_pdu(6, M.bits_of(2, 3) + M.bits_of(15, 5) + K.payload(rng, 64))
    n = K.sdu_len(rng, 3)
    chain = L.llc_pdu(5, M.bits_of(1, 3) + K.payload(rng, L.capacity(5, n) - 3), ns=1)
    assert len(chain) == n
    hurt = list(chain)
    hurt[K.FIRST_CAP + 100] ^= 1
    at = {1: [resource(whole, 268, ssi=0xBEEF11)[0], M.null_pdu()]}
    for first_slot, sdu, ssi in ((2, chain, 0xBEEF12), (3, hurt, 0xBEEF13)):
        for i, pd in enumerate(S.fragment(sdu, [0, 0, 0], ssi=ssi)):
            at[first_slot + 4 * i] = [pd] if i < 2 else [pd, M.null_pdu()]
    items = []
    for b in range(13):
        if b == 0:
            pay, kind = [M.block(rng, 2, [M.sync(M.sync_for_slot(rng, 40, CELL))]), M.block(rng, 1, [M.null_pdu()])], 2
        elif b in at:
            pay, kind = [M.block(rng, 0, at[b])], 0
        else:
            kind = int(rng.integers(0, 2))
            pay = [M.block(rng, k, [M.null_pdu()]) for k in S.BLOCKS_OF[kind]]
        items.append((9 if b == 0 else 0, kind, init, pay))
    bits, _, _ = R.place_bursts(rng, items, tail_gap=40)
    return bits, (whole, chain, hurt)


def stream_frames(lm, cut_seed=5):
    bits, _ = planted()
    h, s = R.hard_of(bits), R.soft_of(bits)
    frames = []
    for at, n in R.chunk_cuts(cut_seed, len(bits) // 2, (700, 1500, 1790)):
        hard, soft = np.zeros((1, n + 2), np.uint8), np.zeros((1, 2 * n + 4), np.int8)
        hard[0, :n], soft[0, :2 * n] = h[at:at + n], s[2 * at:2 * (at + n)]
        frames += lm.decode_stream(soft, hard, np.array([n + 1], np.int32))[0]
    return frames


def plain(x, drop=("llc",)):
    """Frames as plain Python, without the keys llc=True adds."""
    if isinstance(x, dict):
        return {k: plain(v, drop) for k, v in x.items() if k not in drop}
    if isinstance(x, (list, tuple)):
        return [plain(v, drop) for v in x]
    return x.tolist() if isinstance(x, np.ndarray) else x


def has_key(x, key):
    if isinstance(x, dict):
        return key in x or any(has_key(v, key) for v in x.values())
    return isinstance(x, (list, tuple)) and any(has_key(v, key) for v in x)


def test_lower_mac_frames_and_link_messages():
    from tetraear.core.etsi import EtsiLowerMac, link_messages, messages
    cell = dict(zip(("mcc", "mnc", "colour_code"), CELL))
    for kw in (dict(llc=True), dict(mac=True, llc=True), dict(sdu=True, llc=True)):
        with pytest.raises(ValueError):
            EtsiLowerMac(**kw, **cell)
    _, (whole, chain, hurt) = planted()
    off = stream_frames(EtsiLowerMac(mac=True, sdu=True, **cell))
    on = stream_frames(EtsiLowerMac(mac=True, sdu=True, llc=True, **cell))
    # llc=False: no frame knows of it, and llc=True changes nothing else, key for key
    assert not has_key(off, "llc") and has_key(on, "llc") and plain(on) == plain(off, drop=()) and len(off) >= 12
    assert all("llc" in p for f in on for b in f["blocks"] for p in b["pdus"])
    msgs = messages(on)
    assert [m["data"] for m in msgs] == [S.pack(whole), S.pack(chain), S.pack(hurt)]
    assert [m["llc"]["fcs"] for m in msgs] == [True, True, False]
    assert [m["fragments"] for m in msgs] == [1, 3, 3] and all(m["llc"]["status"] == 0 for m in msgs)
    assert [(m["llc"]["type"], m["llc"]["name"], m["llc"]["nr"], m["llc"]["ns"]) for m in msgs] == \
        [(6, "BL-UDATA+FCS", None, None), (5, "BL-DATA+FCS", None, 1), (5, "BL-DATA+FCS", None, 1)]
    for m, sdu in zip(msgs, (whole, chain, hurt)):
        ll = m["llc"]
        assert ll["tl_sdu_bits"] == len(sdu) - (4 if ll["type"] == 6 else 5) - 32
        assert ll["tl_sdu"] == S.pack(sdu[len(sdu) - 32 - ll["tl_sdu_bits"]:len(sdu) - 32])
        assert ll["fcs_rx"] == M._get(sdu, len(sdu) - 32, 32) and ll["fcs_calc"] == L.fcs(sdu[:-32])
    assert msgs[2]["llc"]["fcs_rx"] == msgs[1]["llc"]["fcs_rx"] != msgs[2]["llc"]["fcs_calc"]
    link = link_messages(on)
    assert len(link) == 2 and [m["fcs"] for m in link] == [True, True]
    assert (link[0]["protocol_name"], link[0]["pdu_name"]) == ("CMCE", "D-SDS-DATA")
    assert link[0]["llc"]["protocol"] == 2 and link[0]["llc"]["pdu_type"] == 15
    assert link[0]["tl_sdu"] == S.pack(whole[4:-32]) and link[1]["protocol_name"] == "MM" and link[1]["pdu_name"] is None
    both = link_messages(on, drop_bad_fcs=False)
    assert len(both) == 3 and both[2]["fcs"] is False and both[2]["tl_sdu"] == S.pack(hurt[5:-32])
    assert link_messages(off) == []


def test_decoder_passes_llc_through():
    from tetraear.core import TetraDecoder
    from tetraear.core.etsi import link_messages
    with pytest.raises(ValueError):
        TetraDecoder(auto_decrypt=False, mode="etsi", mac=True, llc=True)._etsi_rx()
    bits, (whole, _, _) = planted()
    bits = bits[:8 * 510]   # the SB, the whole message and the chains' first fragments: one decode_batch row
    hard, soft, nsym = R.pack_rows([(bits, R.soft_of(bits))], len(bits) // 2 + 2)
    cells = np.array([E.scramble_init(*CELL)], np.uint32)
    dec = TetraDecoder(auto_decrypt=False, mode="etsi", mac=True, sdu=True, llc=True)
    raw = dec._etsi_rx().decode_batch(soft, hard, nsym, cells=cells)[0]
    got = link_messages(raw)
    assert [(m["tl_sdu"], m["fcs"], m["pdu_name"]) for m in got] == [(S.pack(whole[4:-32]), True, "D-SDS-DATA")]
    frames = dec._etsi_frames(raw)
    tagged = [p["llc"] for f in frames for p in f["mac_pdus"] if "llc" in p and p["llc"]["status"] == 0]
    assert [ll["pdu_name"] for ll in tagged] == ["D-SDS-DATA"]


# the wideband chain: one capture of seven slots as in tests/test_gpu_etsi_sdu.py, one carrier with a
# two-fragment BL-DATA + FCS (CMCE, D-SETUP) on slots 1 and 5, the cell given
NW = 2_000_000
WB_CARRIER = 401


@functools.lru_cache(maxsize=None)
def wb_capture():
    import wideband as W
    d = W.design()
    nbb = NW // d["D"] + 1
    rng = np.random.default_rng(971)
    init = E.scramble_init(*CELL)
    sdu = L.llc_pdu(5, M.bits_of(2, 3) + M.bits_of(7, 5) + K.payload(rng, L.capacity(5, K.sdu_len(rng, 2)) - 8), ns=0)
    pdus = S.fragment(sdu, [0, 0], ssi=0xBEEF21)
    at = {1: [pdus[0]], 5: [pdus[1], M.null_pdu()]}
    items = []
    for b in range(7):
        kind = 0 if b in at else int(rng.integers(0, 2))
        pay = [M.block(rng, 0, at[b])] if b in at else [M.block(rng, k, [M.null_pdu()]) for k in S.BLOCKS_OF[kind]]
        items.append((100 if b == 0 else 0, kind, init, pay))
    bits, _, _ = R.place_bursts(rng, items, tail_gap=40)
    s = np.zeros((d["M"], nbb), np.complex128)
    cells = np.full(d["M"], 3, np.uint32)
    cells[WB_CARRIER] = init
    s[WB_CARRIER] = E.modulate(bits, nbb, fs=d["fs"] / d["D"], t0=0.23, phase0=0.7, cfo=25.0)
    return W.synthesize(s, d, NW).astype(np.complex64), cells, sdu


def test_wideband_decode_and_stream():
    from tetraear.core.etsi import link_messages
    from tetraear.signal.wideband import WidebandReceiver, WidebandStream
    x, cells, sdu = wb_capture()
    rx = WidebandReceiver()
    with pytest.raises(ValueError):
        rx.decode(x[:1000], cells, mac=True, timebase="vote", llc=True)
    with pytest.raises(ValueError):
        WidebandStream(cells, mac=True, timebase="vote", llc=True)
    want = [(S.pack(sdu[5:-32]), len(sdu) - 37, True, "CMCE", "D-SETUP", 2, S.pack(sdu))]

    def read(frames):
        return [(m["tl_sdu"], m["tl_sdu_bits"], m["fcs"], m["protocol_name"], m["pdu_name"], m["fragments"], m["data"])
                for m in link_messages(frames) if m["fragments"] > 1]
    off = rx.decode(x, cells, mac=True, timebase="vote", sdu=True)
    on = rx.decode(x, cells, mac=True, timebase="vote", sdu=True, llc=True)
    assert read(on[WB_CARRIER]) == want and not has_key(off, "llc") and plain(on) == plain(off, drop=())
    st = WidebandStream(cells, mac=True, timebase="vote", sdu=True, llc=True)
    frames = []
    for a, b in ((0, 611_111), (611_111, 700_001), (700_001, NW)):
        frames += st.decode(x[a:b])[WB_CARRIER]
    assert read(frames) == want   # once, though the carried tails are decoded twice
