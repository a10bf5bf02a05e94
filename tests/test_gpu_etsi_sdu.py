"""tetra_etsi_sdu (k_sdu_walk, k_sdu_join) on the GPU against tests/_etsi_sdu_model.py: every output array
compared whole -- the outputs are poisoned before the call, so what it leaves alone shows -- and the
carried fragment state after every call.

  * the scenarios of tests/_etsi_sdu_cases.py (every rule of the walk at its edge, chains, groups of
    overlapping rows), stacked into calls of 17 rows and 1 row, with host and with device pointers, the
    device type-1 pointer odd;
  * a seeded sweep over C in {1, 5, 17, 33, ...} rows and G in {1, 2, 3, 64} rows per group;
  * built rows through tetra_lmac_etsi_stream -> tetra_etsi_mac -> tetra_etsi_sdu over random chunk cuts:
    the planted TM-SDU comes back byte for byte whatever the cuts (no model involved);
  * the Python surfaces, and the argument checks.
tests/test_etsi_sdu_model.py checks the model itself on the CPU.
"""
import functools
import os

import numpy as np
import pytest

import etsi as E
import _lmac_rows as R
import _etsi_mac_model as M
import _etsi_sdu_cases as K
import _etsi_sdu_model as S

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("TETRA_FUZZ_SCALE", "1")))
INVALID = -1   # TETRA_E_INVALID


# ------------------------------------------------------------------------------ the library's call

def poisoned_outputs(seed, C, G, maxd):
    rng = np.random.default_rng(seed)
    nd = max(maxd, 1)
    return [rng.integers(-99, 99, (C, S.MAXJ, S.MAXPDU, S.SDU_FIELDS)).astype(np.int32),
            rng.integers(0, 256, (C, S.MAXJ, S.SDU_ROW)).astype(np.uint8),
            np.full(C // G, -77, np.int32),
            rng.integers(-99, 99, (C // G, nd, S.DONE_FIELDS)).astype(np.int32),
            rng.integers(0, 256, (C // G, nd, S.SDU_MAXBYTES)).astype(np.uint8)]


SMALL = {"nsym": 0, "nburst": 1, "nblock": 3, "npdu": 6, "keep": 8}   # the arrays that share one staged input


def call_sdu(call, frag, outs, device=False, mixed=()):
    """tetra_etsi_sdu on host arrays or (device) on torch tensors, the type-1 tensor at an odd address;
    frag and outs are updated in place.  mixed: the names of SMALL passed as device tensors in a call
    whose other arrays are the host's.  Returns the return code."""
    from tetraear import _hip
    c = _hip.ctx()
    arrays = [None if a is None else np.ascontiguousarray(a) for a in call["arrays"]]
    nsym, keep = None if call["nsym"] is None else np.ascontiguousarray(call["nsym"], np.int32), call["keep"]
    C = call.get("C", len(call["arrays"][1]) if call["arrays"][0] is None else len(call["arrays"][0]))
    args = [nsym] + arrays + [keep] + outs[:2] + [None if frag is None else frag.view(np.uint8)] + outs[2:]
    if device:
        import torch
        dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args]
        odd = torch.zeros(arrays[4].size + 1, dtype=torch.uint8, device="cuda")
        odd[1:] = dev[5].reshape(-1)
        dev[5] = odd[1:]
        assert dev[5].data_ptr() % 2 == 1
        p = [_hip.ptr(a) for a in dev]
    else:
        p = [_hip.ptr(a) for a in args]
    if mixed:
        import torch
        held = {SMALL[k]: torch.from_numpy(np.ascontiguousarray(args[SMALL[k]])).cuda() for k in mixed}
        torch.cuda.synchronize()
        for i, t in held.items():
            p[i] = _hip.ptr(t)
    rc = c.lib.tetra_etsi_sdu(c.handle, p[0], C, call["G"], call["row_bits"], call["advance"], call["gap_slots"],
                              p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], call["maxd"],
                              p[12], p[13], p[14])
    if device:
        torch.cuda.synchronize()
        for host, d in zip(args[9:], dev[9:]):
            host[...] = d.cpu().numpy().reshape(host.shape)
    return rc


def check_call(call, frag, models, seed, device=False, what=""):
    """One call on the library and on the model (models: [Frag] per group, frag: their array so far)."""
    C, G = len(call["arrays"][0]), call["G"]
    outs = poisoned_outputs(seed, C, G, call["maxd"])
    before = [o.copy() for o in outs]
    recs, ndone, done = S.run(models, G, call["row_bits"], call["advance"], call["gap_slots"], call["maxd"],
                              call["nsym"], *call["arrays"], keep=call["keep"])
    assert call_sdu(call, frag, outs, device) == 0, what
    want = S.expected_arrays(recs, ndone, done, before[0], before[1], before[3], before[4])
    for name, got, exp in zip(("sdu", "sdu_data", "done", "done_data"), (outs[0], outs[1], outs[3], outs[4]), want):
        assert np.array_equal(got, exp), (what, name, np.argwhere(got != exp)[:4].tolist())
    assert outs[2].tolist() == ndone.tolist(), (what, "ndone")
    S.assert_frag_equal(frag, models, what)
    return outs, (recs, ndone, done)


def frag_array(models):
    a = np.zeros(len(models), S.FRAG_DTYPE)
    for i, m in enumerate(models):
        a[i] = m.to_array()
    return a


# ------------------------------------------------------------------------------ the scenarios, stacked

def stack(calls):
    """Calls of one row each (G = 1, the same gap_slots and maxd) as one call of len(calls) rows."""
    out = dict(calls[0])
    out["arrays"] = tuple(np.concatenate([c["arrays"][i] for c in calls]) for i in range(7))
    out["nsym"] = np.concatenate([c["nsym"] for c in calls])
    return out


def empty_call(rng, like):
    out = dict(like)
    out["arrays"] = S.build_rows(rng, [[]])
    return out


@functools.lru_cache(maxsize=None)
def stacked_scenarios():
    """17 rows: the edge scenarios with maxd 4 and two chains; (scenarios, [call of 17 rows])."""
    rng = np.random.default_rng(50)
    scs = [sc for sc, _ in K.edge_cases(rng) if sc.maxd == 4]
    for nfrag, step in ((8, 4), (4, 12)):
        sdu = K.payload(rng, K.sdu_len(rng, nfrag))
        scs.append(K.Scenario(f"chain {nfrag}", K.chain_bursts(rng, sdu, nfrag, 123, step * K.SLOT)))
    assert len(scs) == 17
    per = [sc.calls(rng) for sc in scs]
    calls = []
    for k in range(max(len(p) for p in per)):
        calls.append(stack([p[k] if k < len(p) else empty_call(rng, p[0]) for p in per]))
    return scs, calls


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_scenarios_equal_the_model(device):
    scs, calls = stacked_scenarios()
    models = [S.Frag(sc.bit0) for sc in scs]
    frag = frag_array(models)
    done = [[] for _ in scs]
    for k, call in enumerate(calls):
        _, (_, _, d) = check_call(call, frag, models, 700 + k, device, f"call {k}")
        for (g, i) in sorted(d):
            done[g].append(d[(g, i)][1])
    # the model's outcome here is the one tests/test_etsi_sdu_model.py holds it to
    exp = {sc.name: e for sc, e in K.edge_cases(np.random.default_rng(50))}
    for sc, got, m in zip(scs, done, models):
        if sc.name in exp:
            assert got == [S.pack(b) for b in exp[sc.name]["done"]], sc.name
            assert (m.dropped, m.orphans) == (exp[sc.name]["dropped"], exp[sc.name]["orphans"]), sc.name
        else:
            assert len(got) == 1, sc.name


def test_maxd_below_the_completions_one_row():
    rng = np.random.default_rng(50)
    sc = [sc for sc, _ in K.edge_cases(rng) if sc.maxd == 1][0]
    models = [S.Frag()]
    frag = frag_array(models)
    for k, call in enumerate(sc.calls(rng)):
        outs, _ = check_call(call, frag, models, 800 + k, what=sc.name)
        assert outs[2].tolist() == [2]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_groups_of_overlapping_rows(device):
    rng = np.random.default_rng(21)
    for sc, sdu in K.group_cases(rng):
        models = [S.Frag()]
        frag = frag_array(models)
        got = []
        for k, call in enumerate(sc.calls(rng)):
            outs, _ = check_call(call, frag, models, 900 + k, device, sc.name)
            got += [bytes(outs[4][0, i, :(int(outs[3][0, i, S.D_NBITS]) + 7) // 8]) for i in range(int(outs[2][0]))]
        assert got == [S.pack(sdu)], sc.name


def test_one_row_groups_equal_the_streaming_form():
    rng = np.random.default_rng(22)
    nfrag = 5
    sc = K.Scenario("stream", K.chain_bursts(rng, K.payload(rng, K.sdu_len(rng, nfrag)), nfrag, 700))
    ma, mb = [S.Frag()], [S.Frag()]
    fa, fb = frag_array(ma), frag_array(mb)
    for k, call in enumerate(sc.calls(rng)):
        a, _ = check_call(call, fa, ma, 1000 + k, what="streaming")
        other = dict(call, keep=np.ones((1, S.MAXB), np.int32), advance=2 * (int(call["nsym"][0]) - 1))
        b, _ = check_call(other, fb, mb, 1000 + k, what="keep")
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and fa.tobytes() == fb.tobytes()


@functools.lru_cache(maxsize=None)
def two_groups_call():
    """C = 6, G = 3, maxd = 4: two groups of three overlapping rows, a chain of three and of two fragments
    that both complete in the call (the model says so)."""
    rng = np.random.default_rng(77)
    per = []
    for nfrag, ssi in ((3, 0x111111), (2, 0x222222)):
        sdu = K.payload(rng, K.sdu_len(rng, nfrag))
        per.append(K.Scenario(f"G 3, {nfrag} fragments", K.chain_bursts(rng, sdu, nfrag, 300, ssi=ssi), G=3).calls(rng)[0])
    call = dict(per[0], nsym=np.concatenate([c["nsym"] for c in per]), keep=np.concatenate([c["keep"] for c in per]),
                arrays=tuple(np.concatenate([c["arrays"][i] for c in per]) for i in range(7)))
    assert (call["G"], call["maxd"], len(call["arrays"][0])) == (3, 4, 6)
    _, ndone, _ = S.run([S.Frag(), S.Frag()], 3, call["row_bits"], call["advance"], call["gap_slots"], 4, call["nsym"],
                        *call["arrays"], keep=call["keep"])
    assert ndone.tolist() == [1, 1]
    return call


def _run_two_groups(call, mixed=(), models=None):
    """Every output of one call from fresh fragment state, as bytes (models: one Frag a group; default two)."""
    frag = frag_array(models or [S.Frag(), S.Frag()])
    outs = poisoned_outputs(4400, len(call["arrays"][0]), call["G"], call["maxd"])
    assert call_sdu(call, frag, outs, mixed=mixed) == 0, mixed
    return [o.tobytes() for o in outs] + [frag.tobytes()]


@pytest.mark.parametrize("mixed", sorted(SMALL), ids=sorted(SMALL))
def test_one_small_array_on_the_device(mixed):
    """The small arrays share one staged input: with any one of them a device pointer the others still land at
    their own offsets, and every output is the all-host call's, byte for byte."""
    call = two_groups_call()
    assert _run_two_groups(call, (mixed,)) == _run_two_groups(call)


def test_small_arrays_without_keep_and_one_on_the_device():
    call = dict(two_groups_call(), keep=None)
    want = _run_two_groups(call)
    assert want != _run_two_groups(two_groups_call())   # (every copy feeds without keep: the call differs)
    assert _run_two_groups(call, ("nblock",)) == want and _run_two_groups(call, ("nsym", "npdu")) == want


def test_nsym_in_the_pack_of_the_streaming_form():
    """Only the streaming form (G = 1, row_bits 0, no keep) reads nsym, the pack's first part: the 17 stacked rows
    with nsym alone on the device, and with nsym alone on the host, against the all-host call."""
    scs, calls = stacked_scenarios()
    call = calls[0]
    assert (call["G"], call["row_bits"], call["keep"], call["maxd"]) == (1, 0, None, 4)
    models = [S.Frag(sc.bit0) for sc in scs]
    want = _run_two_groups(call, models=models)
    assert _run_two_groups(call, ("nsym",), models) == want
    assert _run_two_groups(call, ("nburst", "nblock", "npdu"), models) == want
    other = dict(call, nsym=call["nsym"] + 64)   # nsym is read: another chunk length moves the streams on otherwise
    assert _run_two_groups(other, ("nsym",), models) == _run_two_groups(other, models=models) != want


# ------------------------------------------------------------------------------ a seeded sweep

SWEEP = ((1, 1), (5, 1), (17, 1), (33, 1), (34, 2), (33, 3), (64, 64), (128, 64))


@pytest.mark.parametrize("C,G", SWEEP)
def test_seeded_sweep(C, G):
    nblocks = 0
    for seed in range(2 * SCALE):
        rng = np.random.default_rng(9100 + 100 * seed + C + G)
        models = [S.Frag(int(rng.integers(0, 1 << 45))) for _ in range(C // G)]
        frag = frag_array(models)
        for k in range(3):   # the state is carried
            arrays, keep = K.random_call(rng, C, G)
            call = dict(G=G, row_bits=0 if G == 1 else 4 * K.SLOT, advance=G * 4 * K.SLOT, gap_slots=int(rng.choice((0, 8, 72))),
                        maxd=int(rng.choice((0, 1, 3, 16))), nsym=np.full(C, 4 * K.SLOT + 1, np.int32), arrays=arrays,
                        keep=keep)
            check_call(call, frag, models, seed * 10 + k, device=bool((seed + k) & 1), what=f"seed {seed}, call {k}")
            nblocks += int(np.sum(arrays[5] > 0))
    assert nblocks >= (300 if C >= 17 else 1)


# ------------------------------------------------------------------------------ through the chain

SMAX = 2048
CELL = (262, 1017, 33)


def null_block(rng, kind):
    return M.block(rng, kind, [M.null_pdu()])


def planted_row(rng, nfrag, lead, first_slot=1, with_sb=True):
    """A row of consecutive bursts: an SB announcing CELL on slot 0, an SDU cut into nfrag SCH/F fragments
    four slots apart from first_slot on, null PDUs everywhere else.  Returns (bits, the SDU's bits)."""
    init = E.scramble_init(*CELL)
    sdu = K.payload(rng, K.sdu_len(rng, nfrag))
    pdus = S.fragment(sdu, [0] * nfrag, ssi=0xBEEF01)
    at = {first_slot + 4 * i: [pd] if i < nfrag - 1 else [pd, M.null_pdu()] for i, pd in enumerate(pdus)}
    items = []
    for b in range(first_slot + 4 * nfrag - 2):
        if b == 0 and with_sb:
            pay, kind = [M.block(rng, 2, [M.sync(M.sync_for_slot(rng, 40, CELL))]), null_block(rng, 1)], 2
        elif b in at:
            pay, kind = [M.block(rng, 0, at[b])], 0
        else:
            kind = int(rng.integers(0, 2))
            pay = [null_block(rng, k) for k in S.BLOCKS_OF[kind]]
        items.append((lead if b == 0 else 0, kind, init, pay))
    bits, _, _ = R.place_bursts(rng, items, tail_gap=40)
    return bits, sdu


def in_burst_row(seed):
    """R.burst_stream (random gaps between its bursts) with a chain inside one burst: SCH/HD block 1 starts,
    block 2 ends, which no gap can part."""
    rng = np.random.default_rng(seed)
    h1, h2 = K.payload(rng, 124 - 43), K.payload(rng, int(rng.integers(0, 100)))
    pays = [[null_block(rng, 0)], [M.block(rng, 1, K.first(h1, ssi=0xBEEF02, n1=124)), M.block(rng, 1, K.last(h2, n1=124))],
            [null_block(rng, 0)]]
    bits, _, _, _ = R.burst_stream(seed, cell_init=E.scramble_init(*CELL), kinds=[0, 1, 0], payloads=pays)
    return bits, h1 + h2


@functools.lru_cache(maxsize=None)
def chain_rows():
    rows = [planted_row(np.random.default_rng(600 + i), nfrag, 7 + 2 * i) for i, nfrag in enumerate((2, 3, 4))]
    rows += [in_burst_row(610), in_burst_row(611)]
    return rows


def run_chain(cut_seed):
    """tetra_lmac_etsi_stream -> tetra_etsi_mac -> tetra_etsi_sdu chunk by chunk on host arrays, the cell
    known from the start; per row the completed messages [(fields, bytes)] and the final frag array."""
    from tetraear import _hip
    c = _hip.ctx()
    rows = chain_rows()
    C, RES = len(rows), _hip.ETSI_RESERVE
    chans = [(R.hard_of(b), R.soft_of(b), R.chunk_cuts(cut_seed + i, len(b) // 2, (255, 256, 257, 700, 1500, 1790)))
             for i, (b, _) in enumerate(rows)]
    soft, hard = np.zeros((C, 2 * SMAX), np.int8), np.zeros((C, SMAX), np.uint8)
    lead = np.full(C, 2 * RES, np.int32)
    cell_init = np.full(C, E.scramble_init(*CELL), np.uint32)
    tdma, frag = np.zeros(C, _hip.ETSI_TDMA), np.zeros(C, _hip.ETSI_FRAG)
    got = [[] for _ in rows]
    p = _hip.ptr
    for k in range(max(len(ch[2]) for ch in chans) + 1):
        nsym = np.ones(C, np.int32)
        hard[:, RES:], soft[:, 2 * RES:] = 0, 0
        for ch, (h, s, cuts) in enumerate(chans):
            at, n = cuts[k] if k < len(cuts) else (len(h), 0)
            hard[ch, RES:RES + n], soft[ch, 2 * RES:2 * RES + 2 * n] = h[at:at + n], s[2 * at:2 * (at + n)]
            nsym[ch] = n + 1
        o = R.lmac_outputs(C)
        slots, npdu = np.zeros((C, M.MAXB, 4), np.int32), np.zeros((C, M.MAXJ), np.int32)
        pdus = np.zeros((C, M.MAXJ, M.MAXPDU, M.NF), np.int32)
        c.check(c.lib.tetra_lmac_etsi_stream(c.handle, p(soft), p(hard), p(nsym), C, SMAX, p(lead), p(soft), p(hard),
                                             p(cell_init), p(o["nburst"]), p(o["bursts"]), p(o["nblock"]), p(o["blocks"]),
                                             p(o["type1"])), "tetra_lmac_etsi_stream")
        c.check(c.lib.tetra_etsi_mac(c.handle, p(nsym), C, p(o["nburst"]), p(o["bursts"]), p(o["nblock"]), p(o["blocks"]),
                                     p(o["type1"]), p(tdma), p(slots), p(npdu), p(pdus)), "tetra_etsi_mac")
        outs = poisoned_outputs(k, C, 1, 4)
        call = dict(G=1, row_bits=0, advance=0, gap_slots=S.GAP_DEFAULT, maxd=4, nsym=nsym, keep=None,
                    arrays=(o["nburst"], o["bursts"], o["nblock"], o["blocks"], o["type1"], npdu, pdus))
        assert call_sdu(call, frag, outs) == 0
        for ch in range(C):
            for i in range(int(outs[2][ch])):
                f = outs[3][ch, i].tolist()
                got[ch].append((f, bytes(outs[4][ch, i, :(f[S.D_NBITS] + 7) // 8])))
    return got, frag


@pytest.mark.parametrize("cut_seed", [1, 20, 300])
def test_planted_sdu_comes_back_whatever_the_cuts(cut_seed):
    got, frag = run_chain(cut_seed)
    for ch, ((_, sdu), msgs) in enumerate(zip(chain_rows(), got)):
        assert [d for _, d in msgs] == [S.pack(sdu)], (cut_seed, ch)
        f = msgs[0][0]
        assert f[S.D_NBITS] == len(sdu) and f[S.D_GAPS] == 0 and f[S.D_SSI] == (0xBEEF01 if ch < 3 else 0xBEEF02)
        assert f[S.D_NFRAG] == ((2, 3, 4)[ch] if ch < 3 else 2)
    assert not frag["dropped"].any() and not frag["orphans"].any() and not frag["chain"]["active"].any()


# ------------------------------------------------------------------------------ the Python surfaces

def stream_frames(lm, cut_seed=5):
    rows = chain_rows()[:3]
    C = len(rows)
    chans = [(R.hard_of(b), R.soft_of(b), R.chunk_cuts(cut_seed + i, len(b) // 2, (700, 1500, 1790)))
             for i, (b, _) in enumerate(rows)]
    frames = [[] for _ in rows]
    for k in range(max(len(ch[2]) for ch in chans) + 1):
        n = [ch[2][k][1] if k < len(ch[2]) else 0 for ch in chans]
        smax = max(max(n), 1) + 2
        hard, soft, nsym = np.zeros((C, smax), np.uint8), np.zeros((C, 2 * smax), np.int8), np.ones(C, np.int32)
        for ch, (h, s, cuts) in enumerate(chans):
            at = cuts[k][0] if k < len(cuts) else len(h)
            hard[ch, :n[ch]], soft[ch, :2 * n[ch]], nsym[ch] = h[at:at + n[ch]], s[2 * at:2 * (at + n[ch])], n[ch] + 1
        for ch, fr in enumerate(lm.decode_stream(soft, hard, nsym)):
            frames[ch] += fr
    return frames


PDU_KEYS = {"sdu", "sdu_bits", "sdu_status", "role", "power_control", "slot_granting", "channel_allocation"}


def strip(frames):
    """The frames without the keys sdu=True adds."""
    out = []
    for f in frames:
        g = {k: v for k, v in f.items() if k not in ("sdus", "blocks")}
        g["blocks"] = [{k: ([{a: b for a, b in p.items() if a not in PDU_KEYS} for p in v] if k == "pdus" else
                            v.tolist() if k == "bits" else v) for k, v in blk.items()} for blk in f["blocks"]]
        out.append(g)
    return out


def test_lower_mac_frames_and_messages():
    from tetraear.core.etsi import EtsiLowerMac, messages
    cell = dict(zip(("mcc", "mnc", "colour_code"), CELL))
    plain = stream_frames(EtsiLowerMac(mac=True, **cell))
    lm = EtsiLowerMac(mac=True, sdu=True, **cell)
    full = stream_frames(lm)
    assert not any("sdus" in f or any("sdu" in p for b in f["blocks"] for p in b["pdus"]) for fr in plain for f in fr)
    for ch, ((_, sdu), a, b) in enumerate(zip(chain_rows(), plain, full)):
        assert strip(b) == strip(a) and len(a) >= 4
        assert all({"sdu", "sdu_bits", "sdu_status", "role"} <= set(p) for f in b for blk in f["blocks"] for p in blk["pdus"])
        msgs = messages(b)
        assert [(m["data"], m["nbits"], m["ssi"], m["fragments"], m["gaps"]) for m in msgs] == \
            [(S.pack(sdu), len(sdu), 0xBEEF01, (2, 3, 4)[ch], 0)]
        assert msgs[0]["tn"] is not None and msgs[0]["span_slots"] == 4 * ((2, 3, 4)[ch] - 1)
        ends = [f for f in b if "sdus" in f]
        assert len(ends) == 1 and set(ends[0]["sdus"][0]) >= {"ssi", "address_type", "aux", "enc", "nbits", "data",
                                                              "fragments", "span_slots", "gaps"}
    st = lm.frag_stats
    assert st["dropped"].tolist() == [0, 0, 0] and st["orphans"].tolist() == [0, 0, 0] and st["lost"].tolist() == [0, 0, 0]
    lm.reset_stream()
    assert lm._frag is None


def test_decoder_hands_the_sdus_to_upper_mac():
    from tetraear.core import TetraDecoder

    class Recorder(TetraDecoder):
        def upper_mac(self, frame, burst, mac_pdu=None):
            self.seen.append(mac_pdu)
            return frame

    bits, sdu = chain_rows()[0]   # two fragments behind an SB: one decode_batch row holds them
    hard, soft, nsym = R.pack_rows([(bits, R.soft_of(bits))], len(bits) // 2 + 2)
    cells = np.array([E.scramble_init(*CELL)], np.uint32)
    on, off = (Recorder(auto_decrypt=False, mode="etsi", mac=True, sdu=s) for s in (True, False))
    plain = TetraDecoder(auto_decrypt=False, mode="etsi", mac=True)
    on.seen, off.seen = [], []
    a = on._etsi_frames(on._etsi_rx().decode_batch(soft, hard, nsym, cells=cells)[0])
    b = off._etsi_frames(off._etsi_rx().decode_batch(soft, hard, nsym, cells=cells)[0])
    ref = plain._etsi_frames(plain._etsi_rx().decode_batch(soft, hard, nsym, cells=cells)[0])
    assert [f["position"] for f in b] == [f["position"] for f in ref]   # sdu=False: today's frames
    assert all(set(f) == set(g) and f["mac_pdus"] == g["mac_pdus"] for f, g in zip(b, ref))
    joined = [p for p in on.seen if p is not None and p.pdu_type.name == "MAC_END"]
    assert len(joined) == 1 and joined[0].reassembled_data == S.pack(sdu)
    first = [p for p in on.seen if p is not None and p.pdu_type.name == "MAC_RESOURCE" and p.length == 63]
    assert len(first) == 1 and first[0].address == 0xBEEF01 and first[0].reassembled_data == b""
    assert first[0].data == S.pack(sdu[:K.FIRST_CAP])
    ends = [f for f in a if "sdus" in f]
    assert len(ends) == 1 and ends[0]["mac_pdus"][0]["role"] == 3 and ends[0]["mac_pdus"][0]["sdu_bits"] > 0


# the wideband chain: one capture of seven slots (the existing traffic tests' six lose the first burst to
# the filter bank's start and the last to the capture's end), two carriers with a two-fragment message each
# on slots 1 and 5, the cells given
NW = 2_000_000
WB_CARRIERS = (130, 401)
WB_LEAD = (0, 100)


@pytest.fixture(scope="module")
def capture():
    import wideband as W
    d = W.design()
    nbb = NW // d["D"] + 1
    s = np.zeros((d["M"], nbb), np.complex128)
    cells = np.full(d["M"], 3, np.uint32)
    sdus = {}
    for i, k in enumerate(WB_CARRIERS):
        rng = np.random.default_rng(970 + i)
        cells[k] = E.scramble_init(*CELL)
        bits, sdus[k] = planted_row(rng, 2, WB_LEAD[i], first_slot=1, with_sb=False)
        s[k] = E.modulate(bits, nbb, fs=d["fs"] / d["D"], t0=0.1 + 0.13 * i, phase0=0.7 * i, cfo=(-40.0, 25.0)[i])
    return W.synthesize(s, d, NW).astype(np.complex64), cells, sdus


def test_wideband_decode_and_stream(capture):
    from tetraear.core.etsi import messages
    from tetraear.signal.wideband import WidebandReceiver, WidebandStream
    x, cells, sdus = capture
    rx = WidebandReceiver()
    with pytest.raises(ValueError):
        rx.decode(x[:1000], cells, sdu=True)
    with pytest.raises(ValueError):
        rx.decode(x[:1000], cells, mac=True, sdu=True)
    with pytest.raises(ValueError):
        WidebandStream(cells, mac=True, sdu=True)
    with pytest.raises(ValueError):
        rx.decode_acquire(x[:1000], np.full(len(cells), 3, np.uint32), mac=True, sdu=True)
    plain = rx.decode(x, cells, mac=True, timebase="vote")
    full = rx.decode(x, cells, mac=True, timebase="vote", sdu=True)
    for k in WB_CARRIERS:
        assert strip(full[k]) == strip(plain[k]) and len(plain[k]) >= 4, [f["sample"] for f in plain[k]]
        got = [m for m in messages(full[k]) if m["fragments"] > 1]
        assert [(m["data"], m["nbits"], m["gaps"]) for m in got] == [(S.pack(sdus[k]), len(sdus[k]), 0)], \
            (k, [(f["sample"], [p["kind"] for b in f["blocks"] for p in b["pdus"]]) for f in full[k]], rx.frag_stats["orphans"][k])
    assert rx.frag_stats["orphans"].sum() == 0 and rx.frag_stats["lost"].sum() == 0
    # the cells handed in as acquired before the capture (its rows hold no SB): the same messages
    known = rx.decode_acquire(x, cells, mac=True, timebase="vote", sdu=True)[0]
    for k in WB_CARRIERS:
        assert len(known[k]) == len(plain[k])
        assert [m["data"] for m in messages(known[k]) if m["fragments"] > 1] == [S.pack(sdus[k])], k
    st = WidebandStream(cells, mac=True, timebase="vote", sdu=True)
    frames = [[] for _ in cells]
    for a, b in ((0, 611_111), (611_111, 700_001), (700_001, NW)):
        for k, fr in enumerate(st.decode(x[a:b])):
            frames[k] += fr
    for k in WB_CARRIERS:   # once, though the carried tails are decoded twice
        got = [m for m in messages(frames[k]) if m["fragments"] > 1]
        assert [(m["data"], m["gaps"]) for m in got] == [(S.pack(sdus[k]), 0)], k
    assert st.frag_stats["orphans"].sum() == 0 and st.frag_stats["dropped"].sum() == 0
    assert st.frag_stats["lost"].sum() == 0


# ------------------------------------------------------------------------------ argument checks

def test_invalid_arguments_write_nothing():
    rng = np.random.default_rng(1)
    arrays, _ = K.random_call(rng, 6, 1)
    good = dict(G=1, row_bits=0, advance=0, gap_slots=72, maxd=2, nsym=np.full(6, 2041, np.int32), arrays=arrays, keep=None)
    bad = [dict(good, G=0), dict(good, G=4), dict(good, G=65), dict(good, row_bits=-1, G=2), dict(good, gap_slots=-1),
           dict(good, maxd=-1), dict(good, nsym=None), dict(good, C=0), dict(good, C=(1 << 24) + 1)]
    bad += [dict(good, arrays=tuple(None if i == j else a for i, a in enumerate(arrays))) for j in range(7)]
    for call in bad:
        frag = np.zeros(6, S.FRAG_DTYPE)
        frag["bit0"] = 5
        outs = poisoned_outputs(3, 6, 1, 2)
        before = [o.copy() for o in outs]
        assert call_sdu(call, frag, outs) == INVALID, {k: v for k, v in call.items() if k not in ("arrays", "nsym")}
        assert all(np.array_equal(x, y) for x, y in zip(outs, before)) and (frag["bit0"] == 5).all()
    for j in range(5):   # a NULL output
        frag = np.zeros(6, S.FRAG_DTYPE)
        outs = poisoned_outputs(3, 6, 1, 2)
        before = [o.copy() for o in outs]
        outs[j] = None
        assert call_sdu(good, frag, outs) == INVALID, j
        assert all(x is None or np.array_equal(x, y) for x, y in zip(outs, before)) and not frag["bit0"].any()
    outs = poisoned_outputs(3, 6, 1, 2)
    assert call_sdu(good, None, outs) == INVALID
    # maxd == 0 needs no done arrays; a good call after the refusals
    frag, outs = np.zeros(6, S.FRAG_DTYPE), poisoned_outputs(3, 6, 1, 0)
    outs[3] = outs[4] = None
    assert call_sdu(dict(good, maxd=0), frag, outs) == 0 and (frag["bit0"] == 4080).all() and (outs[2] >= 0).all()
