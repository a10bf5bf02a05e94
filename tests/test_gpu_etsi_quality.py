"""tetra_etsi_link_quality (k_etsi_quality) against tests/_etsi_quality_model.py: every record equal to
the model's, integer for integer, on rows built on the CPU, on streaming and grouped rows, on the
smallest real chain and on a seeded sweep; then the Python surface.  No tolerance anywhere.
tests/test_etsi_quality_model.py proves on the CPU that the built rows mean what is assumed here."""
import functools
import itertools
import os

import numpy as np
import pytest

import etsi as E
import _etsi_quality_model as Q
import _lmac_groups as LG
import _lmac_rows as R

pytestmark = pytest.mark.gpu

N, P, SB = R.NDB_N, R.NDB_P, R.SB
SCALE = int(os.environ.get("TETRA_FUZZ_SCALE", "1"))
GUARD = 4096   # poison bytes either side of the rows: a stray read would change a sum


def guarded(a, fill):
    """A copy of `a` with GUARD bytes of `fill` in front of and behind it in one buffer."""
    buf = np.full(a.size + 2 * GUARD, fill, a.dtype)
    v = buf[GUARD:GUARD + a.size].reshape(a.shape)
    v[...] = a
    return v


def poison_unwritten(o):
    """Poison what the lower MAC did not write: type-1 bytes past n1, records past the counts."""
    o = {k: v.copy() for k, v in o.items()}
    for c in range(len(o["nburst"])):
        nb, nk = int(o["nburst"][c]), int(o["nblock"][c])
        o["bursts"][c, nb:] = Q.POISON
        o["blocks"][c, nk:] = Q.POISON
        o["type1"][c, nk:] = 0xA5
        for j in range(nk):
            o["type1"][c, j, Q.N1_OF[int(o["blocks"][c, j, 0])]:] = 0xA5
    return o


def check(soft, hard, origin, G, cells, o, what="", device=False):
    """The call against the model on the same inputs, outputs poisoned first: (bq, kq)."""
    from tetraear import _hip
    want = Q.link_quality(soft, hard, origin, G, cells, o["nburst"], o["bursts"], o["nblock"], o["blocks"], o["type1"])
    rc, bq, kq = Q.call(soft, hard, origin, G, cells, o, device=device)
    _hip.ctx().check(rc, "tetra_etsi_link_quality")
    assert np.array_equal(bq, want[0]), (what, np.argwhere(bq != want[0])[:4].tolist())
    assert np.array_equal(kq, want[1]), (what, np.argwhere(kq != want[1])[:4].tolist())
    return bq, kq


# ------------------------------------------------------------------------------ 1. built rows

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_built_rows_equal_the_model(device):
    d = Q.built_rows()
    C = len(d["nsym"])
    for lo in range(0, C, 8):   # at most 8 rows a call
        sl = slice(lo, min(lo + 8, C))
        hard, soft = guarded(d["hard"][sl], 0xFF), guarded(d["soft"][sl], 127)
        o = R.run_lmac(hard, soft, d["nsym"][sl], d["cells"][sl])
        R.assert_rows_equal(o, R.oracle_rows(hard, soft, d["nsym"][sl], d["cells"][sl]), "built rows")
        bq, kq = check(soft, hard, 0, 1, d["cells"][sl], poison_unwritten(o), "built rows", device)
        for c in range(sl.stop - lo):
            assert (bq[c, o["nburst"][c]:] == Q.POISON).all() and (kq[c, o["nblock"][c]:] == Q.POISON).all()
        for r, what, i, f, v in d["expect"]:
            if lo <= r < sl.stop:
                assert int((bq if what == "b" else kq)[r - lo, i, f]) == v, (r, what, i, f, v)


# ------------------------------------------------------------------------------ 2. records that read -1

def test_crc_bad_blocks_and_invalid_bursts():
    d = Q.built_rows()
    hard, soft = guarded(d["hard"][:6], 0xFF), guarded(d["soft"][:6], 127)
    stride = hard.shape[1]
    # row 0 (clean, bursts N SB P): the SCH/F block's first half inverted breaks its CRC
    s = d["planted"][0][0][0]
    soft[0, s + 14:s + 230] = -soft[0, s + 14:s + 230]
    o = R.run_lmac(hard, soft, d["nsym"][:6], d["cells"][:6])
    assert o["blocks"][0, 0].tolist() == [0, 0, 0, 0]
    o = poison_unwritten(o)
    o["bursts"][1, 0, 0] = 2 * stride - 509   # one bit past the row's end
    o["bursts"][2, 1, 0] = -1                 # before the row
    o["bursts"][3, 2, 1] = 7
    o["bursts"][4, 0, 1] = -1
    o["bursts"][5, 0, 0] = 2 * stride - 510   # the last start inside the row: read (zeros and the built row's end)
    bq, kq = check(soft, hard, 0, 1, d["cells"][:6], o, "invalid")
    assert kq[0, 0].tolist() == [-1, 0, 0, 0]
    for c, b in ((1, 0), (2, 1), (3, 2), (4, 0)):
        assert bq[c, b].tolist() == [-1] * 4
        js = [j for j in range(o["nblock"][c]) if o["blocks"][c, j, 2] == b]
        assert js and all(kq[c, j].tolist() == [-1] * 4 for j in js), (c, b)
    assert (bq[5, 0] >= 0).all()


# ------------------------------------------------------------------------------ 3. error returns

def test_error_returns_write_nothing():
    from tetraear import _hip
    d = Q.built_rows()
    hard, soft, cells = d["hard"][:6], d["soft"][:6], d["cells"][:6]
    o = R.run_lmac(hard, soft, d["nsym"][:6], cells)
    c = _hip.ctx()
    C, stride = hard.shape
    for name, kw in (("cell_init NULL", dict(ci=None)), ("G 0", dict(G=0)), ("C % G", dict(G=4)), ("C 0", dict(C=0)),
                     ("origin < 0", dict(origin=-2)), ("bq NULL", dict(bq=None))):
        a = dict(C=C, G=1, origin=0, ci=cells.copy())
        bq, kq = np.full((C, 8, 4), Q.POISON, np.int32), np.full((C, 16, 4), Q.POISON, np.int32)
        a["bq"] = bq
        a.update(kw)
        rc = c.lib.tetra_etsi_link_quality(c.handle, _hip.ptr(soft), _hip.ptr(hard), a["C"], stride, a["origin"],
                                           a["G"], _hip.ptr(a["ci"]), _hip.ptr(o["nburst"]), _hip.ptr(o["bursts"]),
                                           _hip.ptr(o["nblock"]), _hip.ptr(o["blocks"]), _hip.ptr(o["type1"]),
                                           _hip.ptr(a["bq"]), _hip.ptr(kq))
        assert rc == -1, (name, rc)
        assert (bq == Q.POISON).all() and (kq == Q.POISON).all(), name
    rc, bq, kq = Q.call(soft, hard, 0, 3, cells[:2], o)   # and the same call with whole groups is taken
    assert rc == 0 and (kq[:, 0] != Q.POISON).all()


# ------------------------------------------------------------------------------ 4. streaming rows

def _noisy_soft(rng, bits):
    """Soft bits of random strength, a few of them zero and a few of the wrong sign."""
    s = R.soft_of(bits, 1).astype(np.int16) * rng.integers(24, 128, len(bits))
    s[rng.random(len(bits)) < 0.01] = 0
    wrong = rng.random(len(bits)) < 0.006
    s[wrong] = -s[wrong]
    return s.astype(np.int8)


def test_stream_rows_alternate_and_read_the_whole_stream():
    """Three chunks through tetra_lmac_etsi_stream into alternate rows, a burst across each seam: the
    records of every burst, with origin_bits = 2 RESERVE, equal the model on the whole stream."""
    from tetraear import _hip
    c = _hip.ctx()
    RES = _hip.ETSI_RESERVE
    rng = np.random.default_rng(404)
    C, chans = 3, []
    for ch in range(C):
        cell = R.random_cell(rng)
        kinds = [(N, SB, P, N, P, SB), (P, N, SB, SB, N, P), (SB, P, N, P, SB, N)][ch]
        bits, planted, _ = R.place_bursts(rng, [(int(rng.integers(0, 40)), k, cell, None) for k in kinds], 30)
        hard = R.hard_of(bits)
        # seams inside burst 1's first block and burst 3's training sequence
        cuts = R.cuts_at(len(hard), [(planted[1][0] + 120) // 2, (planted[3][0] + 250) // 2])
        chans.append((bits, hard, _noisy_soft(rng, bits), cuts, cell, planted))
    cells = np.array([ch[4] for ch in chans], np.uint32)
    stride = RES + max(n for ch in chans for _, n in ch[3]) + 3
    assert stride <= 2050
    bufs = [(np.zeros((C, 2 * stride), np.int8), np.zeros((C, stride), np.uint8)) for _ in range(2)]
    lead = np.full(C, 2 * RES, np.int32)
    c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(cells), C), "tetra_etsi_set_cells")
    found, negative = [[] for _ in chans], 0
    for k in range(3):
        soft, hard = bufs[k % 2]
        nsoft, nhard = bufs[(k + 1) % 2]
        nsym = np.ones(C, np.int32)
        at0 = []
        for ch, (_, h, s, cuts, _, _) in enumerate(chans):
            at, n = cuts[k]
            hard[ch, RES:RES + n] = h[at:at + n]
            soft[ch, 2 * RES:2 * (RES + n)] = s[2 * at:2 * (at + n)]
            nsym[ch] = n + 1
            at0.append(at)

        def stream(sr, hr, ld, ns_, nh_):
            o = R.lmac_outputs(C)
            c.check(c.lib.tetra_lmac_etsi_stream(c.handle, _hip.ptr(sr), _hip.ptr(hr), _hip.ptr(nsym), C, stride,
                                                 _hip.ptr(ld), _hip.ptr(ns_), _hip.ptr(nh_), None, _hip.ptr(o["nburst"]),
                                                 _hip.ptr(o["bursts"]), _hip.ptr(o["nblock"]), _hip.ptr(o["blocks"]),
                                                 _hip.ptr(o["type1"])), "tetra_lmac_etsi_stream")
            return o

        if k == 0:   # what alternate rows rule out: streamed in place, the rows are not those the call read
            s2, h2, l2 = soft.copy(), hard.copy(), lead.copy()
            stream(s2, h2, l2, s2, h2)
            assert not np.array_equal(s2[:, :2 * RES], soft[:, :2 * RES])
        read = (soft.copy(), hard.copy())
        o = stream(soft, hard, lead, nsoft, nhard)
        assert np.array_equal(soft, read[0]) and np.array_equal(hard, read[1])   # intact for the quality pass
        rc, bq, kq = Q.call(soft, hard, 2 * RES, 1, cells, o)
        c.check(rc, "tetra_etsi_link_quality")
        for ch, (_, h_all, s_all, _, cell, _) in enumerate(chans):   # the same bursts in the whole stream
            one = {key: v[ch:ch + 1].copy() for key, v in o.items()}
            one["bursts"][0, :, 0] += 2 * at0[ch]
            want = Q.link_quality(s_all[None, :], h_all[None, :], 0, 1, cells[ch:ch + 1], one["nburst"], one["bursts"],
                                  one["nblock"], one["blocks"], one["type1"])
            assert np.array_equal(bq[ch], want[0][0]) and np.array_equal(kq[ch], want[1][0]), (k, ch)
            nb = int(o["nburst"][ch])
            assert (bq[ch, :nb] >= 0).all()
            negative += int((o["bursts"][ch, :nb, 0] < 0).sum())
            found[ch] += [(int(s) + 2 * at0[ch], int(kd)) for s, kd in o["bursts"][ch, :nb]]
    assert found == [ch[5] for ch in chans]
    assert negative >= 2 * C   # a burst across each seam began in the carried tail


# ------------------------------------------------------------------------------ 5. groups

@functools.lru_cache(maxsize=None)
def _two_groups():
    """C = 6 rows in G = 3 groups through tetra_lmac_etsi_acquire_groups: (hard, soft, the lower MAC's outputs,
    the cells after the call, the cells A and B the rows were built with)."""
    rng = np.random.default_rng(55)
    rows, _, A = LG.case_sync_in_row(rng, 2)   # the only SB in the group's last row
    B, _ = R.cell_fields(rng)
    rows += [LG.row(rng, [(4 + r, N, B, None), (2, P, B, None)], 2 * r) for r in range(3)]   # no SB: nothing acquired
    hard, soft, nsym = LG.pack(rows)
    out, want, after, good = LG.check_groups(hard, soft, nsym, 3, [3, 3], "quality groups")
    assert after == [A, 3] and good == [1, 0]
    return hard, soft, out, after, A, B


def test_groups_are_scored_with_the_acquired_cell():
    hard, soft, out, after, A, B = _two_groups()
    bq, kq = check(soft, hard, 0, 3, np.array(after, np.uint32), poison_unwritten(out), "groups")
    for ch in range(6):
        for j in range(int(out["nblock"][ch])):
            if ch < 3:   # rows 0 and 1 carry no SB: scored with the cell row 2 announced
                assert out["blocks"][ch, j, 1] == 1 and kq[ch, j, :2].tolist() == [0, 0], (ch, j)
            else:
                assert kq[ch, j].tolist() == [-1, 0, 0, 0], (ch, j)
    # the cell is the call's argument, not the context's table: another cell reads errors on the same rows
    _, _, kq2 = Q.call(soft, hard, 0, 3, np.array([B, 3], np.uint32), out)
    assert kq2[0, 0, Q.NERR] > 50


@pytest.mark.parametrize("on_device", list(itertools.product((False, True), repeat=3)),
                         ids=lambda c: "".join("dh"[not d] for d in c))
def test_small_arrays_host_and_device_mixed(on_device):
    """cell_init, nburst and nblock share one staged input: with any of them a device pointer and the rest the
    host's, both outputs are the all-host call's byte for byte (all three on the device: no staged pack)."""
    import torch
    from tetraear import _hip
    hard, soft, out, after, _, _ = _two_groups()
    o = poison_unwritten(out)
    rc, bq, kq = Q.call(soft, hard, 0, 3, np.array(after, np.uint32), o)
    assert rc == 0 and (kq[:3, 0, Q.NERR] == 0).all()
    small = [np.array(after, np.uint32).view(np.int32), o["nburst"], o["nblock"]]
    held = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if d else a for a, d in zip(small, on_device)]
    torch.cuda.synchronize()
    gb, gk = np.full_like(bq, Q.POISON), np.full_like(kq, Q.POISON)
    c = _hip.ctx()
    p = [_hip.ptr(a) for a in (soft, hard, held[0], held[1], o["bursts"], held[2], o["blocks"], o["type1"], gb, gk)]
    c.check(c.lib.tetra_etsi_link_quality(c.handle, p[0], p[1], 6, hard.shape[1], 0, 3, *p[2:]), str(on_device))
    assert gb.tobytes() == bq.tobytes() and gk.tobytes() == kq.tobytes()


# ------------------------------------------------------------------------------ 6. the smallest real chain

@functools.lru_cache(maxsize=None)
def _chain(snr_db):
    """tetra_synth_etsi at C = 5, N = 131072 -> tetra_demod_etsi -> tetra_lmac_etsi_acquire -> quality."""
    from tetraear.signal import etsi
    iq, cells, kinds, payload, _ = etsi.synth(5, 131072, seed=23, snr_db=snr_db)
    hard, soft, _, ns = etsi.EtsiReceiver().demod_batch(iq)
    state = np.full(5, 3, np.uint32)
    o = R.run_lmac(hard, soft, ns, cell_init=state)
    bq, kq = check(soft, hard, 0, 1, state, poison_unwritten(o), "chain %s" % snr_db)
    return dict(soft=soft, hard=hard, cells=cells, payload=payload, state=state, o=o, bq=bq, kq=kq)


def _good(d):
    return [(c, j) for c in range(5) for j in range(int(d["o"]["nblock"][c])) if d["o"]["blocks"][c, j, 1]]


def test_chain_without_noise_reads_no_errors():
    d = _chain(1000.0)
    good = _good(d)
    assert len(good) >= 3 and int(d["o"]["nburst"].sum()) >= 10
    assert all(d["kq"][c, j, Q.NERR] == 0 and d["kq"][c, j, Q.WERR] == 0 for c, j in good)
    for c in range(5):
        nb = int(d["o"]["nburst"][c])
        assert (d["bq"][c, :nb, :2] == 0).all() and (d["bq"][c, :nb, Q.BWSUM] > 0).all(), c


def test_chain_with_noise_counts_against_the_transmitted_code_word():
    quiet, loud = _chain(14.0), _chain(9.0)
    for d in (quiet, loud):
        o, checked = d["o"], 0
        for c, j in _good(d):
            kind, _, b, blk = (int(v) for v in o["blocks"][c, j])
            n1 = Q.N1_OF[kind]
            sent = [p for p in d["payload"][c, :, blk, :n1] if np.array_equal(p, o["type1"][c, j, :n1])]
            if not sent or (kind != 2 and d["state"][c] != d["cells"][c]):
                continue
            tx = Q.type5(sent[0], kind, 3 if kind == 2 else int(d["cells"][c]))   # the synthesiser's cell
            p = int(o["bursts"][c, b, 0]) + Q.block_offsets(kind, blk)
            assert d["kq"][c, j].tolist() == Q.score(d["soft"][c, p], tx), (c, j)
            checked += 1
        assert checked >= 1
    totals = [int(sum(d["kq"][c, j, Q.NERR] for c, j in _good(d))) for d in (quiet, loud)]
    print("summed NERR at 14 dB and 9 dB:", totals, "CRC-good blocks:", len(_good(quiet)), len(_good(loud)))
    assert totals[1] >= totals[0]


# ------------------------------------------------------------------------------ 7. seeded sweep

def _offset_tensor(a, off):
    """A device copy of `a` that starts `off` bytes past an allocation's (aligned) start."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(raw.size + 8, dtype=torch.uint8, device="cuda:0")
    buf[off:off + raw.size] = torch.from_numpy(raw).to("cuda:0")
    return buf, buf[off:off + raw.size]


@pytest.mark.parametrize("seed", range(20 * SCALE))
def test_random_rows_vs_model(seed):
    """Random C in 1..9, G dividing C, origin, burst placements, soft-bit classes, flips and zeros,
    CRC flags cleared and bursts made invalid; odd seeds on device copies whose type-1 and row
    pointers are not dword aligned."""
    from tetraear import _hip
    rng = np.random.default_rng(9000 + seed)
    C = int(rng.integers(1, 10))
    G = int(rng.choice([g for g in range(1, C + 1) if C % g == 0]))
    cells = np.array([R.random_cell(rng) for _ in range(C // G)], np.uint32)
    rows = []
    for ch in range(C):
        kinds = [int(k) for k in rng.integers(0, 3, int(rng.integers(0, 5)))]
        bits, planted, _ = R.place_bursts(rng, [(int(rng.choice(R.GAPS)), k, int(cells[ch // G]), None) for k in kinds],
                                          int(rng.integers(0, 9)))
        soft = _noisy_soft(rng, bits) if rng.random() < 0.7 else R.soft_class("gauss", bits, rng, 1)
        if planted and rng.random() < 0.3:
            s = planted[0][0]
            soft[s:s + 510] = R.soft_class(str(rng.choice(["m128", "uniform", "zero", "tern"])), bits[s:s + 510], rng)
        rows.append((bits, soft))
    smax = max(len(b) for b, _ in rows) // 2 + 1 + int(rng.integers(0, 4))
    hard, soft, nsym = R.pack_rows(rows, smax)
    o = R.run_lmac(hard, soft, nsym, np.repeat(cells, G))
    o = poison_unwritten(o)
    # the rows `origin` bits to the right, behind random bits
    origin = int(rng.integers(0, 40))
    pad = origin + (origin & 1)
    hb = np.stack([E.Receiver.hard_bits(h) for h in hard])
    hb = np.concatenate([rng.integers(0, 2, (C, origin)).astype(np.uint8), hb, np.zeros((C, pad - origin), np.uint8)], 1)
    hard = np.stack([R.hard_of(b) for b in hb])
    soft = np.concatenate([rng.integers(-128, 128, (C, origin)).astype(np.int8), soft,
                           np.zeros((C, pad - origin), np.int8)], 1)
    for ch in range(C):   # records the lower MAC would not write
        nb, nk = int(o["nburst"][ch]), int(o["nblock"][ch])
        if nk and rng.random() < 0.3:
            o["blocks"][ch, int(rng.integers(0, nk)), 1] = 0
        if nb and rng.random() < 0.3:
            b = int(rng.integers(0, nb))
            o["bursts"][ch, b] = [(2 * hard.shape[1], 0), (-origin - 1, 1), (0, 7), (0, -1)][int(rng.integers(0, 4))]
        if rng.random() < 0.1:
            o["nblock"][ch] = 99
        if rng.random() < 0.1:
            o["nburst"][ch] = -3
    want = Q.link_quality(soft, hard, origin, G, cells, o["nburst"], o["bursts"], o["nblock"], o["blocks"], o["type1"])
    if seed % 2 == 0:
        rc, bq, kq = Q.call(soft, hard, origin, G, cells, o)
    else:
        import torch
        c = _hip.ctx()
        keep, ts = _offset_tensor(soft, 1 + seed % 3)
        keep2, th = _offset_tensor(hard, 3 - seed % 3)
        keep3, t1 = _offset_tensor(o["type1"], 1 + (seed // 2) % 3)
        dev = [torch.from_numpy(a).to("cuda:0") for a in (cells.view(np.int32), o["nburst"], o["bursts"], o["nblock"],
                                                          o["blocks"])]
        tb = torch.full((C, 8, 4), Q.POISON, dtype=torch.int32, device="cuda:0")
        tk = torch.full((C, 16, 4), Q.POISON, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        rc = c.lib.tetra_etsi_link_quality(c.handle, _hip.ptr(ts), _hip.ptr(th), C, hard.shape[1], origin, G,
                                           *[_hip.ptr(a) for a in dev], _hip.ptr(t1), _hip.ptr(tb), _hip.ptr(tk))
        c.synchronize()
        bq, kq = tb.cpu().numpy(), tk.cpu().numpy()
    assert rc == 0
    assert np.array_equal(bq, want[0]), (seed, np.argwhere(bq != want[0])[:4].tolist())
    assert np.array_equal(kq, want[1]), (seed, np.argwhere(kq != want[1])[:4].tolist())


# ------------------------------------------------------------------------------ 8. the Python surface

BURST_KEYS = ("training_errors", "edge_errors", "soft_sum", "saturated")
BLOCK_KEYS = ("channel_errors", "channel_bits", "soft_errors", "soft_sum", "erased", "ber")


def strip(frames):
    """Frames without the link-quality keys, as plain values."""
    out = []
    for f in frames:
        g = {k: v for k, v in f.items() if k not in BURST_KEYS and k != "blocks"}
        g["blocks"] = [{k: (v.tobytes() if k == "bits" else v) for k, v in b.items() if k not in BLOCK_KEYS}
                       for b in f["blocks"]]
        out.append(g)
    return out


def test_decode_stream_with_link_quality_keeps_the_frames():
    from tetraear.core.etsi import EtsiLowerMac, cell_of
    rng = np.random.default_rng(81)
    cell = R.random_cell(rng)
    bits, planted, _ = R.place_bursts(rng, [(int(rng.integers(0, 30)), k, cell, None) for k in (N, P, SB, N, SB, P, N)], 10)
    hard, soft = R.hard_of(bits), _noisy_soft(rng, bits)
    cuts = R.cuts_at(len(hard), [(planted[1][0] + 300) // 2, (planted[3][0] + 8) // 2, (planted[5][0] + 505) // 2])
    plain, lq = EtsiLowerMac(*cell_of(cell)), EtsiLowerMac(*cell_of(cell), link_quality=True)
    nframes = scored = 0
    for at, n in cuts:
        args = (soft[None, 2 * at:2 * (at + n)], hard[None, at:at + n], np.array([n + 1], np.int32))
        a, b = plain.decode_stream(*args)[0], lq.decode_stream(*args)[0]
        assert not any(k in f for f in a for k in BURST_KEYS)
        assert strip(b) == strip(a) and all(k in f for f in b for k in BURST_KEYS)
        for f in b:   # against the model on the whole stream
            one = dict(nburst=np.array([1], np.int32), bursts=np.array([[[f["position"] + 2 * at, f["burst_kind"]]]], np.int32))
            bq, _ = Q.link_quality(soft[None, :], hard[None, :], 0, 1, [cell], one["nburst"], one["bursts"],
                                   np.zeros(1, np.int32), np.zeros((1, 16, 4), np.int32), np.zeros((1, 16, 268), np.uint8))
            assert [f[k] for k in BURST_KEYS] == bq[0, 0].tolist()
            for blk in f["blocks"]:
                assert blk["channel_bits"] in (432, 216, 120) and (blk["channel_errors"] is None) == (not blk["crc_ok"])
                if blk["crc_ok"]:
                    assert blk["ber"] == blk["channel_errors"] / (blk["channel_bits"] - blk["erased"])
                    scored += 1
        nframes += len(b)
    assert nframes == len(planted) and scored >= nframes


def test_decoder_and_carrier_quality():
    from tetraear.core import TetraDecoder
    from tetraear.core.etsi import EtsiLowerMac, carrier_quality, cell_of
    d = Q.built_rows()
    # rows 0 (clean) and 4 (three flips a block) as two carriers of one cell each
    clean, noisy = (EtsiLowerMac(*cell_of(int(d["cells"][r])), link_quality=True).decode_batch(
        d["soft"][r:r + 1], d["hard"][r:r + 1], d["nsym"][r:r + 1]) for r in (0, 4))
    q = carrier_quality(clean + noisy)
    assert q[0]["blocks"] == q[0]["blocks_ok"] == 5 and q[0]["channel_errors"] == 0 and q[0]["ber"] == 0.0
    assert q[1]["blocks_ok"] == 5 and q[1]["channel_errors"] == 9 and q[1]["ber"] > q[0]["ber"]
    assert sorted(range(2), key=lambda k: q[k]["ber"]) == [0, 1]
    # TetraDecoder passes it through (hard symbols only: +-64 soft values)
    dec = TetraDecoder(auto_decrypt=False, mode="etsi", link_quality=True)
    n = int(d["nsym"][0]) - 1
    raw = dec._etsi_rx().decode(d["hard"][0, :n], stream=False)
    assert len(raw) == 3 and all(f["training_errors"] == 0 and f["soft_sum"] == 510 * 64 for f in raw)
    assert not TetraDecoder(auto_decrypt=False, mode="etsi")._etsi_rx().link_quality


def test_wideband_decode_acquire_with_link_quality():
    from tetraear.core.etsi import carrier_quality
    from tetraear.signal.wideband import WidebandReceiver, synth_wideband
    x, cells = synth_wideband(3_300_000, seed=17, snr_db=25.0, cfo_max=300.0)[:2]
    rx = WidebandReceiver()
    unknown = np.full(len(cells), 3, np.uint32)
    plain, state0, ngood0 = rx.decode_acquire(x, unknown)
    got, state, ngood = rx.decode_acquire(x, unknown, link_quality=True)
    assert np.array_equal(state, state0) and np.array_equal(ngood, ngood0)
    assert [strip(fr) for fr in got] == [strip(fr) for fr in plain]
    blocks = [b for fr in got for f in fr for b in f["blocks"]]
    assert blocks and all((b["channel_errors"] is None) == (not b["crc_ok"]) for b in blocks)
    assert all(k in f for fr in got for f in fr for k in BURST_KEYS)
    q = carrier_quality(got)
    heard = [k for k in range(len(cells)) if ngood[k] > 0]
    assert heard and all(q[k]["blocks_ok"] > 0 and q[k]["ber"] < 0.1 for k in heard)
    # the given-cells call and the stream pass it through too
    given = rx.decode(x, cells, link_quality=True)
    assert [strip(fr) for fr in given] == [strip(fr) for fr in rx.decode(x, cells)]
    assert sum(b["crc_ok"] for fr in given for f in fr for b in f["blocks"]) >= sum(b["crc_ok"] for b in blocks)
    from tetraear.signal.wideband import WidebandStream
    a, b = WidebandStream(link_quality=True).decode(x), WidebandStream().decode(x)
    assert [strip(fr) for fr in a] == [strip(fr) for fr in b] and any(len(fr) for fr in a)
    assert all(k in f for fr in a for f in fr for k in BURST_KEYS)
    assert all(k in blk for fr in a for f in fr for blk in f["blocks"] for k in BLOCK_KEYS)
