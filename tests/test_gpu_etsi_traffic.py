"""tetra_etsi_traffic (k_etsi_traffic) against tests/_etsi_traffic_model.py: every record and every
exported byte equal to the model's on rows built on the CPU, on hand-made records at the row's edges, on
streaming and grouped rows and on a seeded sweep; then the smallest real chain and the wideband chain,
where noiseless planted traffic comes back sign for sign.  No tolerance anywhere.
tests/test_etsi_traffic_model.py proves on the CPU that the built bursts mean what is assumed here."""
import functools
import os

import numpy as np
import pytest

import etsi as E
import _etsi_mac_model as MM
import _etsi_traffic_model as T
import _lmac_rows as R

pytestmark = pytest.mark.gpu

N, P, SB = R.NDB_N, R.NDB_P, R.SB
SCALE = int(os.environ.get("TETRA_FUZZ_SCALE", "1"))
CTRL = "c"   # an ordinary coded burst of the kind


def check(soft, origin, G, cells, o, slots=None, keep=None, what="", device=False, tch_offset=0):
    """The call against the model on the same inputs, outputs poisoned first: (tq, tch)."""
    from tetraear import _hip
    want = T.traffic(soft, origin, G, cells, o["nburst"], o["bursts"], o["nblock"], o["blocks"], slots, keep)
    rc, tq, tch = T.call(soft, origin, G, cells, o, slots, keep, device=device, tch_offset=tch_offset)
    _hip.ctx().check(rc, "tetra_etsi_traffic")
    assert np.array_equal(tq, want[0]), (what, np.argwhere(tq != want[0])[:4].tolist())
    assert np.array_equal(tch, want[1]), (what, np.argwhere(tch != want[1])[:4].tolist())
    return tq, tch


def poisoned(o):
    """The lower MAC's outputs with what it did not write poisoned."""
    o = {k: v.copy() for k, v in o.items()}
    for c in range(len(o["nburst"])):
        o["bursts"][c, int(o["nburst"][c]):] = T.POISON
        o["blocks"][c, int(o["nblock"][c]):] = T.POISON
    return o


def build_row(rng, cell, items, lead, tail=0, gaps=(0, 1, 2, 3, 5)):
    """A row of bursts (kind, t4 or CTRL): (bits, [(start, kind, t4 or None)])."""
    scr = E.scramble_seq(int(cell), 432)
    parts, planted, at = [rng.integers(0, 2, lead).astype(np.uint8)], [], lead
    for kind, t4 in items:
        ctrl = isinstance(t4, str)
        b = E.make_burst(kind, rng, scr)[0] if ctrl else T.traffic_burst(kind, t4, scr, rng)[0]
        g = int(rng.choice(gaps))
        parts += [b, rng.integers(0, 2, g).astype(np.uint8)]
        planted.append((at, kind, None if ctrl else t4))
        at += 510 + g
    parts.append(rng.integers(0, 2, tail + ((at + tail) & 1)).astype(np.uint8))
    return np.concatenate(parts), planted


def noisy_soft(rng, bits, planted=(), flips=0.0):
    """Soft bits of random strength, a few of them zero; in the fields a planted traffic burst exports a few
    -128 too (a 1 at full scale; the control decoders never read those fields' CRC as good anyway)."""
    s = R.soft_of(bits, 1).astype(np.int16) * rng.integers(24, 128, len(bits))
    s[rng.random(len(bits)) < 0.01] = 0
    for start, kind, t4 in planted:
        if t4 is not None:
            p = start + T.field_offsets(T.FULL if kind == N else T.HALF)
            p = p[(rng.random(len(p)) < 0.03) & (np.asarray(bits)[p] == 1)]
            s[p] = -128
    if flips:
        wrong = rng.random(len(bits)) < flips
        s[wrong] = -s[wrong].clip(-127, 127)
    return s.astype(np.int8)


def expected_class(kind, t4):
    return T.NONE if kind == SB else T.CONTROL if t4 is None else T.FULL if kind == N else T.HALF


@functools.lru_cache(maxsize=None)
def built(C):
    """C rows of three bursts (<= 1600 bits): row r starts its first burst at bit r mod 8 -- row 0 at row
    bit 0 -- and the gaps of 0..5 bits put the others at every byte alignment and at odd bits."""
    rng = np.random.default_rng(5000 + C)
    cells = np.array([R.random_cell(rng) for _ in range(C)], np.uint32)
    menu = [(N, "t"), (P, "t"), (SB, CTRL), (N, CTRL), (P, CTRL)]
    rows, planted = [], []
    for r in range(C):
        items = [menu[(r + i) % 5] if i else menu[r % 2] for i in range(3)]
        items = [(k, rng.integers(0, 2, 432 if k == N else 216).astype(np.uint8) if t == "t" else CTRL) for k, t in items]
        bits, pl = build_row(rng, cells[r], items, r % 8, int(rng.integers(0, 5)))
        assert len(bits) <= 1600
        rows.append((bits, noisy_soft(rng, bits, pl)))
        planted.append(pl)
    hard, soft, nsym = R.pack_rows(rows, max(len(b) for b, _ in rows) // 2 + 1 + C % 3)
    return dict(hard=hard, soft=soft, nsym=nsym, cells=cells, planted=planted)


# ------------------------------------------------------------------------------ 1. built rows

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("C", [1, 5, 7, 64])
def test_built_rows_equal_the_model(C, device):
    d = built(C)
    o = R.run_lmac(d["hard"], d["soft"], d["nsym"], d["cells"])
    tq, tch = check(d["soft"], 0, 1, d["cells"], poisoned(o), what="built %d" % C, device=device)
    starts = set()
    for r, pl in enumerate(d["planted"]):
        assert o["nburst"][r] == 3 and [tuple(v) for v in o["bursts"][r, :3].tolist()] == [(s, k) for s, k, _ in pl], r
        for b, (s, k, t4) in enumerate(pl):
            assert tq[r, b, T.CLASS] == expected_class(k, t4), (r, b)
            starts.add(s % 8)
            if t4 is not None:   # the soft bits carry the planted signs (a zero decides for 0)
                n = len(t4)
                nz = tch[r, b, :n] != 0
                assert tq[r, b, T.NBITS] == n and np.array_equal(T.signs(tch[r, b, :n])[nz], t4[nz]), (r, b)
                assert tq[r, b, T.NZERO] == int((~nz).sum()) and (tch[r, b, n:] == T.POISON8).all()
        assert (tq[r, 3:] == T.POISON).all() and (tch[r, 3:] == T.POISON8).all()
    if C >= 5:   # every byte alignment, odd bits, row bit 0
        assert {v % 4 for v in starts} == {0, 1, 2, 3} and d["planted"][0][0][0] == 0


# ------------------------------------------------------------------------------ 2. hand-made records

def _records(C):
    return dict(nburst=np.zeros(C, np.int32), bursts=np.full((C, 8, 2), T.POISON, np.int32),
                nblock=np.zeros(C, np.int32), blocks=np.full((C, 16, 4), T.POISON, np.int32))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_row_edges_clamps_and_stray_records(device):
    rng = np.random.default_rng(61)
    C, stride = 6, 2300   # 4600 bits a row: eight bursts side by side, and odd leftovers
    soft = rng.integers(-128, 128, (C, 2 * stride)).astype(np.int8)
    cells = np.array([R.random_cell(rng) for _ in range(C)], np.uint32)
    o = _records(C)
    # row 0: a burst at row bit 0 and one ending on the row's last bit; one bit past it, one before the row,
    # kinds outside 0..2
    o["nburst"][0] = 6
    o["bursts"][0, :6] = [(0, 0), (2 * stride - 510, 1), (2 * stride - 509, 0), (-1, 1), (7, 3), (7, -1)]
    o["nblock"][0] = 1
    o["blocks"][0, 0] = (1, 1, 1, 0)
    # row 1: nburst > 8 and nblock > 16 clamp; the sixteenth record decides burst 7, a seventeenth would not count
    o["nburst"][1], o["nblock"][1] = 99, 99
    o["bursts"][1] = [(3 + 571 * b, b % 2) for b in range(8)]
    o["blocks"][1] = [(2, 1, 0, 0)] * 15 + [(1, 1, 7, 0)]
    # row 2: records that name no live burst (3 is past nburst, -1, 8), an impossible (kind, index), another
    # burst's kind, a CRC-bad one: none of them makes burst 0 or 1 CONTROL
    o["nburst"][2], o["nblock"][2] = 3, 8
    o["bursts"][2, :3] = [(11, 0), (600, 1), (1201, 0)]
    o["blocks"][2, :8] = [(0, 1, 3, 0), (0, 1, -1, 0), (0, 1, 8, 0), (0, 1, 0, 1), (1, 1, 0, 0), (0, 0, 0, 0),
                          (1, 1, 1, 1), (0, 1, 2, 0)]
    # row 3: negative counts write nothing; row 4: no bursts
    o["nburst"][3], o["nblock"][3] = -3, -1
    # row 5: -128 under q = 0 and q = 1, and zeros, in both fields
    o["nburst"][5] = 2
    o["bursts"][5, :2] = [(5, 0), (1001, 1)]
    o["nblock"][5] = 1
    o["blocks"][5, 0] = (1, 1, 1, 0)
    soft[5, 5 + 14:5 + 230:3] = -128
    soft[5, 5 + 282:5 + 498:5] = 0
    soft[5, 1001 + 282:1001 + 498:2] = -128
    tq, tch = check(soft, 0, 1, cells, o, what="edges", device=device)
    assert tq[0, :6, 0].tolist() == [T.FULL, T.HALF, -1, -1, -1, -1] and (tq[0, 6:] == T.POISON).all()
    assert tq[1, :, 0].tolist() == [T.FULL, T.LOST] * 3 + [T.FULL, T.HALF]
    assert tq[2, :3, 0].tolist() == [T.FULL, T.LOST, T.CONTROL]
    assert (tq[3:5] == T.POISON).all() and (tch[3:5] == T.POISON8).all()
    scr = E.scramble_seq(int(cells[5]), 432)
    assert (tch[5, 0, :216:3][scr[:216:3] == 1] == 127).all() and (tch[5, 0, :216:3][scr[:216:3] == 0] == -128).all()
    assert tq[5, 0, T.NZERO] >= 44 and (tch[5, 1, :216:2][scr[:216:2] == 1] == 127).any()


# ------------------------------------------------------------------------------ 3. error returns

def test_error_returns_write_nothing():
    from tetraear import _hip
    d = built(5)
    o = R.run_lmac(d["hard"], d["soft"], d["nsym"], d["cells"])
    for name, kw in (("cell_init NULL", dict(cells=None)), ("G 0", dict(G=0)), ("C % G", dict(G=4)),
                     ("stride 0", dict(stride=0)), ("origin < 0", dict(origin=-2)), ("nburst NULL", dict(drop="nburst")),
                     ("bursts NULL", dict(drop="bursts")), ("nblock NULL", dict(drop="nblock")),
                     ("blocks NULL", dict(drop="blocks"))):
        a = dict(cells=d["cells"], G=1, origin=0, stride=None, drop=None)
        a.update(kw)
        oo = dict(o)
        if a["drop"]:
            oo[a["drop"]] = None
        rc, tq, tch = T.call(d["soft"], a["origin"], a["G"], a["cells"], oo, stride=a["stride"])
        assert rc == -1, (name, rc)
        assert (tq == T.POISON).all() and (tch == T.POISON8).all(), name
    c = _hip.ctx()
    tq, tch = np.full((5, 8, 4), T.POISON, np.int32), np.full((5, 8, 432), T.POISON8, np.int8)
    base = [_hip.ptr(d["soft"]), 5, d["soft"].shape[1] // 2, 0, 1, _hip.ptr(d["cells"]), _hip.ptr(o["nburst"]),
            _hip.ptr(o["bursts"]), _hip.ptr(o["nblock"]), _hip.ptr(o["blocks"]), None, None, _hip.ptr(tq), _hip.ptr(tch)]
    for i, name in ((0, "softbits NULL"), (1, "C 0"), (12, "tq NULL"), (13, "tch NULL")):
        args = list(base)
        args[i] = 0 if i == 1 else None
        assert c.lib.tetra_etsi_traffic(c.handle, *args) == -1, name
    assert (tq == T.POISON).all() and (tch == T.POISON8).all()
    assert c.lib.tetra_etsi_traffic(None, *base) == -1
    assert c.lib.tetra_etsi_traffic(c.handle, *base) == 0 and (tq[:, :3] != T.POISON).all()


# ------------------------------------------------------------------------------ 4. streaming rows

def test_stream_rows_with_negative_starts():
    """Three chunks through tetra_lmac_etsi_stream into alternate rows, a traffic burst across each seam:
    with origin_bits = 2 RESERVE the records equal the model on the whole stream, sign for sign the planted
    bits."""
    from tetraear import _hip
    c = _hip.ctx()
    RES = _hip.ETSI_RESERVE
    rng = np.random.default_rng(414)
    C, chans = 3, []
    for ch in range(C):
        cell = R.random_cell(rng)
        kinds = [(SB, N, P, N, N, P), (N, P, SB, N, P, N), (P, N, N, P, SB, N)][ch]
        items = [(k, CTRL if k == SB or i in (0, 5) else rng.integers(0, 2, 432 if k == N else 216).astype(np.uint8))
                 for i, k in enumerate(kinds)]
        bits, planted = build_row(rng, cell, items, int(rng.integers(0, 40)), 30, gaps=(0, 1, 7, 12))
        hard = R.hard_of(bits)
        # seams inside burst 1's second field and burst 3's first
        cuts = R.cuts_at(len(hard), [(planted[1][0] + 400) // 2, (planted[3][0] + 100) // 2])
        chans.append((bits, hard, noisy_soft(rng, bits, planted), cuts, cell, planted))
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
        o = R.lmac_outputs(C)
        c.check(c.lib.tetra_lmac_etsi_stream(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, stride,
                                             _hip.ptr(lead), _hip.ptr(nsoft), _hip.ptr(nhard), None, _hip.ptr(o["nburst"]),
                                             _hip.ptr(o["bursts"]), _hip.ptr(o["nblock"]), _hip.ptr(o["blocks"]),
                                             _hip.ptr(o["type1"])), "tetra_lmac_etsi_stream")
        tq, tch = check(soft, 2 * RES, 1, cells, poisoned(o), what="stream %d" % k, device=bool(k % 2))
        for ch, (_, _, s_all, _, cell, planted) in enumerate(chans):   # the same bursts in the whole stream
            one = {key: v[ch:ch + 1].copy() for key, v in o.items()}
            one["bursts"][0, :, 0] += 2 * at0[ch]
            want = T.traffic(s_all[None, :], 0, 1, cells[ch:ch + 1], one["nburst"], one["bursts"], one["nblock"],
                             one["blocks"])
            nb = int(o["nburst"][ch])
            assert np.array_equal(tq[ch, :nb], want[0][0, :nb]) and np.array_equal(tch[ch, :nb], want[1][0, :nb]), (k, ch)
            negative += int((o["bursts"][ch, :nb, 0] < 0).sum())
            for b in range(nb):
                s, kd = int(o["bursts"][ch, b, 0]) + 2 * at0[ch], int(o["bursts"][ch, b, 1])
                t4 = dict((p[0], p[2]) for p in planted)[s]
                found[ch].append((s, kd))
                assert tq[ch, b, 0] == expected_class(kd, t4), (k, ch, b)
                if t4 is not None:
                    nz = tch[ch, b, :len(t4)] != 0
                    assert np.array_equal(T.signs(tch[ch, b, :len(t4)])[nz], t4[nz])
    assert found == [[(s, kd) for s, kd, _ in ch[5]] for ch in chans]
    assert negative >= 2 * C   # a burst across each seam began in the carried tail


# ------------------------------------------------------------------------------ 5. groups, slots and keep

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_groups_slots_and_keep(device):
    """G = 3 with a different cell per group; slots / keep NULL and given, FN = 18 and keep = 0 set by hand."""
    rng = np.random.default_rng(87)
    C, G = 6, 3
    cells = np.array([R.random_cell(rng) for _ in range(C // G)], np.uint32)
    rows, planted = [], []
    for r in range(C):
        t4 = rng.integers(0, 2, 432).astype(np.uint8)
        bits, pl = build_row(rng, cells[r // G], [(N, t4), (P, t4[:216]), (SB, CTRL)][r % 3:] + [(N, t4)], r + 1)
        rows.append((bits, noisy_soft(rng, bits, pl)))
        planted.append(pl)
    hard, soft, nsym = R.pack_rows(rows, max(len(b) for b, _ in rows) // 2 + 2)
    o = R.run_lmac(hard, soft, nsym, np.repeat(cells, G))
    assert o["nburst"].tolist() == [len(pl) for pl in planted]
    tq, tch = check(soft, 0, G, cells, poisoned(o), what="groups", device=device)
    for r, pl in enumerate(planted):
        for b, (s, k, t4) in enumerate(pl):
            assert tq[r, b, 0] == expected_class(k, t4)
            if t4 is not None:
                nz = tch[r, b, :len(t4)] != 0
                assert np.array_equal(T.signs(tch[r, b, :len(t4)])[nz], t4[nz]), (r, b)
    # the cell is the call's argument: with the groups' cells exchanged the signs are not the planted ones
    _, tch2 = check(soft, 0, G, cells[::-1].copy(), poisoned(o), what="groups, cells exchanged", device=device)
    assert (T.signs(tch2[0, 0]) != planted[0][0][2]).sum() > 100
    slots = rng.integers(1, 18, (C, 8, 4)).astype(np.int32)
    keep = np.ones((C, 8), np.int32)
    slots[0, 0, T.SLOT_FN] = slots[1, 0, T.SLOT_FN] = slots[2, 0, T.SLOT_FN] = 18   # a full slot, a half slot, an SB
    keep[0, 1] = keep[3, 0] = keep[2, 0] = 0
    keep[4, 0] = 2   # any non-zero value keeps
    for sl, kp in ((slots, None), (None, keep), (slots, keep)):
        got, _ = check(soft, 0, G, cells, poisoned(o), sl, kp, what="slots / keep", device=device)
        assert got[0, 0, 0] == (T.CONTROL if sl is not None else T.FULL)
        assert got[0, 1, 0] == (T.NONE if kp is not None else T.HALF)
        assert got[2, 0, 0] == T.NONE and got[4, 0, 0] == tq[4, 0, 0]
        assert got[3, 0, 0] == (T.NONE if kp is not None else T.FULL)
        assert got[1, 0, 0] == (T.CONTROL if sl is not None else T.HALF)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_tch_base_that_is_not_dword_aligned(off):
    d = built(7)
    o = R.run_lmac(d["hard"], d["soft"], d["nsym"], d["cells"])
    check(d["soft"], 0, 1, d["cells"], poisoned(o), what="tch + %d" % off, device=True, tch_offset=off)


def test_one_kernel_under_its_profile_stage():
    """With device pointers the call is one launch under the stage etsi_traffic."""
    import ctypes
    import torch
    from tetraear import _hip
    d = built(5)
    o = R.run_lmac(d["hard"], d["soft"], d["nsym"], d["cells"])
    c = _hip.ctx()
    c.check(c.lib.tetra_profile(c.handle, 1), "tetra_profile")
    try:
        rc, _, _ = T.call(d["soft"], 0, 1, d["cells"], o, device=True)
        torch.cuda.synchronize()
        names = ctypes.create_string_buffer(4096)
        ms, cnt, n = (ctypes.c_double * 64)(), (ctypes.c_int64 * 64)(), ctypes.c_int()
        c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    finally:
        c.check(c.lib.tetra_profile(c.handle, 0), "tetra_profile")
    stages = [s.decode() for s in names.raw.split(b"\0")[:n.value]]
    assert rc == 0 and "etsi_traffic" in stages and cnt[stages.index("etsi_traffic")] == 1


# ------------------------------------------------------------------------------ 6. seeded sweep

@pytest.mark.parametrize("seed", range(20 * SCALE))
def test_random_rows_vs_model(seed):
    """Random C in 1..9, G dividing C, origin, burst placements, soft-bit classes, CRC flags changed, bursts
    made invalid, counts out of range, random slots and keep; odd seeds on device copies whose row and tch
    pointers are not dword aligned."""
    rng = np.random.default_rng(9100 + seed)
    C = int(rng.integers(1, 10))
    G = int(rng.choice([g for g in range(1, C + 1) if C % g == 0]))
    cells = np.array([R.random_cell(rng) for _ in range(C // G)], np.uint32)
    rows = []
    for ch in range(C):
        items = []
        for _ in range(int(rng.integers(0, 4))):
            k = int(rng.integers(0, 3))
            traffic = k != SB and rng.random() < 0.6
            items.append((k, rng.integers(0, 2, 432 if k == N else 216).astype(np.uint8) if traffic else CTRL))
        bits, planted = build_row(rng, cells[ch // G], items, int(rng.choice(R.GAPS[3:6])) if rng.random() < 0.5 else 0,
                                  int(rng.integers(0, 9)), gaps=R.GAPS[:6])
        soft = noisy_soft(rng, bits, planted, 0.004)
        if planted and rng.random() < 0.4:
            s = planted[0][0]
            soft[s:s + 510] = R.soft_class(str(rng.choice(["m128", "uniform", "zero", "tern"])), bits[s:s + 510], rng)
        rows.append((bits, soft))
    smax = max(max(len(b) for b, _ in rows) // 2 + 1 + int(rng.integers(0, 4)), 4)
    hard, soft, nsym = R.pack_rows(rows, smax)
    o = poisoned({k: v for k, v in R.run_lmac(hard, soft, nsym, np.repeat(cells, G)).items() if k != "type1"})
    origin = int(rng.integers(0, 40))   # the rows `origin` bits to the right, behind random soft bits
    soft = np.concatenate([rng.integers(-128, 128, (C, origin)).astype(np.int8), soft,
                           np.zeros((C, origin & 1), np.int8)], 1)
    for ch in range(C):   # records the lower MAC would not write
        nb, nk = int(o["nburst"][ch]), int(o["nblock"][ch])
        if nk and rng.random() < 0.4:
            j = int(rng.integers(0, nk))
            o["blocks"][ch, j, 1] = int(rng.integers(0, 3)) * int(rng.integers(0, 2))
        if nk and rng.random() < 0.2:
            o["blocks"][ch, int(rng.integers(0, nk)), int(rng.integers(2, 4))] = int(rng.integers(-1, 9))
        if nb and rng.random() < 0.3:
            b = int(rng.integers(0, nb))
            o["bursts"][ch, b] = [(soft.shape[1], 0), (-origin - 1, 1), (0, 7), (0, -1), (soft.shape[1] - 509, 1)][
                int(rng.integers(0, 5))]
        if rng.random() < 0.1:
            o["nblock"][ch] = 99
        if rng.random() < 0.1:
            o["nburst"][ch] = -3
    slots = keep = None
    if rng.random() < 0.6:
        slots = rng.integers(0, 19, (C, 8, 4)).astype(np.int32)
        slots[rng.random((C, 8)) < 0.2, T.SLOT_FN] = 18
    if rng.random() < 0.6:
        keep = (rng.random((C, 8)) < 0.7).astype(np.int32) * rng.integers(1, 4, (C, 8)).astype(np.int32)
    if seed % 2 == 0:
        check(soft, origin, G, cells, o, slots, keep, what=seed)
        return
    import torch
    raw = soft.reshape(-1)   # the rows 1..3 bytes past an allocation's start
    buf = torch.zeros(raw.size + 8, dtype=torch.int8, device="cuda:0")
    off = 1 + seed % 3
    buf[off:off + raw.size] = torch.from_numpy(raw).to("cuda:0")
    want = T.traffic(soft, origin, G, cells, o["nburst"], o["bursts"], o["nblock"], o["blocks"], slots, keep)
    rc, tq, tch = T.call(_Rows(buf[off:off + raw.size], soft.shape), origin, G, cells, o, slots, keep, device=True,
                         tch_offset=(seed // 2) % 4)
    assert rc == 0
    assert np.array_equal(tq, want[0]), (seed, np.argwhere(tq != want[0])[:4].tolist())
    assert np.array_equal(tch, want[1]), (seed, np.argwhere(tch != want[1])[:4].tolist())


class _Rows:
    """A device tensor that T.call passes on as it is, with the shape of the rows it holds."""
    def __init__(self, t, shape):
        self.t, self.shape = t, shape


# ------------------------------------------------------------------------------ 7. the smallest real chain

CHAIN_KINDS = (N, SB, N, N, P, P, N, SB, N, P, N, N, SB, N, N)
CHAIN_TRAFFIC = {3: 432, 5: 216, 8: 432}   # burst -> exported bits: two full slots, one stolen + half slot


@functools.lru_cache(maxsize=None)
def _chain():
    """One channel at 2.4 MSps, four 131072-sample chunks of an E.modulate'd stream without noise, through
    EtsiStream + EtsiLowerMac(traffic=True, mac=True) in acquisition mode: (frames per chunk, the model's
    (tq, tch) per chunk on the rows each call read, planted t4 per burst, the cell)."""
    from tetraear import _hip
    from tetraear.signal.etsi import EtsiStream
    from tetraear.core.etsi import EtsiLowerMac
    rng = np.random.default_rng(2718)
    fields = (int(rng.integers(1, 1024)), int(rng.integers(0, 1 << 14)), int(rng.integers(0, 64)))
    cell = E.scramble_init(*fields)
    scr = E.scramble_seq(cell, 432)
    parts, t4s = [rng.integers(0, 2, 60).astype(np.uint8)], {}
    for b, kind in enumerate(CHAIN_KINDS):
        if b in CHAIN_TRAFFIC:
            t4s[b] = rng.integers(0, 2, CHAIN_TRAFFIC[b]).astype(np.uint8)
            parts.append(T.traffic_burst(kind, t4s[b], scr, rng)[0])
        else:
            pay = None
            if kind == SB:   # slot counts from 0: frames 1..4, never the control frame
                pay = [MM.block(rng, 2, [MM.sync(MM.sync_for_slot(rng, b, fields))]), rng.integers(0, 2, 124).astype(np.uint8)]
            parts.append(E.make_burst(kind, rng, scr, pay)[0])
    parts.append(rng.integers(0, 2, 400).astype(np.uint8))
    L = 131072
    x = E.modulate(np.concatenate(parts), 4 * L, t0=0.4, phase0=1.1, cfo=120.0)
    st, lm = EtsiStream(2.4e6, 1), EtsiLowerMac(traffic=True, mac=True)
    frames, model = [], []
    for k in range(4):
        d = st.demod(x[None, k * L:(k + 1) * L])
        fr = lm.decode_stream(d[1], d[0], d[3])[0]
        # the records of the call, from the frames; the rows it read are the receiver's other set now
        o = _records(1)
        o["nburst"][0] = len(fr)
        slots = np.zeros((1, 8, 4), np.int32)
        j = 0
        for b, f in enumerate(fr):
            o["bursts"][0, b] = (f["position"], f["burst_kind"])
            slots[0, b, T.SLOT_FN] = f["fn"] or 0
            for blk in f["blocks"]:
                o["blocks"][0, j] = ({"SCH/F": 0, "SCH/HD": 1, "BSCH": 2}[blk["channel"]], int(blk["crc_ok"]), b, blk["block"])
                j += 1
        o["nblock"][0] = j
        model.append(T.traffic(lm._alt[0], 2 * _hip.ETSI_RESERVE, 1, [int(lm.cell_state[0])], o["nburst"], o["bursts"],
                               o["nblock"], o["blocks"], slots) + (bool(lm.acquired[0]),))
        frames.append(fr)
    return frames, model, t4s, cell, lm


def test_chain_exports_equal_the_model_on_the_rows_read():
    frames, model, _, cell, lm = _chain()
    assert int(lm.cell_state[0]) == cell and sum(len(fr) for fr in frames) >= 12
    usages = []
    for fr, (tq, tch, has_cell) in zip(frames, model):
        for b, f in enumerate(fr):
            usages.append(f["usage"])
            if not has_cell:
                assert f["usage"] is None and f["traffic"] is None
                continue
            cls = int(tq[0, b, 0])
            assert f["usage"] == {T.NONE: "sync", T.CONTROL: "control", T.FULL: "traffic", T.HALF: "stolen", T.LOST: "lost"}[cls]
            if cls in (T.FULL, T.HALF):
                t = f["traffic"]
                assert [t["bits"], t["soft_sum"], t["erased"]] == tq[0, b, 1:].tolist()
                assert np.array_equal(t["soft"], tch[0, b, :t["bits"]])
            else:
                assert f["traffic"] is None
    assert usages.count("traffic") == 2 and usages.count("stolen") == 1 and "sync" in usages and "control" in usages
    assert "lost" not in usages


def test_chain_returns_the_planted_bits_and_the_codec_frame():
    from tetraear.core.etsi import codec_frame, slot_usage, traffic_streams
    frames, _, t4s, _, _ = _chain()
    flat = [f for fr in frames for f in fr]
    got = [f for f in flat if f["usage"] in ("traffic", "stolen")]
    want = [t4s[b] for b in sorted(t4s)]
    assert len(got) == len(want)
    for f, t4 in zip(got, want):   # in time order, sign for sign
        t = f["traffic"]
        assert t["bits"] == len(t4) and t["erased"] == 0 and np.array_equal(T.signs(t["soft"]), t4)
        assert t["soft_sum"] >= len(t4) and f["tn"] is not None and f["fn"] != 18
        if t["bits"] == 432:
            w = np.frombuffer(codec_frame(t["soft"]), "<i2")
            assert w[0] == 0x6B21 and np.array_equal(w[np.r_[1:115, 116:230, 231:345, 346:436]] > 0, t4 == 1)
        else:
            with pytest.raises(ValueError):
                codec_frame(t["soft"])
    # bursts 3 and 8 are slots 3 and 8: TN 4 and TN 1
    st = traffic_streams(flat)
    assert sorted(st) == [1, 4] and all(len(v) == 1 for v in st.values())
    use = slot_usage(flat)
    assert use[4]["traffic"] == 1 and use[1]["traffic"] == 1 and sum(sum(d.values()) for d in use.values()) == len(flat)


def test_traffic_false_keeps_the_frames():
    from tetraear.core.etsi import EtsiLowerMac, cell_of
    d = built(5)
    for r in range(3):
        kw = dict(zip(("mcc", "mnc", "colour_code"), cell_of(int(d["cells"][r]))))
        a = EtsiLowerMac(**kw).decode_batch(d["soft"][r:r + 1], d["hard"][r:r + 1], d["nsym"][r:r + 1])[0]
        b = EtsiLowerMac(traffic=True, **kw).decode_batch(d["soft"][r:r + 1], d["hard"][r:r + 1], d["nsym"][r:r + 1])[0]
        assert len(a) == len(b) == 3 and not any("usage" in f or "traffic" in f for f in a)
        for f, g, (s, k, t4) in zip(a, b, d["planted"][r]):
            assert set(g) == set(f) | {"usage", "traffic"}
            assert all(np.array_equal(f[key], g[key]) if key != "blocks" else len(f[key]) == len(g[key]) for key in f)
            assert g["usage"] == {T.NONE: "sync", T.CONTROL: "control", T.FULL: "traffic", T.HALF: "stolen"}[expected_class(k, t4)]
    # acquisition mode: a channel without a cell reports nothing
    r = [i for i in range(5) if all(k != SB for _, k, _ in d["planted"][i])][0]
    fr = EtsiLowerMac(traffic=True).decode_batch(d["soft"][r:r + 1], d["hard"][r:r + 1], d["nsym"][r:r + 1])[0]
    assert len(fr) == 3 and all(f["usage"] is None and f["traffic"] is None for f in fr)


def test_decoder_keeps_the_exported_slots():
    """TetraDecoder(mode="etsi") drops a burst without a PDU whose CRC failed; with traffic=True the slots
    exported for the codec stay, and nothing else about the frames changes."""
    from tetraear.core import TetraDecoder
    from tetraear.core.etsi import codec_frame
    d = built(5)   # row 0: a full slot, a stolen + half slot, an SB that announces nothing the rows need
    rows = (d["soft"][:1], d["hard"][:1], d["nsym"][:1])
    cells = d["cells"][:1]
    on, off = (TetraDecoder(auto_decrypt=False, mode="etsi", traffic=t) for t in (True, False))
    a = on._etsi_frames(on._etsi_rx().decode_batch(*rows, cells=cells)[0])
    b = off._etsi_frames(off._etsi_rx().decode_batch(*rows, cells=cells)[0])
    full = d["planted"][0][0]
    assert full[1] == N and full[2] is not None
    kept = [f for f in a if f["position"] == full[0]]
    assert len(kept) == 1 and kept[0]["usage"] == "traffic" and not any(f["position"] == full[0] for f in b)
    assert len(codec_frame(kept[0]["traffic"]["soft"])) == 1380
    # every frame of the plain decoder is there, and what is there beyond them was exported (the full slot,
    # and the half slot when its stolen half held no PDU)
    at = {f["position"]: f for f in a}
    assert len(b) >= 1 and not any("usage" in f for f in b)
    for g in b:
        f = at.pop(g["position"])
        assert set(f) == set(g) | {"usage", "traffic"} and f["header"] == g["header"] and f["burst_crc"] == g["burst_crc"]
    assert full[0] in at and all(f["traffic"] is not None for f in at.values())


# ------------------------------------------------------------------------------ 8. the wideband chain

NW = 1_700_000
CARRIERS = (3, 130, 257, 401, 640, 797)
WB_KINDS = ((0, 2, 1, 0, 2, 0, 1, 0), (1, 2, 0, 0, 1, 2, 0, 0), (0, 1, 0, 2, 0, 1, 0, 0), (2, 0, 0, 0, 2, 0, 1, 0),
            (0, 2, 0, 1, 2, 1, 0, 0), (1, 1, 2, 2, 0, 0, 1, 0))
WB_SLOT0 = (4316, 70, 2000, 17, 4319, 1234)
# traffic slots (carrier index, burst): carrier 130's bursts 2 (full) and 4 (stolen + half); carrier 401's
# burst 3, which 450 lead bits put at symbols 990..1245 of the row -- whole inside both chunks (the second
# starts at symbol 983, 3932 samples in, and the first ends at 1253: the 1080-sample overlap)
WB_TRAFFIC = {(1, 2): 432, (1, 4): 216, (3, 3): 432}
WB_LEAD = {3: 450}
# a carrier of normal bursts only: it never announces its cell
WB_SILENT, WB_SILENT_KINDS = 520, (0, 1, 0, 0, 1, 0, 1, 0)


@pytest.fixture(scope="module")
def planted():
    """(x [NW] complex64, cells [800] uint32, {(carrier, burst): (t4, slot)})."""
    import wideband as W
    d = W.design()
    M, D = d["M"], d["D"]
    nbb = NW // D + 1
    s = np.zeros((M, nbb), np.complex128)
    cells = np.full(M, 3, np.uint32)
    truth = {}
    for i, k in enumerate(CARRIERS):
        rng = np.random.default_rng(940 + i)
        cell = (int(rng.integers(1, 1024)), int(rng.integers(0, 1 << 14)), int(rng.integers(0, 64)))
        cells[k] = E.scramble_init(*cell)
        scr = E.scramble_seq(int(cells[k]))
        bits = [rng.integers(0, 2, WB_LEAD.get(i, 0)).astype(np.uint8)]
        for b, kind in enumerate(WB_KINDS[i]):
            slot = (WB_SLOT0[i] + b) % MM.TDMA_SLOTS
            if (i, b) in WB_TRAFFIC:
                t4 = rng.integers(0, 2, WB_TRAFFIC[(i, b)]).astype(np.uint8)
                truth[(k, b)] = (t4, slot)
                bits.append(T.traffic_burst(kind, t4, scr, rng)[0])
                continue
            pay = None
            if kind == E.BURST_SB:
                pay = [MM.block(rng, 2, [MM.sync(MM.sync_for_slot(rng, slot, cell))]), rng.integers(0, 2, 124).astype(np.uint8)]
            bits.append(E.make_burst(kind, rng, scr, pay)[0])
        s[k] = E.modulate(np.concatenate(bits), nbb, fs=d["fs"] / D, t0=0.1 + 0.13 * i, phase0=0.7 * i,
                          cfo=(-100.0, -40.0, 0.0, 25.0, 60.0, 100.0)[i])
    rng = np.random.default_rng(949)
    cells[WB_SILENT] = R.random_cell(rng)
    scr = E.scramble_seq(int(cells[WB_SILENT]))
    s[WB_SILENT] = E.modulate(np.concatenate([E.make_burst(kind, rng, scr)[0] for kind in WB_SILENT_KINDS]), nbb,
                              fs=d["fs"] / D, t0=0.3, phase0=0.5, cfo=-70.0)
    return W.synthesize(s, d, NW).astype(np.complex64), cells, truth


def _judge(frames, truth, what):
    """Every planted traffic slot is reported once, with its tn / fn / mn and the planted signs; no other
    frame of a planted carrier claims traffic."""
    hits = {}
    for k, fr in enumerate(frames):
        if k not in CARRIERS:
            continue
        for f in fr:
            if f["usage"] not in ("traffic", "stolen"):
                assert f["traffic"] is None, (what, k)
                continue
            t = f["traffic"]
            mine = [key for key, (t4, _) in truth.items() if key[0] == k and len(t4) == t["bits"] and
                    np.array_equal(T.signs(t["soft"]), t4)]
            if not mine:   # a burst an edge cut reads as a candidate too: never a decoded one
                assert not f["crc_ok"], (what, k, f["sample"])
                continue
            assert mine[0] not in hits, (what, mine[0])
            hits[mine[0]] = f
            slot = truth[mine[0]][1]
            assert (f["tn"], f["fn"], f["mn"]) == (slot % 4 + 1, slot // 4 % 18 + 1, slot // 72 + 1), (what, mine[0])
            assert f["usage"] == ("traffic" if t["bits"] == 432 else "stolen") and t["erased"] == 0
    assert sorted(hits) == sorted(truth), (what, sorted(hits))
    return hits


def test_wideband_reports_each_planted_slot_once(planted):
    from tetraear import _hip
    from tetraear.signal.wideband import WidebandReceiver
    x, cells, truth = planted
    rx = WidebandReceiver()
    frames = rx.decode(x, cells, traffic=True, timebase="vote")
    hits = _judge(frames, truth, "decode")
    plain = rx.decode(x, cells, timebase="vote")
    for k in CARRIERS:   # the same frames, two keys more
        assert len(frames[k]) == len(plain[k]) > 0
        for f, g in zip(frames[k], plain[k]):
            assert set(f) == set(g) | {"usage", "traffic"} and all(f[key] == g[key] for key in g if key != "blocks")
    assert all(f["usage"] in ("sync", "control", "traffic", "stolen", "lost") for k in CARRIERS for f in frames[k])
    assert len(frames[WB_SILENT]) >= 4 and all(f["usage"] == "control" for f in frames[WB_SILENT])
    # the slot in the overlap is whole in both chunk rows: both export it, keep reports one
    k = CARRIERS[3]
    hard, soft, _, ns = rx.demod(x)
    o = R.run_lmac(np.ascontiguousarray(hard[k]), np.ascontiguousarray(soft[k]), np.ascontiguousarray(ns[k]),
                   np.repeat(cells[k], hard.shape[1]))
    tq, tch = check(np.ascontiguousarray(soft[k]), 0, hard.shape[1], cells[k:k + 1], poisoned(
        {key: v for key, v in o.items() if key != "type1"}), what="overlap rows")
    t4 = truth[(k, 3)][0]
    both = [(r, b) for r in range(hard.shape[1]) for b in range(int(o["nburst"][r]))
            if tq[r, b, 0] == T.FULL and np.array_equal(T.signs(tch[r, b]), t4)]
    assert [r for r, _ in both] == [0, 1], both
    assert hits[(k, 3)]["chunk"] in (0, 1)
    # acquisition: the same slots with the acquired cells, and nothing claimed where no cell was heard
    got, state, ngood = rx.decode_acquire(x, np.full(len(cells), 3, np.uint32), traffic=True, timebase="vote")
    assert all(int(state[k]) == int(cells[k]) and ngood[k] > 0 for k in CARRIERS)
    _judge(got, truth, "decode_acquire")
    silent = [f for k, fr in enumerate(got) if ngood[k] == 0 for f in fr]
    assert all(f["usage"] is None and f["traffic"] is None for f in silent)
    assert all(ngood[k] == 0 for k in range(len(cells)) if k not in CARRIERS)
    # the carrier without an SB is heard (descrambled with no cell: every CRC fails) and claims nothing
    assert len(got[WB_SILENT]) >= 4 and not any(f["crc_ok"] for f in got[WB_SILENT]) and int(state[WB_SILENT]) == 3
    # a cell known before the capture counts: by the default (cell_init != 3), and not when `acquired` denies it
    known = np.full(len(cells), 3, np.uint32)
    known[WB_SILENT] = cells[WB_SILENT]
    for acquired, usage in ((None, "control"), (np.zeros(len(cells), bool), None)):
        fr = rx.decode_acquire(x, known, traffic=True, timebase="vote", acquired=acquired)[0][WB_SILENT]
        assert len(fr) >= 4 and all(f["crc_ok"] and f["usage"] == usage and f["traffic"] is None for f in fr), acquired
    assert _hip.TCH_BITS == 432


def test_wideband_stream_passes_traffic_through(planted):
    from tetraear.signal.wideband import WidebandStream
    x, cells, truth = planted
    for given in (True, False):
        st = WidebandStream(cells if given else None, timebase="vote", traffic=True)
        frames = [[] for _ in cells]
        for a, b in ((0, 611_111), (611_111, 700_001), (700_001, NW)):
            for k, fr in enumerate(st.decode(x[a:b])):
                frames[k] += fr
        assert all("usage" in f and "traffic" in f for fr in frames for f in fr)
        found = {key for key, (t4, _) in truth.items() for f in frames[key[0]]
                 if f["traffic"] is not None and f["traffic"]["bits"] == len(t4) and
                 np.array_equal(T.signs(f["traffic"]["soft"]), t4)}
        # acquisition: every planted slot lies in a buffer behind the one that holds its carrier's first SB
        assert sorted(found) == sorted(truth), (given, sorted(found))
        quiet = frames[WB_SILENT]
        assert len(quiet) >= 4 and all(f["usage"] == ("control" if given else None) for f in quiet)
    assert not any("usage" in f for fr in WidebandStream(cells).decode(x[:611_111]) for f in fr)
