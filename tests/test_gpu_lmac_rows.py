"""The lower MAC's production kernels -- k_etsi_sync, k_etsi_viterbi, k_etsi_traceback, k_cell_acquire,
k_etsi_tail / tail_move -- on rows built on the CPU (tests/_lmac_rows.py), with no demodulator in
front: bursts at the scan's thresholds and edges, and soft bits chosen to break the trellis.

Bar: bit-identical to the C oracle (oracle/etsi.py Receiver.sync / sync_from / decode_block /
lower_mac / lower_mac_acquire and the streaming hand-off LmacStream) -- nburst, every burst's
(start, kind), nblock, every block's (kind, crc_ok, burst, index) and its type-1 bits, CRC-bad blocks
included; where the oracle itself could be wrong, the independent restatement oracle/etsi_spec.py
(maximum likelihood of every CRC-good decode) and the component decoder tetra_etsi_decode_blocks
(another kernel) are held against both.  Integer and bit-exact: no tolerance anywhere.
tests/test_lmac_rows.py proves on the CPU that the rows mean what is assumed here.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import etsi as E
import etsi_spec as S
import _lmac_rows as R

pytestmark = pytest.mark.gpu

N, P, SB = R.NDB_N, R.NDB_P, R.SB
SMAX = 2050   # the widest row tetra_lmac_etsi takes


# ------------------------------------------------------------------------------ scan thresholds

def test_scan_thresholds():
    """Bursts with TOTAL - THRESH scored bits flipped (found) and one more (not found), random and
    with the flips kept in the head, the tail with bit 509, y's last six bits and the n / p
    difference: one batch; the oracle's answer and the known one."""
    cases = R.threshold_rows(1, 7)
    assert len(cases) <= 64
    hard, soft, nsym = R.pack_rows([(b, R.soft_of(b)) for b, _, _, _ in cases], 801)
    cells = np.full(len(cases), 3, np.uint32)
    out = R.run_lmac(hard, soft, nsym, cells)
    R.assert_rows_equal(out, R.oracle_rows(hard, soft, nsym, cells), "thresholds")
    for ch, (_, off, kind, found) in enumerate(cases):
        nb = int(out["nburst"][ch])
        assert nb == int(found), (ch, off, kind, found, nb)
        if found:
            assert tuple(out["bursts"][ch, 0]) == (off, kind), (ch, off, kind)


# ------------------------------------------------------------------------------ scan geometry

@functools.lru_cache(maxsize=None)
def _geometry():
    """[(name, bits, nsym, known bursts or None)] and the cell the blocks are scrambled with."""
    rng = np.random.default_rng(40)
    cell = R.random_cell(rng)
    scr = E.scramble_seq(cell, 432)
    cases = []

    def row(name, nbits, plants, known="planted", nsym=None):
        bits = rng.integers(0, 2, max([nbits] + [o + 510 for o, _ in plants])).astype(np.uint8)
        for off, kind in plants:
            R.plant(bits, off, E.make_burst(kind, rng, scr)[0])
        cases.append((name, bits[:nbits], nbits // 2 + 1 if nsym is None else nsym,
                      list(plants) if known == "planted" else known))

    row("bit 0", 1200, [(0, N)])
    row("last legal start", 1400, [(890, P)])
    row("one past the last start", 1400, [(891, N)], [])
    for off, kind in ((1, SB), (37, N), (511, P), (889, SB)):
        row("odd bit %d" % off, 1400, [(off, kind)])
    for i, off in enumerate((63, 64, 65, 127, 128)):
        row("lane %d of the scan window" % off, 1200, [(off, (N, P, SB)[i % 3])])
    for i, off in enumerate((563, 564, 565)):   # the scan resumes at 500: lanes 63, 64, 65 again
        row("lane %d after a burst" % (off - 500), 1300, [(0, (P, SB, N)[i]), (off, (N, P, SB)[i])])
    row("510 apart", 1300, [(10, N), (520, SB)])
    row("500 apart, second written last", 1300, [(10, N), (510, P)], None)
    row("500 apart, first written last", 1300, [(510, P), (10, N)], None)
    row("254 dibits", 508, [(0, N)], [])
    row("255 dibits", 510, [(0, N)])
    row("256 dibits", 512, [(0, P)])
    row("256 dibits, bit 1", 512, [(1, N)])
    row("256 dibits, bit 2", 512, [(2, SB)])
    row("full table", 4098, [(510 * i, (P, SB)[i & 1]) for i in range(8)])
    row("full table to bit 4096", 4098, [(16 + 510 * i, (SB, P)[i & 1]) for i in range(8)])
    row("full table to the row's last bit", 4098, [(18 + 510 * i, (P, N, SB)[i % 3]) for i in range(8)])
    row("nsym 0", 0, [], [], nsym=0)
    row("nsym 1", 0, [], [], nsym=1)
    row("no burst", 4096, [], [])
    row("nsym 0 beside a row of bits", 1200, [(0, N)], [], nsym=0)
    rx = E.Receiver()
    want = []
    for name, bits, nsym, known in cases:
        nd = max(nsym - 1, 0)
        w = rx.lower_mac(R.soft_of(bits[:2 * nd]), R.hard_of(bits[:2 * nd]), cell)
        if known is not None:   # the fixture means what it says
            assert [(s, k) for s, k, _ in w] == known, (name, w, known)
        want.append(w)
    return cases, want, cell


@pytest.mark.parametrize("C", [1, 5, 7, 64])
def test_scan_geometry(C):
    """Each case its own channel: bit 0, the last legal start and one past it, odd bits, lanes 63 / 64
    / 65 / 127 / 128 of the scan window, bursts 510 and 500 apart, rows of 254 / 255 / 256 dibits,
    the full burst table (8 bursts, 16 blocks), nsym 0 and 1 -- in batches that fill SYNC_WAVES and
    leave it partly empty."""
    cases, want, cell = _geometry()
    sel = [(i + C) % len(cases) for i in range(C)]
    hard = np.zeros((C, SMAX), np.uint8)
    soft = np.zeros((C, 2 * SMAX), np.int8)
    nsym = np.zeros(C, np.int32)
    for ch, i in enumerate(sel):
        name, bits, ns, known = cases[i]
        hard[ch, :len(bits) // 2] = R.hard_of(bits)
        soft[ch, :len(bits)] = R.soft_of(bits)
        nsym[ch] = ns
    out = R.run_lmac(hard, soft, nsym, np.full(C, cell, np.uint32))
    for ch, i in enumerate(sel):
        one = {k: v[ch:ch + 1] for k, v in out.items()}
        R.assert_rows_equal(one, [want[i]], cases[i][0])
    if C == 64:
        full = [ch for ch, i in enumerate(sel) if cases[i][0].startswith("full table")]
        assert len(full) >= 3 and all(out["nburst"][ch] == 8 for ch in full)
        assert max(int(out["nblock"][ch]) for ch in full) == 16
        assert all(bool(b[1]) for ch in range(C) for b in out["blocks"][ch, :out["nblock"][ch]]
                   if "500 apart" not in cases[sel[ch]][0])   # clean rows: every block CRC-good


# ------------------------------------------------------------------------------ production Viterbi

@functools.lru_cache(maxsize=None)
def _viterbi(wmod):
    b = R.viterbi_batch(100 + wmod, 64, wmod)
    want = R.oracle_rows(b["hard"], b["soft"], b["nsym"], b["cells"])
    out = R.run_lmac(b["hard"], b["soft"], b["nsym"], b["cells"])
    return b, want, out


@pytest.mark.parametrize("wmod", [0, 1, 2, 3])
def test_production_viterbi_on_adversarial_soft_bits(wmod):
    """Every block kind at every start bit mod 4 on rows of width mod 4 = wmod (every byte alignment
    of load_seg's segments), the soft bits of each block of one class: +-127, -128 mixed in, all zero
    (every ACS a tie), {-1, 0, 1}, uniform, signs inverted against the hard bits, Gaussian.
    Bit-identical to the oracle; the clean class returns the payload; every CRC-good Gaussian decode
    is at least as likely as the transmitted codeword (oracle/etsi_spec.py); the component decoder
    (k_decode_blocks) gives the same bits on the blocks cut out."""
    from tetraear import _hip
    b, want, out = _viterbi(wmod)
    assert b["hard"].shape[1] % 4 == wmod
    R.assert_rows_equal(out, want, "viterbi")
    per_kind = {0: [], 1: [], 2: []}
    good = {}
    for ch, blocks in enumerate(b["blocks"]):
        assert int(out["nburst"][ch]) == 3 and int(out["nblock"][ch]) == len(blocks)
        for j, (start, bk, kind, fields, cls, t1, tx) in enumerate(blocks):
            got, ok = out["type1"][ch, j, :len(t1)], bool(out["blocks"][ch, j, 1])
            assert int(out["blocks"][ch, j, 0]) == kind
            soft5 = R.block_soft(b["soft"][ch], start, fields)
            init = 3 if kind == 2 else int(b["cells"][ch])
            per_kind[kind].append((ch, j, soft5, init))
            if cls == "clean":
                assert ok and np.array_equal(got, t1), (ch, j)
            if cls == "zero":
                assert not ok and not got.any(), (ch, j)
            if cls == "inverted":   # the scan read the hard bits, the trellis the soft bits
                assert not ok and not np.array_equal(got, t1), (ch, j)
            if cls == "gauss":
                n, g = good.get(kind, (0, 0))
                good[kind] = (n + 1, g + ok)
                if ok:
                    m_got = S.codeword_metric(soft5, S.type2(got), kind, init)
                    m_sent = S.codeword_metric(soft5, S.type2(t1), kind, init)
                    assert m_got >= m_sent, (ch, j, m_got, m_sent)
    print("Gaussian class (blocks, CRC-good) per kind:", good)
    for kind, (n, g) in good.items():   # the oracle's share (tests/test_lmac_rows.py), here the GPU's
        assert 0.25 <= g / n <= 0.75, (kind, n, g)
    c = _hip.ctx()
    for kind, items in per_kind.items():   # production kernel = component kernel (= oracle, above)
        F, n1 = len(items), E.KIND_PARAMS[kind][3]
        soft5 = np.ascontiguousarray(np.stack([it[2] for it in items]), np.int8)
        inits = np.array([it[3] for it in items], np.uint32)
        dec = np.zeros((F, n1), np.uint8)
        ok = np.zeros(F, np.uint8)
        c.check(c.lib.tetra_etsi_decode_blocks(c.handle, _hip.ptr(soft5), F, kind, _hip.ptr(inits), _hip.ptr(dec),
                                               _hip.ptr(ok)), "tetra_etsi_decode_blocks")
        for f, (ch, j, _, _) in enumerate(items):
            assert np.array_equal(dec[f], out["type1"][ch, j, :n1]) and int(ok[f]) == int(out["blocks"][ch, j, 1]), \
                (kind, ch, j)


_CHILD = """
import sys
sys.path[:0] = sys.argv[2:]
import numpy as np
import _lmac_rows as R
b = R.viterbi_batch(100, 64, 0)
out = R.run_lmac(b["hard"], b["soft"], b["nsym"], b["cells"])
for k, v in out.items():
    np.save(sys.argv[1] + "/" + k + ".npy", v)
"""


def test_grid_cap_walks_the_jobs(tmp_path):
    """TETRA_LMAC_GRID_CAP=3 (read once per process, so in a fresh child process): three trellis
    workgroups and one traceback workgroup walk the C = 64 batch's 20 + 5 wave-batches with the
    grid stride and give the uncapped call's outputs."""
    b, want, out = _viterbi(0)
    env = dict(os.environ, TETRA_LMAC_GRID_CAP="3")
    paths = [p for p in sys.path if p and os.path.isdir(p)]
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", _CHILD, str(tmp_path)] + paths, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    capped = {k: np.load(tmp_path / (k + ".npy")) for k in out}
    assert R.live_outputs(capped) == R.live_outputs(out)
    assert int(out["nblock"].sum()) == 64 * 5


# ------------------------------------------------------------------------------ cell acquisition

def _noise_field(rng, soft, start, off, n):
    soft[start + off:start + off + n] = rng.integers(-127, 128, n).astype(np.int8)


def test_cell_acquisition_on_built_rows():
    """tetra_lmac_etsi_acquire against lower_mac_acquire, cell_init in and out: one sync burst with
    normal bursts of its cell before and after it (all decode); two sync bursts of cells A then B (B
    wins, blocks scrambled with A fail); a sync burst whose BSCH is noise (the incoming cell stays);
    then a second call on the same context where only the even channels change cell."""
    rng = np.random.default_rng(60)
    rx = E.Receiver()
    rows, inits, cellsA, cellsB = [], [], [], []
    for rep in range(2):
        (A, fA), (B, fB) = R.cell_fields(rng), R.cell_fields(rng)
        for scen in range(5):
            if scen == 0:
                items, init = [(7, N, A, None), (3, SB, A, R.sync_payloads(rng, fA)), (0, P, A, None),
                               (64, N, A, None)], 3
            elif scen == 1:
                items, init = [(0, N, A, None), (1, SB, A, R.sync_payloads(rng, fA)), (0, P, A, None),
                               (5, SB, B, R.sync_payloads(rng, fB)), (0, N, A, None)], 3
            elif scen == 2:
                items, init = [(2, N, A, None), (0, SB, A, R.sync_payloads(rng, fB)), (9, P, A, None)], A
            elif scen == 3:
                items, init = [(1, P, A, None), (0, N, A, None)], A
            else:
                items, init = [(300, SB, A, R.sync_payloads(rng, fA))], 3
            bits, planted, jobs = R.place_bursts(rng, items, tail_gap=4 * scen)
            soft = R.soft_of(bits)
            if scen == 2:
                _noise_field(rng, soft, planted[1][0], 94, 120)
            rows.append((bits, soft))
            inits.append(init)
            cellsA.append(A)
            cellsB.append(B)
    C = len(rows)
    hard, soft, nsym = R.pack_rows(rows, max(len(b) for b, _ in rows) // 2 + 3)
    cell_init = np.array(inits, np.uint32)
    out = R.run_lmac(hard, soft, nsym, cell_init=cell_init)
    want, state = [], []
    for ch in range(C):
        nd = int(nsym[ch]) - 1
        w, init = rx.lower_mac_acquire(soft[ch, :2 * nd], hard[ch, :nd], inits[ch])
        want.append(w)
        state.append(init)
    R.assert_rows_equal(out, want, "acquire")
    assert cell_init.tolist() == state
    for ch in range(C):   # the known answers
        scen, ok = ch % 5, [bool(o) for _, _, dec in want[ch] for _, _, o in dec]
        assert state[ch] == (cellsB[ch] if scen == 1 else cellsA[ch]), (ch, scen)
        if scen in (0, 3, 4):
            assert all(ok), (ch, scen, ok)
        if scen == 1:   # BSCH of A, BSCH of B and B's SCH/HD pass; everything scrambled with A fails
            assert ok == [False, True, False, False, False, True, True, False], (ch, ok)
        if scen == 2:   # the noise BSCH fails, the rest decodes with the cell that came in
            assert ok == [True, False, True, True, True], (ch, ok)
    # second call, same context and channel count: even channels hear a new cell, odd ones keep theirs
    rows2, news = [], []
    for ch in range(C):
        if ch % 2 == 0:
            Z, fZ = R.cell_fields(rng)
            items = [(5, SB, Z, R.sync_payloads(rng, fZ)), (0, N, Z, None)]
            news.append(Z)
        else:
            items = [(3, N, state[ch], None), (0, P, state[ch], None)]
            news.append(state[ch])
        bits, _, _ = R.place_bursts(rng, items)
        rows2.append((bits, R.soft_of(bits)))
    hard, soft, nsym = R.pack_rows(rows2, hard.shape[1])
    before = cell_init.copy()
    out = R.run_lmac(hard, soft, nsym, cell_init=cell_init)
    want = []
    for ch in range(C):
        nd = int(nsym[ch]) - 1
        w, init = rx.lower_mac_acquire(soft[ch, :2 * nd], hard[ch, :nd], int(before[ch]))
        want.append(w)
        assert init == news[ch] == int(cell_init[ch]), ch
        assert all(o for _, _, dec in w for _, _, o in dec), ch
    R.assert_rows_equal(out, want, "acquire, second call")


# ------------------------------------------------------------------------------ streaming

FIELD_CUTS = (6, 250, 100, 400, 505, -2, 2)   # head, training sequence, blocks 1 and 2, tail, a dibit either side


def _run_stream(chans, alias, acquire=False):
    """tetra_lmac_etsi_stream chunk by chunk against LmacStreamModel.  chans: [(hard, soft, cuts,
    cell init)]; alias: the next rows are the input rows (k_etsi_tail), else a second pair (the tail
    moves inside k_etsi_sync).  Returns per channel the bursts found as (stream bit, kind), the number
    that began in a carried tail with the number of chunks that stopped on an odd bit, and the models."""
    from tetraear import _hip
    c = _hip.ctx()
    C, RES, stride = len(chans), _hip.ETSI_RESERVE, SMAX
    assert RES == E.RESERVE
    rx = E.Receiver()
    bufs = [(np.zeros((C, 2 * stride), np.int8), np.zeros((C, stride), np.uint8)) for _ in range(1 if alias else 2)]
    lead = np.full(C, 2 * RES, np.int32)
    models = [R.LmacStreamModel(rx, None if acquire else ch[3]) for ch in chans]
    cell_init = np.full(C, 3, np.uint32) if acquire else None
    if not acquire:
        cells = np.array([ch[3] for ch in chans], np.uint32)
        c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(cells), C), "tetra_etsi_set_cells")
    found, seams, odd = [[] for _ in chans], 0, 0
    for k in range(max(len(ch[2]) for ch in chans) + 1):   # one more: an empty chunk for every channel
        soft, hard = bufs[k % len(bufs)]
        nsoft, nhard = bufs[(k + 1) % len(bufs)]
        nsym = np.ones(C, np.int32)
        new = []
        for ch, (h, s, cuts, _) in enumerate(chans):
            at, n = cuts[k] if k < len(cuts) else (len(h), 0)
            hard[ch, RES:RES + n] = h[at:at + n]
            soft[ch, 2 * RES:2 * (RES + n)] = s[2 * at:2 * (at + n)]
            nsym[ch] = n + 1
            new.append((at, h[at:at + n], s[2 * at:2 * (at + n)]))
        o = R.lmac_outputs(C)
        c.check(c.lib.tetra_lmac_etsi_stream(c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(nsym), C, stride,
                                             _hip.ptr(lead), _hip.ptr(nsoft), _hip.ptr(nhard),
                                             _hip.ptr(cell_init), _hip.ptr(o["nburst"]), _hip.ptr(o["bursts"]),
                                             _hip.ptr(o["nblock"]), _hip.ptr(o["blocks"]), _hip.ptr(o["type1"])),
                "tetra_lmac_etsi_stream")
        want = []
        for ch, (at, nh, ns) in enumerate(new):
            m = models[ch]
            r = m.push(nh, ns)
            want.append(r["bursts"])
            T = len(m.tail_hard)
            assert int(lead[ch]) == 2 * (RES - T) + m.phase, (k, ch, int(lead[ch]), T, m.phase)
            assert np.array_equal(nhard[ch, RES - T:RES], m.tail_hard), (k, ch)
            assert np.array_equal(nsoft[ch, 2 * (RES - T):2 * RES], m.tail_soft), (k, ch)
            if acquire:
                assert int(cell_init[ch]) == r["cell"], (k, ch)
            found[ch] += [(2 * at + pos, kind) for pos, kind, _ in r["bursts"]]
            seams += sum(pos < 0 for pos, _, _ in r["bursts"])
            odd += m.phase
        R.assert_rows_equal(o, want, "stream chunk %d" % k)
    return found, (seams, odd), models


@functools.lru_cache(maxsize=None)
def _stream_channels():
    """8 of the CPU test's streams: four cut inside the head, the training sequence, the first and
    second block and the tail of their bursts and one dibit either side of a burst start, four cut
    into chunks of CHUNKS dibits."""
    chans, planted_all = [], []
    for i in range(8):
        bits, planted, jobs, cell = R.burst_stream(i)
        hard, soft = R.hard_of(bits), R.soft_of(bits)
        if i < 4:
            cuts = R.cuts_at(len(hard), [(s + FIELD_CUTS[(i + j) % len(FIELD_CUTS)]) // 2
                                         for j, (s, _) in enumerate(planted)])
        else:
            cuts = R.chunk_cuts(i, len(hard))
        assert max(n for _, n in cuts) + E.RESERVE <= SMAX - 1
        chans.append((hard, soft, cuts, cell))
        planted_all.append(planted)
    return chans, planted_all


@pytest.mark.parametrize("alias", [True, False], ids=["same_rows", "other_rows"])
def test_stream_hand_off(alias):
    """Per chunk: lead, the carried tail's dibits and soft bits, the burst starts (negative ones
    included) and the blocks equal LmacStreamModel's; over all chunks every planted burst is found
    exactly once."""
    chans, planted = _stream_channels()
    found, (seams, odd), _ = _run_stream(list(chans), alias)
    assert found == planted
    # bursts that began in a carried tail; chunks whose scan stopped on an odd bit
    assert seams >= 20 and odd >= 10, (seams, odd)


def test_stream_acquires_from_a_sync_burst_across_a_cut():
    """Acquisition over streaming rows: the sync burst is whole only with the carried tail in front of
    the next chunk; the cell comes from it and the bursts after it decode."""
    rng = np.random.default_rng(70)
    chans, cells = [], []
    for off in (150, 230, 400):   # the cut in the BSCH block, in the sync sequence, in block 2
        A, fA = R.cell_fields(rng)
        bits, planted, jobs = R.place_bursts(rng, [(3, N, A, None), (0, SB, A, R.sync_payloads(rng, fA)),
                                                   (1, N, A, None), (0, P, A, None)])
        hard = R.hard_of(bits)
        chans.append((hard, R.soft_of(bits), R.cuts_at(len(hard), [(planted[1][0] + off) // 2]), A))
        cells.append((A, planted))
    found, (seams, _), models = _run_stream(chans, True, acquire=True)
    assert found == [p for _, p in cells] and seams >= 3
    assert [m.cell for m in models] == [a for a, _ in cells]
