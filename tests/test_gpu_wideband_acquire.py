"""The wideband chain acquiring every carrier's cell from its own BSCH (WidebandReceiver.decode_acquire,
WidebandStream(cells=None), mac=True, BenchStep with TETRA_WB_CELLS=acquire) on one synthetic capture
of three timing chunks per carrier.  The reference is the existing given-cells path on the same
capture: a carrier that heard a CRC-good BSCH must decode exactly as with its cell given, any other
exactly as with the unknown cell (init 3).  Bit-exact: no tolerance anywhere.
"""
import numpy as np
import pytest

import _etsi_mac_model as MM

pytestmark = pytest.mark.gpu

NW = 3_300_000
PIECES = ((0, 1_234_567), (1_234_567, 1_300_001), (1_300_001, 2_711_113), (2_711_113, NW))


@pytest.fixture(scope="module")
def capture3():
    from tetraear.signal.wideband import synth_wideband
    return synth_wideband(NW, seed=17, snr_db=25.0, cfo_max=300.0)   # three timing chunks per carrier


def view(f, key="sample"):
    """A frame as plain values (bits as bytes), for equality."""
    return (f[key], f["position"], f["burst_kind"], f["chunk"], f["crc_ok"],
            [(b["channel"], b["crc_ok"], b["block"], b["bits"].tobytes()) for b in f["blocks"]])


def heard(frames):
    """Per carrier: a frame holds a CRC-good BSCH block."""
    return np.array([any(b["channel"] == "BSCH" and b["crc_ok"] for f in fr for b in f["blocks"]) for fr in frames])


@pytest.fixture(scope="module")
def decoded(capture3):
    """The capture decoded with the cells given, with every cell unknown, and acquiring (mac=True)."""
    from tetraear.signal.wideband import WidebandReceiver
    x, cells = capture3[0], capture3[1]
    rx = WidebandReceiver()
    unknown = np.full(len(cells), 3, np.uint32)
    given = rx.decode(x, cells)
    blind = rx.decode(x, unknown)
    got, state, ngood = rx.decode_acquire(x, unknown, mac=True)
    assert unknown.tolist() == [3] * len(cells)   # the caller's array is not written
    return given, blind, got, state, ngood


def test_decode_acquire_equals_given_cells_where_a_bsch_was_heard(capture3, decoded):
    cells = capture3[1]
    given, blind, got, state, ngood = decoded
    assert state.dtype == np.uint32 and ngood.dtype == np.int32 and len(state) == len(ngood) == len(cells)
    first = heard(given)
    print("carriers that heard a CRC-good BSCH: %d of %d (%.3f)" % (first.sum(), len(cells), first.mean()))
    assert first.any()
    for k in range(len(cells)):
        if first[k]:
            assert int(state[k]) == int(cells[k]) and ngood[k] > 0, k
            assert [view(f) for f in got[k]] == [view(f) for f in given[k]], k
        else:
            assert int(state[k]) == 3 and ngood[k] == 0, k
            assert [view(f) for f in got[k]] == [view(f) for f in blind[k]], k
    # acquisition is what decodes: with the cell unknown the SCH blocks of these carriers fail
    k = int(np.flatnonzero(first)[0])
    assert sum(b["crc_ok"] for f in got[k] for b in f["blocks"]) > sum(b["crc_ok"] for f in blind[k] for b in f["blocks"])


def test_decode_acquire_keeps_a_state_handed_in(capture3, decoded):
    """A second capture's worth: the state handed in is what carriers without a BSCH decode with."""
    from tetraear.signal.wideband import WidebandReceiver
    x, cells = capture3[0], capture3[1]
    given = decoded[0]
    got, state, ngood = WidebandReceiver().decode_acquire(x, cells)
    assert state.tolist() == cells.tolist()
    for k in (0, 1, 399, 400, 799):
        assert [view(f) for f in got[k]] == [view(f) for f in given[k]], k
        assert set(got[k][0]) == {"position", "burst", "burst_kind", "timeslot", "blocks", "crc_ok", "chunk", "sample"}
    with pytest.raises(ValueError):
        WidebandReceiver().decode_acquire(x, cells[:5])


def test_mac_attaches_pdus_and_no_timebase(decoded):
    """mac=True: every block carries npdu / pdus -- for a CRC-good block the dicts of the model's walk
    of its type-1 bits (tests/_etsi_mac_model.py), for a CRC-bad one none -- and no frame carries tn /
    fn / mn."""
    from tetraear.core.etsi import pdu_dict
    got = decoded[2]
    kinds = {"SCH/F": 0, "SCH/HD": 1, "BSCH": 2}
    ngood = nsync = 0
    for fr in got:
        for f in fr:
            assert not {"tn", "fn", "mn", "slot_flags"} & set(f)
            for b in f["blocks"]:
                if not b["crc_ok"]:
                    assert b["npdu"] == 0 and b["pdus"] == []
                    continue
                recs = MM.walk(b["bits"], kinds[b["channel"]])
                assert b["npdu"] == len(recs), (f["sample"], b["channel"])
                assert b["pdus"] == [pdu_dict(r) for r in recs[:MM.MAXPDU]], (f["sample"], b["channel"])
                ngood += 1
                nsync += b["channel"] == "BSCH"
    assert ngood > 1000 and nsync > 100, (ngood, nsync)


def test_stream_acquires_and_carries_the_cells(capture3):
    """WidebandStream() over four pieces against WidebandStream(cells) and WidebandStream(all 3) over
    the same pieces.  After each piece a carrier's state is its cell exactly when some buffer so far
    held a CRC-good BSCH for it (the given-cells stream's buffers, before its duplicates are dropped);
    a carrier acquired by the end of a piece emits that piece's frames of the given-cells stream, one
    not yet acquired those of the all-3 stream; no burst is emitted twice; reset() clears the state."""
    from tetraear.core.etsi import cell_of
    from tetraear.signal import wideband as WB
    x, cells = capture3[0], capture3[1]
    M = len(cells)
    st, sg, sb = WB.WidebandStream(), WB.WidebandStream(cells), WB.WidebandStream(np.full(M, 3, np.uint32))
    assert st.cells == [None] * M and sg.cells is not None and np.array_equal(sg.cells, cells)
    raw = []   # the given-cells stream's buffers as decoded, duplicates included
    inner = sg.rx.decode
    sg.rx.decode = lambda buf, c, **kw: raw.append(inner(buf, c, **kw)) or raw[-1]
    known = np.zeros(M, bool)
    emitted = [[] for _ in range(M)]
    late = 0
    for a, b in PIECES:
        fa, fg, fb = st.decode(x[a:b]), sg.decode(x[a:b]), sb.decode(x[a:b])
        was = known.copy()
        known |= heard(raw[-1])
        assert np.array_equal(st.acquired, known)
        assert np.array_equal(st.cell_state, np.where(known, cells, 3).astype(np.uint32))
        for k in range(M):
            want = fg[k] if known[k] else fb[k]
            assert [view(f, "stream_sample") for f in fa[k]] == [view(f, "stream_sample") for f in want], (a, k)
            emitted[k] += [f["stream_sample"] for f in fa[k]]
        late += int((known & ~was).sum()) if a else 0
    # a carrier's row holds at least 10 whole slots, a quarter of the synthesised bursts are
    # synchronisation bursts: 0.75^10 = 6 % of the carriers hear none (0.8: far below the 94 % expected)
    assert len(raw) == len(PIECES) and known.sum() > 0.8 * M
    assert late > 0   # some carriers heard their first BSCH after the first piece: the state was carried to it
    for k in range(M):
        assert all(q - p > st.tol for p, q in zip(emitted[k], emitted[k][1:])), k
    assert st.cells == [cell_of(c) if a else None for c, a in zip(cells, known)]
    st.reset()
    assert st.cells == [None] * M and st.cell_state.tolist() == [3] * M and not st.acquired.any()


def _bench_outputs(st):
    import torch
    torch.cuda.synchronize(st.x.device)
    return [t.cpu().numpy() for t in (st.nburst, st.bursts, st.nblock, st.blocks, st.type1)]


@pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])
def test_bench_step_acquires(pipelined, monkeypatch):
    """bench.py's wideband step with TETRA_WB_CELLS=acquire: for the carriers that acquired, nburst,
    bursts, nblock, blocks and the live type-1 bits equal the default (given-cells) step's;
    quality()["cells_acquired"] is their count; the default step reports neither key nor attribute."""
    import torch
    from tetraear import _hip
    from tetraear.signal.wideband import BenchStep
    dev = torch.device("cuda", 0)
    steps = []
    for mode in (None, "acquire"):
        if mode is None:
            monkeypatch.delenv("TETRA_WB_CELLS", raising=False)
        else:
            monkeypatch.setenv("TETRA_WB_CELLS", mode)
        c = _hip.Context()
        c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
        st = BenchStep(c, NW, seed=3, device=dev)
        if pipelined and mode:
            st.pipeline()
        for _ in range(2 if mode else 1):   # the second step runs on the state the first one left
            st()
        steps.append(st)
    ref, acq = steps
    assert not hasattr(ref, "cells_mode") and "cells_acquired" not in ref.quality()
    assert acq.cells_mode == "acquire" and acq.nchunk == 3
    assert acq.config(1)["cells"] == "acquire" and "cells" not in ref.config(1)   # the bench line's config
    want, got = _bench_outputs(ref), _bench_outputs(acq)
    state, true = acq.cell_state.cpu().numpy(), acq.cells_true.cpu().numpy()
    ok = state == true
    assert np.all(state[~ok] == 3) and np.array_equal(acq.ngood.cpu().numpy() > 0, ok)
    q = acq.quality()
    print("cells_acquired %d of %d; crc_ok %d of %d blocks (given cells: %d)" %
          (q["cells_acquired"], len(ok), q["crc_ok"], q["blocks"], ref.quality()["crc_ok"]))
    assert q["cells_acquired"] == int(ok.sum()) > 0.8 * len(ok)   # 94 % expected, as in the stream test
    n1 = {0: 268, 1: 124, 2: 60}
    for k in np.flatnonzero(ok):
        for ch in range(k * acq.nchunk, (k + 1) * acq.nchunk):
            nb, nk = int(want[0][ch]), int(want[2][ch])
            assert (int(got[0][ch]), int(got[2][ch])) == (nb, nk), ch
            assert np.array_equal(got[1][ch, :nb], want[1][ch, :nb]) and np.array_equal(got[3][ch, :nk], want[3][ch, :nk]), ch
            for j in range(nk):
                n = n1[int(want[3][ch, j, 0])]
                assert np.array_equal(got[4][ch, j, :n], want[4][ch, j, :n]), (ch, j)
