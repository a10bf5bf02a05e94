"""bench.py's plain run and --dump-outputs: a plain run prints the headline line without the --full
extras and writes the last timed step's outputs; the dump holds the written parts of the step's own
buffers and is the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps(tmp_path):
    C, N, steps = 256, 131072, 3
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--channels", str(C), "--samples", str(N),
           "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["full"] is False and d["steps"] == steps and d["ms_per_step"] > 0 and d["unit"] == "Msamples/s"
    assert d["higher_is_better"] is True and d["dtype"]
    want = C * N * steps / (d["ms_per_step"] * steps / 1e3) / 1e6
    assert abs(d["value"] - want) <= 1e-3 * want, (d["value"], want)
    # what takes work of its own is behind --full
    assert "cpu_baseline" not in d and "decoded_last_step" not in d
    assert "measured_read_floor_GBs" not in d["roofline"] and "traffic" not in d["roofline"]
    files = {f: np.load(out / f) for f in os.listdir(out)}
    assert {"rows.npy", "nsym.npy", "sym.npy", "soft.npy", "hard.npy", "nburst.npy", "bursts.npy", "nblock.npy",
            "blocks.npy", "type1.npy"} == set(files)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in files.values())
    assert sum(v.nbytes for v in files.values()) <= 64e6
    assert np.array_equal(files["rows.npy"], np.arange(C)) and all(len(v) == C for v in files.values())
    assert files["nblock.npy"].sum() >= 3 * C   # the chain decoded its blocks


def test_dump_is_the_steps_written_outputs_and_repeats(tmp_path, monkeypatch):
    """Two steps of the same arguments dump the same files; the rows are a fixed sample when the
    budget does not hold them all; each file holds the step's buffer rows up to the counts."""
    import torch
    sys.path.insert(0, REPO)
    import bench
    from tetraear import _hip
    from tetraear.signal.etsi import BenchStep
    dev = torch.device("cuda", 0)
    monkeypatch.setattr(bench, "DUMP_BYTES", 40 * 37000)   # ~40 of the 64 rows fit
    dumps = []
    for k in range(2):
        c = _hip.Context()
        c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
        st = BenchStep(c, 64, 131072, 2.4e6, seed=11, device=dev, cells="acquire", chunks=3).pipeline()
        for _ in range(3):
            st()
        torch.cuda.synchronize(dev)
        bench.dump_outputs(st, str(tmp_path / str(k)), dev)
        dumps.append({f: np.load(tmp_path / str(k) / f) for f in sorted(os.listdir(tmp_path / str(k)))})
    a, b = dumps
    assert list(a) == list(b) and all(np.array_equal(a[f], b[f]) for f in a)
    rows = a["rows.npy"].astype(int)
    assert 30 <= len(rows) < 64 and np.all(np.diff(rows) > 0) and rows[-1] < 64
    # against the last step's own buffers (the streaming rows start ETSI_RESERVE dibits in)
    R = _hip.ETSI_RESERVE
    sym, soft, hard, nsym = (t.cpu().numpy() for t in st.bufs[(st.k - 1) & 1])
    nk, blocks, t1 = st.nblock.cpu().numpy(), st.blocks.cpu().numpy(), st.type1.cpu().numpy()
    assert np.array_equal(a["nsym.npy"], nsym[rows]) and np.array_equal(a["nblock.npy"], nk[rows])
    for i, ch in enumerate(rows):
        n = int(nsym[ch])
        assert n > 900
        assert np.array_equal(a["sym.npy"][i, :n], sym[ch, R:R + n]) and not a["sym.npy"][i, n:].any()
        assert np.array_equal(a["hard.npy"][i, :n - 1], hard[ch, R:R + n - 1]) and not a["hard.npy"][i, n - 1:].any()
        assert np.array_equal(a["soft.npy"][i, :2 * n - 2], soft[ch, 2 * R:2 * R + 2 * n - 2])
        assert np.array_equal(a["blocks.npy"][i, :nk[ch]], blocks[ch, :nk[ch]]) and not a["blocks.npy"][i, nk[ch]:].any()
        for j in range(int(nk[ch])):   # type-1 bits per block kind; the rest of a type1 row is padding
            n1 = {0: 268, 1: 124, 2: 60}[int(blocks[ch, j, 0])]
            assert np.array_equal(a["type1.npy"][i, j, :n1], t1[ch, j, :n1]) and not a["type1.npy"][i, j, n1:].any()
        assert not a["type1.npy"][i, nk[ch]:].any()
    assert a["blocks.npy"][..., 1].sum() > len(rows)   # CRC-good blocks on every row's worth
