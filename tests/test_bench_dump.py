"""bench.py --dump-outputs on the CPU: the row selection keeps only what a step wrote (its buffers are
torch.empty, so padding must not reach a file), and the new options parse with their defaults off."""
import sys
import types

import numpy as np
import torch

import bench
from tetraear import _hip


def test_options_default_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.no_cpu is True and a.dump_outputs == "d"


def test_demod_rows_keep_the_written_part_only():
    C, L, off = 5, 12, 3
    nsym = torch.tensor([0, 1, 7, L - off, 4], dtype=torch.int32)
    sym = torch.full((C, L, 2), float("nan"))
    soft = torch.full((C, 2 * L), -7, dtype=torch.int8)
    hard = torch.full((C, L), 9, dtype=torch.uint8)
    for ch, n in enumerate(nsym.tolist()):
        sym[ch, off:off + n] = ch + 1.0
        soft[ch, 2 * off:2 * off + 2 * max(n - 1, 0)] = 5
        hard[ch, off:off + max(n - 1, 0)] = 2
    r = torch.tensor([4, 0, 2, 3, 1])
    out = bench._demod_rows(r, sym, soft, hard, nsym, off)
    assert out["nsym"].tolist() == [4, 0, 7, L - off, 1]
    for i, ch in enumerate(r.tolist()):
        n = int(nsym[ch])
        want = np.zeros((L - off, 2), np.float32)
        want[:n] = ch + 1.0
        assert np.array_equal(out["sym"][i].numpy(), want)   # no NaN from the padding
        assert out["hard"][i].tolist() == [2] * max(n - 1, 0) + [0] * (L - off - max(n - 1, 0))
        assert out["soft"][i].tolist() == [5] * (2 * max(n - 1, 0)) + [0] * (2 * (L - off) - 2 * max(n - 1, 0))


def test_lmac_rows_mask_blocks_and_type1_bits():
    C, J, B = 3, _hip.ETSI_MAXJ, _hip.ETSI_MAXB
    g = torch.Generator().manual_seed(1)
    step = types.SimpleNamespace(
        nburst=torch.tensor([0, 2, B], dtype=torch.int32), nblock=torch.tensor([0, 3, J], dtype=torch.int32),
        bursts=torch.randint(1, 1000, (C, B, 2), generator=g, dtype=torch.int32),
        blocks=torch.randint(3, 1 << 30, (C, J, 4), generator=g, dtype=torch.int32),   # padding: no valid kind
        type1=torch.full((C, J, 268), 1, dtype=torch.uint8))
    step.blocks[1, :3, 0] = torch.tensor([0, 1, 2], dtype=torch.int32)
    step.blocks[2, :, 0] = 1
    out = bench._etsi_lmac_rows(step, torch.arange(C))
    assert not out["bursts"][0].any() and not out["blocks"][0].any() and not out["type1"][0].any()
    assert torch.equal(out["bursts"][1, :2], step.bursts[1, :2]) and not out["bursts"][1, 2:].any()
    assert torch.equal(out["blocks"][1, :3], step.blocks[1, :3]) and not out["blocks"][1, 3:].any()
    assert out["type1"][1].sum(-1).tolist() == [268, 124, 60] + [0] * (J - 3)
    assert torch.equal(out["bursts"][2], step.bursts[2]) and out["type1"][2].sum(-1).tolist() == [124] * J
