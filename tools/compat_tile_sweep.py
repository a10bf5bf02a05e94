#!/usr/bin/env python3
"""Rerun rate of the exact time-tiled compat decimator (tests/_tiled_model.py), on the CPU.

The tiled decimator is exact for any tile / warm-up length; a tile whose warm-started state is not
bit-identical to the sequential one is rerun.  This prints, per decimation factor and signal family
of tests/golden/_signals.py:sweep_chunks, how many checked tiles were rerun for a few (tile, warm)
pairs -- the figures the built-in defaults are chosen with.

    python tools/compat_tile_sweep.py [--seeds 4] [--chunks 10] [--pairs 8192:16384,8192:8192]
"""
import argparse
import collections
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

import _signals  # noqa: E402
import _tiled_model as model  # noqa: E402

RATES = {7: 1.8e6, 8: 2.0e6, 9: 2.2e6, 10: 2.4e6}   # q = int(fs / 240000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--chunks", type=int, default=10)
    ap.add_argument("--pairs", default="8192:16384,8192:8192,4096:16384,8192:4096")
    ap.add_argument("--q", default="7,8,9,10")
    args = ap.parse_args()
    pairs = [tuple(int(v) for v in p.split(":")) for p in args.pairs.split(",")]
    for q in (int(v) for v in args.q.split(",")):
        tot = collections.defaultdict(lambda: [0, 0])
        for seed in range(args.seeds):
            for _, fam, _, x, _ in _signals.sweep_chunks(seed, args.chunks, fs=RATES[q]):
                for tw in pairs:
                    _, st = model.decimate_tiled(x, q, *tw)
                    for key in ((tw, fam), (tw, "all")):
                        tot[key][0] += st[0] + st[2]
                        tot[key][1] += st[1] + st[3]
        for tw in pairs:
            fams = " ".join(f"{fam}={tot[(tw, fam)][1]}/{tot[(tw, fam)][0]}"
                            for fam in _signals.SWEEP_FAMILIES if (tw, fam) in tot)
            c, r = tot[(tw, "all")]
            print(f"q={q} fs={RATES[q] / 1e6:.1f}M tile={tw[0]} warm={tw[1]}: rerun {r}/{c} "
                  f"({100.0 * r / max(c, 1):.2f} %)  {fams}", flush=True)


if __name__ == "__main__":
    main()
