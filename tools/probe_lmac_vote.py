#!/usr/bin/env python3
"""The cell vote against last-good-BSCH acquisition on the bench steps (tetra_profile's HIP events, one
context, the stages one after another): the etsi_acquire stage -- BSCH trellis, its traceback and
k_cell_vote_groups or k_cell_acquire(_groups) -- with the vote and without, alternating in one
session on one step object, whose lower-MAC call is switched between runs; then the decoded work of
either (bursts, blocks, CRC-good blocks summed over a run's steps) and the scores the vote reached.
usage: probe_lmac_vote.py wideband [samples] [runs] [steps]    (7200 rows, G = 9 at 10 M samples)
       probe_lmac_vote.py narrowband [channels] [runs] [steps] (streaming, a run = the capture once)
"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tetraear-bladerf_amd"), REPO]


def read_profile(c):
    names = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 64)()
    n = ctypes.c_int(0)
    c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    raw = names.raw.split(b"\0")
    return {raw[i].decode(): (ms[i], int(cnt[i])) for i in range(n.value)}


def main():
    import torch
    from tetraear import _hip
    shape = sys.argv[1] if len(sys.argv) > 1 else "wideband"
    size = int(sys.argv[2]) if len(sys.argv) > 2 else (10_000_000 if shape == "wideband" else 8192)
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    steps = int(sys.argv[4]) if len(sys.argv) > 4 else (8 if shape == "wideband" else 4)
    dev = torch.device("cuda", 0)
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    if shape == "wideband":
        os.environ["TETRA_WB_CELLS"] = "vote"
        from tetraear.signal.wideband import BenchStep
        st = BenchStep(c, size, seed=1, device=dev)
        rows, G, true = st.C, st.nchunk, st.cells_true
    else:
        from tetraear.signal.etsi import BenchStep
        st = BenchStep(c, size, 131072, 2.4e6, 1, dev, cells="acquire", chunks=steps, vote=True)
        rows, G, true = st.C, 1, st.cells
    live = torch.arange(_hip.ETSI_MAXJ, device=dev)[None, :]

    def run(vote, n):
        """n steps with the vote or without: (stage ms per step, decoded work summed over the steps)."""
        st.vote = vote
        c.check(c.lib.tetra_profile(c.handle, 1), "profile")
        read_profile(c)
        work = torch.zeros(4, dtype=torch.int64, device=dev)
        for _ in range(n):
            st()
            c.synchronize()
            k = live < st.nblock[:, None]
            good = k & (st.blocks[:, :, 1] != 0)
            work += torch.stack([st.nburst.sum(), st.nblock.sum(), good.sum(), (good & (st.blocks[:, :, 0] == 2)).sum()])
        prof = read_profile(c)
        c.check(c.lib.tetra_profile(c.handle, 0), "profile")
        return {k: ms / n for k, (ms, _) in prof.items()}, work.tolist()

    run(False, steps)   # warm-up: workspaces, the cells acquired (both modes then start from the same state)
    run(True, steps)
    first = None
    if shape == "wideband":   # a fresh state: what one step's ballots weigh
        st.cell_state.fill_(3)
        st.cell_score.zero_()
        run(True, 1)
        sc, ng = st.cell_score.cpu().numpy(), st.ngood.cpu().numpy()
        open_ = (ng > 0) & (sc < _hip.TETRA_ETSI_VOTE_CAP_DEFAULT)   # below the cap the score is the sum of the w
        w = sc[open_] / ng[open_]
        first = {"carriers_with_a_ballot": int((ng > 0).sum()), "ballots": int(ng.sum()), "at_cap": int((sc >= _hip.TETRA_ETSI_VOTE_CAP_DEFAULT).sum()),
                 "mean_w_per_ballot": {"min": round(float(w.min()), 1), "median": round(float(sorted(w)[len(w) // 2]), 1),
                                       "max": round(float(w.max()), 1)},
                 "agree_equals_ngood": bool((st.agree == st.ngood).all().item())}
        run(True, steps - 1)
    out = {"shape": shape, "rows": rows, "rows_per_group": G, "runs": runs, "steps_per_run": steps, "acquire": [], "vote": []}
    works = {"acquire": [], "vote": []}
    for _ in range(runs):
        for name, flag in (("acquire", False), ("vote", True)):
            prof, work = run(flag, steps)
            out[name].append({k: round(v, 4) for k, v in sorted(prof.items()) if k.startswith("etsi_")})
            works[name].append(work)
    out["work_bursts_blocks_crcgood_bschgood"] = works
    out["same_decoded_work"] = all(w == works["acquire"][0] for w in works["acquire"] + works["vote"])
    sc = st.cell_score.cpu().numpy()
    out["cells_held"] = int((st.cell_state == true).sum().item())
    out["score_after"] = {"min": int(sc.min()), "median": int(sorted(sc)[len(sc) // 2]), "max": int(sc.max()),
                          "at_cap": int((sc >= _hip.TETRA_ETSI_VOTE_CAP_DEFAULT).sum())}
    if first:
        out["first_step_from_unknown"] = first
    print(json.dumps(out))


if __name__ == "__main__":
    main()
