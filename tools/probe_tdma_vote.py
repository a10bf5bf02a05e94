#!/usr/bin/env python3
"""The timebase vote against tetra_etsi_mac_groups on the wideband bench step (tetra_profile's HIP events,
one context, the stages one after another): the etsi_mac_groups stage, timed in the same session and
alternating with etsi_quality + etsi_mac_vote_groups on one step object whose MAC call is switched
between runs; then the decoded work of either (bursts kept, CRC-good blocks among them, timebase_known /
timebase_wrong, the ballots).
usage: probe_tdma_vote.py [wideband samples] [runs] [steps] [snr_db]   (7200 rows, G = 9 at 10 M samples)
"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tetraear-bladerf_amd"), REPO]
os.environ["TETRA_WB_MAC"] = "vote"


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
    from tetraear.signal.wideband import BenchStep
    Nw = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    snr = float(sys.argv[4]) if len(sys.argv) > 4 else 30.0
    dev = torch.device("cuda", 0)
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    st = BenchStep(c, Nw, seed=1, device=dev, snr_db=snr)

    def run(vote, n):
        """n steps from new streams with the vote or without: stage ms per step."""
        st.tdma_vote = vote
        st.tdma.zero_()
        st.tdma_score.zero_()
        c.synchronize()
        c.check(c.lib.tetra_profile(c.handle, 1), "profile")
        read_profile(c)
        for _ in range(n):
            st()
        c.synchronize()
        prof = read_profile(c)
        c.check(c.lib.tetra_profile(c.handle, 0), "profile")
        return {k: ms / n for k, (ms, _) in prof.items()}

    run(False, 3)   # warm-up: workspaces
    run(True, 3)
    out = {"wideband_samples": Nw, "snr_db": snr, "rows": st.C, "rows_per_group": st.nchunk, "runs": runs,
           "steps_per_run": steps, "timebase": [], "vote": [], "quality": {}}
    for _ in range(runs):
        for name, flag in (("timebase", False), ("vote", True)):
            prof = run(flag, steps)
            out[name].append({k: round(v, 4) for k, v in sorted(prof.items()) if k.startswith("etsi_")})
            q = st.quality()
            q["scores"] = None
            if flag:
                sc = st.tdma_score.cpu().numpy()
                q["scores"] = {"min": int(sc.min()), "median": int(sorted(sc)[len(sc) // 2]), "max": int(sc.max()),
                               "at_cap": int((sc >= _hip.TETRA_TDMA_VOTE_CAP_DEFAULT).sum())}
            out["quality"].setdefault(name, q)
            assert {k: v for k, v in out["quality"][name].items() if k != "scores"} == \
                   {k: v for k, v in q.items() if k != "scores"}, "a run decoded other work than the one before"
    run(True, 1)   # what one step from new streams casts: cast, agreed, outvoted, won
    out["tvote_first_step"] = st.tvote.sum(dim=0).tolist()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
