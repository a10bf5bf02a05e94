#!/usr/bin/env python3
"""The loss-of-lock monitor next to the stream demod it follows, on the streaming bench step
(tetra_profile's HIP events, one context, the two calls one after the other on one stream): per step the
device time of tetra_demod_etsi_stream's stage and of k_etsi_lock on that call's soft bits, nsym and
track, device pointers throughout; then what the monitor made of the synthesised channels.
usage: probe_lock.py [channels] [chunks] [runs]    (8192 channels of 131072-sample chunks at 2.4 MSps)
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
    from tetraear.signal.etsi import BenchStep, RESERVE
    C = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    chunks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    N = 131072
    dev = torch.device("cuda", 0)
    c = _hip.Context()
    c.check(c.lib.tetra_set_stream(c.handle, None), "set_stream")
    st = BenchStep(c, C, N, 2.4e6, 1, dev, cells="acquire", chunks=chunks)
    state = torch.zeros((C, _hip.ETSI_LOCK_STATE.itemsize // 4), dtype=torch.int32, device=dev)
    rec = torch.zeros((C, _hip.LOCK_FIELDS), dtype=torch.int32, device=dev)
    args = (_hip.ETSI_LOCK_NUM_DEFAULT, _hip.ETSI_LOCK_DEN_DEFAULT, _hip.ETSI_LOCK_WEAK_DEFAULT,
            _hip.ETSI_LOCK_NMIN_DEFAULT, _hip.ETSI_LOCK_PATIENCE_DEFAULT)

    def step():
        sym, soft, hard, nsym = st.bufs[st.kchunk & 1]
        st._demod(c, sym, soft, hard, nsym)
        c.check(c.lib.tetra_etsi_lock(c.handle, ctypes.c_void_p(soft.data_ptr() + 2 * RESERVE), _hip.ptr(nsym), C,
                                      st.stride, *args, _hip.ptr(st.track), _hip.ptr(state), _hip.ptr(rec)),
                "tetra_etsi_lock")
        st._lmac(c, soft, hard, nsym)

    for _ in range(chunks):   # warm-up: workspaces, one pass over the capture
        step()
    c.synchronize()
    out = []
    for r in range(runs):
        c.check(c.lib.tetra_profile(c.handle, 1), "profile")
        read_profile(c)
        for _ in range(chunks):
            step()
        prof = read_profile(c)
        c.check(c.lib.tetra_profile(c.handle, 0), "profile")
        out.append({k: round(ms / max(n, 1), 4) for k, (ms, n) in prof.items()})
    flags = rec[:, _hip.LOCK_FLAGS].cpu().numpy()
    r = rec.cpu().numpy()
    res = {"channels": C, "samples": N, "chunks": chunks, "stride_symbols": st.stride,
           "soft_bytes_read": int(2 * r[:, _hip.LOCK_N].sum()),
           "ms_per_call": out,
           "last_step": {"judged": int((flags & _hip.LOCK_JUDGED != 0).sum()), "bad": int((flags & _hip.LOCK_BAD != 0).sum()),
                         "railed": int((flags & _hip.LOCK_RAILED != 0).sum()),
                         "searching": int((flags & _hip.LOCK_SEARCHING != 0).sum()),
                         "relocks": int(r[:, _hip.LOCK_RELOCKS].sum()), "stream_resets": st.resets}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
