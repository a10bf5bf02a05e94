#!/usr/bin/env python3
"""Benchmark: sustained IQ Msamples/s through the TETRA receive hot path on 1..N MI355X.

Workload (BASELINE.json configs[4], per rank): C channels x N samples of 2.4 MSps complex64 IQ
(the reference's drop-in unit: one GUI chunk, /root/reference/tetraear/ui/modern.py:1919), resident
in HBM before the timed region.  Channels are independent shards: rank r owns its own C channels
(weak scaling, no data-path collective; 65536 channels at 8 GPUs with the default C=8192).

A step = one pass of the hot path over the rank's batch:
  --chain etsi   (default) channel filter + pi/4-DQPSK demod with Gardner timing + sync/slicing +
                 descramble + deinterleave + RCPC Viterbi + CRC  (the north-star chain)
  --chain compat reference-compatible process() + decode() lower MAC
  --chain wideband  C3 (configs[2]): a 20 MSps capture of 800 carriers (--wb-samples per rank)
                 -> polyphase filter bank + 800-point FFT (fused, in LDS) -> per-carrier RRC resampler to 72 kHz ->
                 timing/decision -> lower MAC, every carrier cut into 3932-sample timing chunks

A plain run does only what its headline needs: set-up, warm-up, the timed steps, the result line.
  --full         adds what takes work of its own after the clock stopped: the CPU baselines (unless
                 --no-cpu), the measured read floor and the committed PMC traffic in "roofline", and the
                 last step's decoded-block statistics ("decoded_last_step")
  --dump-outputs DIR  writes what the last timed step computed (a fixed, seeded sample of its rows,
                 the written parts only) as DIR/<name>.npy; the inputs depend only on the arguments

Launch: python bench.py --gpus 1 --steps 5 --warmup 2
        python bench.py --gpus N ...   (starts torch.distributed.run --nproc-per-node N as a child)
        python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N
        (--gpus must equal the launcher's WORLD_SIZE, or bench exits non-zero before any GPU work)
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "tetraear-bladerf_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from tetraear import _hip  # noqa: E402
from tetraear.shard import aggregate_msps, max_over_ranks, rank_seed  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak (MI355X_MICROARCH.md, chip-level parameters)
FS = 2.4e6


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chain", choices=("etsi", "compat", "wideband"),
                    default=os.environ.get("TETRA_BENCH_CHAIN", "etsi"))
    ap.add_argument("--wb-samples", type=int, default=10_000_000,
                    help="wideband: 20 MSps samples per rank per step (C3: 0.5 s)")
    ap.add_argument("--channels", type=int, default=8192, help="channels per rank")
    ap.add_argument("--samples", type=int, default=131072, help="samples per channel chunk")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need, after the timed steps: the CPU baselines, the "
                         "read floor and the committed PMC traffic of the roofline, the decoded-block statistics")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64; a fixed, "
                         "seeded sample of the rows, at most 64 MB in all)")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="--full: CPU-baseline budget (rank 0)")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU baselines")
    ap.add_argument("--iq", choices=("cf32", "sc16"), default="cf32",
                    help="etsi: input sample format in HBM (sc16 = the BladeRF wire format, 4 B/sample)")
    ap.add_argument("--pipeline", choices=("auto", "on", "off"), default="auto",
                    help="etsi: overlap the demod of batch k+1 with the lower MAC of batch k on two streams "
                         "(auto: on for cf32 and sc16 -- sc16 since the lower MAC's traceback kernel: 1.210 -> "
                         "1.197 ms per step); compat: run consecutive batches' "
                         "whole chains on --compat-lanes streams (auto: on); wideband: channeliser of capture k+1 beside "
                         "the timing + lower MAC of capture k (auto: on)")
    ap.add_argument("--no-pipeline", action="store_true", help="same as --pipeline off")
    ap.add_argument("--compat-lanes", type=int, default=2,
                    help="compat pipeline: batches in flight (contexts / streams)")
    ap.add_argument("--host-input", action="store_true",
                    help="etsi: PCIe-inclusive mode -- each batch is copied from pinned host memory (double-buffered "
                         "copy stream); value is then the host-fed rate, never the HBM-resident headline")
    ap.add_argument("--cells", choices=("acquire", "given"), default="acquire",
                    help="etsi: the lower MAC acquires each channel's cell itself (default: BSCH with colour code 0 "
                         "first, the SYNC PDU's MCC / MNC / colour code kept per channel from step to step, over "
                         "--chunks consecutive chunks of each channel's capture, as a streaming receiver does), or "
                         "is given the synthesised cells up front")
    ap.add_argument("--chunks", type=int, default=None,
                    help="etsi: each channel is one continuous capture of CHUNKS x --samples samples resident in "
                         "HBM, decoded as one stream (CHUNKS > 1, fused demod: step k demodulates chunk k's window with "
                         "the timing loops carried and resumes the lower MAC's burst scan on the previous step's "
                         "unconsumed dibits; past the last chunk the capture restarts as a new one).  Default with "
                         "--cells acquire: warmup + steps (>= 8, capped by free HBM), so the timed steps never restart "
                         "it; 1 (each step the same chunk on its own) with --cells given")
    ap.add_argument("--demod", choices=("fused", "split"), default="fused",
                    help="etsi: fused channel filter + timing in one launch, or split (y through HBM, timing "
                         "launched separately -- beside the next batch's channel filter when pipelined)")
    return ap.parse_args()


def traffic_from_profiles(kernel, workload_key, profiles=None):
    """HBM bytes per launch of `kernel` from the newest committed rocprofv3 PMC summary of this
    workload (profiles/*_summary.json, written by tools/pmc_summary.py from separate FETCH_SIZE /
    WRITE_SIZE passes over the timed launches, with the gfx950 x2 FETCH correction, calibrated at
    4-, 8- and 16-B loads: profiles/r05_fetch_calibration.json).

    Only a summary of the CURRENT code counts: its entry must carry the kernel source's hash
    (tools/pmc_summary.py: kernel_source -- the .hip file defining the kernel plus common.h) and that
    hash must equal the file's hash now.  Otherwise {"bytes": None, "reason": ...} says why (no
    summary of this workload, or only summaries of other code), never a stale number."""
    import glob
    import re
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from pmc_summary import kernel_source
    now = kernel_source(kernel)

    def age(f):   # (round, version): r02_x beats r01_x_v10, v10 beats v9 (not a string sort)
        b = os.path.basename(f)
        r, v = re.match(r"r(\d+)_", b), re.search(r"_v(\d+)_", b)
        return (int(r.group(1)) if r else 0, int(v.group(1)) if v else 0, b)

    best, stale = None, []
    for f in sorted(glob.glob(os.path.join(profiles or os.path.join(REPO, "profiles"), "*_summary.json")), key=age):
        try:
            d = json.load(open(f))
        except ValueError:
            continue
        # round-5 summaries key kernels by full name with a "short" field; older ones by short name.
        # Of the entries for this kernel, the one with timed (in-window) launches and PMC bytes
        ks = [v for n, v in d.get("kernels", {}).items() if v.get("short", n) == kernel and "hbm_bytes_per_launch" in v]
        ks.sort(key=lambda v: v.get("timed_launches", 0))
        k = ks[-1] if ks else {}
        if workload_key in d.get("workload", "") and k and (d.get("selection") != "markers" or "timed_launches" in k):
            if now is None or k.get("source") != now:
                stale.append(os.path.basename(f))
                continue
            best = (k["hbm_bytes_per_launch"], os.path.basename(f), k.get("timed_avg_ns", k.get("avg_ns")))
    if best is None:
        if now is None:
            why = f"no source file defines {kernel}"
        elif stale:
            why = (f"{len(stale)} summaries of this workload (newest {stale[-1]}) profiled other code than the "
                   f"current {now['file']} (sha256 {now['sha256'][:12]}); re-profile with tools/profile_bench.sh")
        else:
            why = "no rocprofv3 PMC summary of this workload under profiles/"
        return {"bytes": None, "source": None, "reason": why}
    # the same summary's rocprof average duration of the kernel (timed launches when recorded), so the
    # line's live launch_ms can be checked against the committed profile
    return {"bytes": best[0], "source": best[1], "rocprof_avg_ms": round(best[2] / 1e6, 4) if best[2] else None}


def read_profile(c):
    if isinstance(c, (list, tuple)):
        out = {}
        for x in c:
            for k, (ms, n) in read_profile(x).items():
                m0, n0 = out.get(k, (0.0, 0))
                out[k] = (m0 + ms, n0 + n)
        return out
    names = ctypes.create_string_buffer(4096)
    ms = (ctypes.c_double * 64)()
    cnt = (ctypes.c_int64 * 64)()
    n = ctypes.c_int(0)
    c.check(c.lib.tetra_profile_read(c.handle, names, 4096, ms, cnt, 64, ctypes.byref(n)), "tetra_profile_read")
    raw = names.raw.split(b"\0")
    return {raw[i].decode(): (ms[i], cnt[i]) for i in range(n.value)}


class CompatStep:
    """process() + decode() lower MAC over the batch (tetra_demod_compat + tetra_lmac_compat).

    The chain's IIR passes are sequential per stream by construction (bit-exact scipy order): a
    batch of 8192 channels is one wave per SIMD, issue-latency bound.  pipeline(lanes) runs
    consecutive batches on `lanes` contexts / HIP streams, so batch k+1's kernels interleave with
    batch k's; every step still does the whole chain for one batch."""

    class _Lane:
        def __init__(self, c, C, smax, dev):
            self.c = c
            self.mc = torch.zeros(C, dtype=torch.float64, device=dev)
            self.mo = torch.zeros(C, dtype=torch.uint8, device=dev)
            self.soft = torch.empty((C, smax, 2), dtype=torch.float64, device=dev)
            self.hard = torch.empty((C, smax), dtype=torch.uint8, device=dev)
            self.hard64 = torch.empty((C, smax), dtype=torch.int64, device=dev)
            self.nsym = torch.empty(C, dtype=torch.int32, device=dev)
            self.nhard = torch.empty(C, dtype=torch.int32, device=dev)
            self.nsync = torch.empty(C, dtype=torch.int32, device=dev)
            self.rec = torch.empty((C, _hip.MAX_SYNC, _hip.F_FIELDS), dtype=torch.int32, device=dev)
            self.fb = torch.empty((C, _hip.MAX_SYNC, 510), dtype=torch.uint8, device=dev)
            self.bb = torch.empty((C, _hip.MAX_SYNC, 510), dtype=torch.uint8, device=dev)
            self.stream = None   # torch's current stream

    def __init__(self, c, iq, C, N):
        from tetraear.signal.processor import compat_plan
        from tetraear.core.decoder import cascade_table
        self.c, self.C, self.N = c, C, N
        self.plan, m, _ = compat_plan(FS, N, _hip.TETRA_CF32)
        self.smax = m // self.plan.sps + 1
        dev = iq.device
        self.iq = iq
        self.kmax = torch.from_numpy(cascade_table().copy()).to(dev)
        self.f32 = ctypes.c_int32(0)
        self.lanes = [self._Lane(c, C, self.smax, dev)]
        self.k = 0
        self.pipelined = False

    def pipeline(self, lanes=2):
        dev = self.iq.device
        for _ in range(lanes - 1):
            back = _hip.Context()
            s = torch.cuda.Stream(device=dev)
            back.check(back.lib.tetra_set_stream(back.handle, ctypes.c_void_p(s.cuda_stream)), "set_stream")
            lane = self._Lane(back, self.C, self.smax, dev)
            lane.stream = s
            s.wait_stream(torch.cuda.current_stream(dev))   # the lane's inputs are zeroed on the current stream
            self.lanes.append(lane)
        self.pipelined = True
        return self

    def contexts(self):
        return [ln.c for ln in self.lanes]

    def __getattr__(self, name):   # the first lane's outputs (tests read st.hard, st.nsync, ...)
        if name in ("soft", "hard", "nsym", "nsync", "rec", "fb", "bb"):
            return getattr(self.__dict__["lanes"][0], name)
        raise AttributeError(name)

    def __call__(self):
        ln = self.lanes[self.k % len(self.lanes)]
        self.k += 1
        c = ln.c
        with torch.cuda.stream(ln.stream or torch.cuda.current_stream(self.iq.device)):
            c.check(c.lib.tetra_demod_compat(c.handle, self.plan, _hip.ptr(self.iq), _hip.TETRA_CF32, self.C, self.N,
                                             _hip.ptr(ln.mc), _hip.ptr(ln.mo), _hip.ptr(ln.soft), _hip.ptr(ln.hard),
                                             _hip.ptr(ln.nsym), self.smax, self.f32), "demod")
            # hard symbols -> int64 stream rows for the lower MAC (torch ops on the lane's stream)
            ln.hard64.copy_(ln.hard)
            torch.sub(ln.nsym, 1, out=ln.nhard)
            ln.nhard.clamp_(min=0)
            c.check(c.lib.tetra_lmac_compat(c.handle, _hip.ptr(ln.hard64), _hip.ptr(ln.nhard), self.C, self.smax,
                                            _hip.ptr(self.kmax), _hip.ptr(ln.nsync), _hip.ptr(ln.rec),
                                            _hip.ptr(ln.fb), _hip.ptr(ln.bb)), "lmac")

    def algorithmic_bytes_per_sample(self):
        # 8 B cf32 in + per symbol (16 B complex128 soft + 1 B hard) + decoded bits (negligible)
        return 8.0 + 17.0 * 18000.0 / FS

    def dominant(self):
        # reads each input sample once (8 B); complex64 rows always take the banked forward pass
        return ("compat_sos_fwd", 8.0, "k_sos_fwd_bank")


def cpu_baseline(a, step):
    """BASELINE.md §3 on this box's host cores (tools/cpu_baseline.py -- the checker, timed; never
    in the timed region): the compat restatement of the reference's process() + decode(), single-core
    and all-core (worker processes); for the ETSI chain also its C oracle (thread pool) under
    "etsi_oracle"; for C3 the wideband restatement."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import cpu_baseline as CB
    if a.chain == "wideband":
        return CB.wideband_rate(step, a.cpu_seconds)
    out = CB.compat_rate(a.samples, 0.25 * a.cpu_seconds, 0.4 * a.cpu_seconds)
    if a.chain == "etsi":
        x = step.iq[:4].float().cpu().numpy()
        if step.fmt == _hip.TETRA_SC16:
            x = x / 32768   # the oracle filters cf32; SC16 -> cf32 is exact
        x = np.ascontiguousarray(x, np.float32).view(np.complex64)[..., 0]
        cells = step.cells[:4].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        out["etsi_oracle"] = CB.etsi_rate(x, cells, 0.35 * a.cpu_seconds)
    return out


def read_floor(c, step, reps=5):
    """GB/s of k_read_floor over the step's own input (rows x row_bytes at the dominant kernel's
    LDS footprint), timed with HIP events on the context stream."""
    ptr, rows, row_bytes, lds = step.floor_args()
    c.check(c.lib.tetra_profile(c.handle, 1), "profile")
    c.check(c.lib.tetra_read_floor(c.handle, ptr, rows, row_bytes, lds), "read_floor")   # warm-up launch
    read_profile(c)   # drop the warm-up record: only the reps below are averaged
    for _ in range(reps):
        c.check(c.lib.tetra_read_floor(c.handle, ptr, rows, row_bytes, lds), "read_floor")
    ms, n = read_profile(c).get("read_floor", (0.0, 0))
    c.check(c.lib.tetra_profile(c.handle, 0), "profile")
    return round(rows * row_bytes / (ms / n * 1e-3) / 1e9, 2) if n else None


def time_steps(step, steps, warmup, world, sync, on_timed=None):
    """The driver contract's timing: `warmup` untimed steps, then exactly `steps` steps bracketed by
    a barrier (N > 1) and a device synchronize on both sides; returns this rank's elapsed seconds
    (bench takes the max over ranks with max_over_ranks)."""
    for _ in range(warmup):
        step()
    sync()
    if on_timed is not None:
        on_timed()
    grouped = world > 1 or (dist.is_available() and dist.is_initialized())
    if grouped:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    if grouped:
        dist.barrier()
    return time.perf_counter() - t0


DUMP_BYTES = 56_000_000   # of the 64 MB a dump may take (its row indices included), shared by the row groups
DUMP_SEED = 20240531


def _upto(n, length, start=0):
    """[rows, length] bool: start <= j < start + n[row]."""
    j = torch.arange(length, device=n.device)[None, :]
    return (j >= start) & (j < start + n[:, None])


def _keep(t, mask):
    """t where mask (broadcast over t's trailing dims), 0 elsewhere: the buffers are torch.empty, so only
    the written parts of a row compare from run to run."""
    while mask.dim() < t.dim():
        mask = mask[..., None]
    return torch.where(mask, t, torch.zeros((), dtype=t.dtype, device=t.device))


def _demod_rows(r, sym, soft, hard, nsym, off=0):
    """Rows r of a demod's outputs: nsym symbols, nsym - 1 dibits and their soft bits, from column off."""
    ns = nsym[r].long()
    nh = (ns - 1).clamp(min=0)
    L = hard.shape[1] - off
    return {"nsym": ns, "sym": _keep(sym[r, off:], _upto(ns, L)), "soft": _keep(soft[r, 2 * off:], _upto(2 * nh, 2 * L)),
            "hard": _keep(hard[r, off:], _upto(nh, L))}


def _etsi_lmac_rows(step, r):
    """Rows r of the ETSI lower MAC's outputs: nburst bursts, nblock blocks, each block's type-1 bits."""
    nb, nk = step.nburst[r].long(), step.nblock[r].long()
    live = _upto(nk, _hip.ETSI_MAXJ)
    blocks = _keep(step.blocks[r], live)
    # type-1 bits per block kind (the rest of a type1 row is padding)
    bits = torch.tensor((268, 124, 60), device=nk.device)[blocks[..., 0].clamp(0, 2).long()] * live
    return {"nburst": nb, "bursts": _keep(step.bursts[r], _upto(nb, _hip.ETSI_MAXB)), "nblock": nk, "blocks": blocks,
            "type1": _keep(step.type1[r], torch.arange(268, device=nk.device)[None, None, :] < bits[..., None])}


def last_outputs(step):
    """What a caller of the timed path holds after its last step, as row groups [(file prefix, rows, fn)]: fn(r)
    gives {name: device tensor} of the rows r (an index tensor), unwritten parts zeroed."""
    if isinstance(step, CompatStep):
        ln = step.lanes[(step.k - 1) % len(step.lanes)]

        def compat(r):
            ns = ln.nsym[r].long()   # nsym soft symbols (complex128 pairs), nsym - 1 hard ones
            L = ln.hard.shape[1]
            out = {"nsym": ns, "soft": _keep(ln.soft[r], _upto(ns, L)),
                   "hard": _keep(ln.hard[r], _upto((ns - 1).clamp(min=0), L))}
            rec = _keep(ln.rec[r], _upto(ln.nsync[r].long(), _hip.MAX_SYNC))
            nbits = rec[..., _hip.F_NBITS] * (rec[..., _hip.F_VALID] != 0)   # 0 for a slot decode() skips
            j = torch.arange(510, device=rec.device)[None, None, :]
            out.update(nsync=ln.nsync[r], rec=rec, frame_bits=_keep(ln.fb[r], j < nbits[..., None]),
                       burst_bits=_keep(ln.bb[r], nbits >= 510))
            return out
        return [("", step.C, compat)]
    if hasattr(step, "wf"):   # wideband: the waterfall rows, and per (carrier, chunk) the timing + lower MAC
        return [("", step.C, lambda r: {**_demod_rows(r, step.sym, step.soft, step.hard, step.nsym),
                                        **_etsi_lmac_rows(step, r)}),
                ("waterfall_", step.nfr, lambda r: {"waterfall": step.wf[r]})]
    # etsi: the demod outputs of the last step's buffer (streaming rows start ETSI_RESERVE dibits in)
    if step.stream or (step.pipelined and step.demod_mode != "split"):
        sym, soft, hard, nsym = step.bufs[((step.k if step.pipelined else step.kchunk) - 1) & 1]
    else:
        sym, soft, hard, nsym = step.sym, step.soft, step.hard, step.nsym
    off = _hip.ETSI_RESERVE if step.stream else 0
    return [("", step.C, lambda r: {**_demod_rows(r, sym, soft, hard, nsym, off), **_etsi_lmac_rows(step, r)})]


def dump_outputs(step, path, dev):
    """Write last_outputs(step) as path/<name>.npy: float32, or float64 for 32- and 64-bit integers and
    doubles (exact).  Each row group keeps a fixed, seeded sample of its rows (all of them where they
    fit), listed in path/<group>rows.npy, so that the files of two runs with the same arguments hold
    the same rows."""
    def host(t):
        wide = t.dtype in (torch.int32, torch.int64, torch.float64)
        return t.to(torch.float64 if wide else torch.float32).cpu().numpy()

    os.makedirs(path, exist_ok=True)
    groups = last_outputs(step)
    for prefix, rows, fn in groups:
        one = {k: host(v) for k, v in fn(torch.zeros(1, dtype=torch.long, device=dev)).items()}
        per_row = sum(v.nbytes for v in one.values()) + 8
        n = max(1, min(rows, DUMP_BYTES // len(groups) // per_row))
        pick = np.arange(rows) if n == rows else np.sort(np.random.default_rng(DUMP_SEED).choice(rows, n, replace=False))
        np.save(os.path.join(path, prefix + "rows.npy"), pick.astype(np.float64))
        for k, v in fn(torch.from_numpy(pick).to(dev)).items():
            np.save(os.path.join(path, k + ".npy"), host(v))


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(a):
    """`--gpus N` means N GPUs, however bench.py is started.

    Under a launcher (WORLD_SIZE set) the world must equal --gpus, or bench exits non-zero before any
    GPU work.  Started bare with N > 1, bench starts `torch.distributed.run --nproc-per-node N` on
    itself as a CHILD process (never exec: nothing here has touched the GPU yet, and the ranks are
    new processes), lets rank 0's one JSON line through on the inherited stdout and returns the
    child's exit code.  Returns None when this process is itself the (only or a) rank to run."""
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is not None:
        if int(env_world) != a.gpus:
            print(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={env_world} ranks; "
                  f"launch with --nproc-per-node {a.gpus}", file=sys.stderr, flush=True)
            return 2
        return None
    if a.gpus <= 1:
        return None
    backend = os.environ.get("TETRA_BENCH_DIST", "nccl")
    have = torch.cuda.device_count()   # counts devices without initialising HIP in this process
    if backend == "nccl" and have < a.gpus:
        print(f"bench.py: --gpus {a.gpus} asks for one GPU per rank but {have} are visible "
              f"(TETRA_BENCH_DIST=gloo rehearses more ranks than GPUs)", file=sys.stderr, flush=True)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    import subprocess
    return subprocess.call(cmd, env=dict(os.environ, MASTER_ADDR="127.0.0.1"))


def main():
    a = parse()
    rc = launch_ranks(a)
    if rc is not None:
        sys.exit(rc)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # RCCL ("nccl") on a node with one GPU per rank.  TETRA_BENCH_DIST=gloo rehearses the N>1
    # path with several ranks sharing fewer GPUs (rank -> LOCAL_RANK mod device count; the timing
    # all_reduce then runs on a host tensor).
    backend = os.environ.get("TETRA_BENCH_DIST", "nccl")
    # TETRA_BENCH_FORCE_DIST=1: join the process group and run the timing all_reduce even at
    # WORLD_SIZE 1 (torchrun --nproc-per-node 1), so a one-GPU box executes the RCCL path itself
    force = os.environ.get("TETRA_BENCH_FORCE_DIST") == "1"
    gpu = local % max(1, torch.cuda.device_count()) if backend == "gloo" else local
    torch.cuda.set_device(gpu)
    dev = torch.device("cuda", gpu)
    if world > 1 or force:
        dist.init_process_group(backend, init_method="env://")
    os.environ["TETRA_HIP_DEVICE"] = str(gpu)
    c = _hip.ctx()
    stream = torch.cuda.current_stream(dev)
    c.check(c.lib.tetra_set_stream(c.handle, ctypes.c_void_p(stream.cuda_stream)), "set_stream")

    C, N = a.channels, a.samples
    if a.chain == "wideband":
        from tetraear.signal.wideband import BenchStep as WbStep
        step = WbStep(c, a.wb_samples, seed=rank_seed(1000, rank), device=dev)
        if (a.pipeline if not a.no_pipeline else "off") != "off":
            step.pipeline()
        C, N = 1, a.wb_samples   # units: wideband samples
    elif a.chain == "etsi":
        from tetraear.signal.etsi import BenchStep as EtsiStep
        if a.chunks is not None:
            chunks = a.chunks
        elif a.cells == "acquire" and a.demod == "fused" and not a.host_input:
            # one continuous capture per channel, long enough that the run never restarts it: the
            # streaming receiver decodes it as one symbol stream (capped by the free HBM)
            per = C * N * (4 if a.iq == "sc16" else 8)
            free = torch.cuda.mem_get_info(dev)[0]
            chunks = max(2, min(max(8, a.warmup + a.steps), int(0.8 * free) // per))
        else:
            chunks = 1
        step = EtsiStep(c, C, N, FS, seed=rank_seed(1000, rank), device=dev, iq_format=a.iq, demod=a.demod,
                        cells=a.cells, chunks=chunks)
        pipe = "off" if a.no_pipeline else a.pipeline
        if pipe != "off":
            step.pipeline()
        if a.host_input:
            step.host_feed()
    else:
        g = torch.Generator(device=dev)
        g.manual_seed(rank_seed(1000, rank))
        iq = (0.25 * torch.randn((C, N, 2), generator=g, device=dev, dtype=torch.float32))
        iq = torch.round(iq * 32768) / 32768   # SC16 grid, like capture.py:259-269
        step = CompatStep(c, iq, C, N)
        if (a.pipeline if not a.no_pipeline else "off") != "off":
            step.pipeline(a.compat_lanes)
    torch.cuda.synchronize(dev)
    ctxs = step.contexts() if hasattr(step, "contexts") else [c]

    def profile_on():
        for x in ctxs:
            x.check(x.lib.tetra_profile(x.handle, 1), "profile")
        read_profile(ctxs)   # drop warm-up records
        # marker launch: rocprofv3 traces of this command find the timed launches after it
        # (tools/pmc_summary.py); it completes in the synchronize before the clock starts
        c.check(c.lib.tetra_mark(c.handle, 1), "mark")

    elapsed = time_steps(step, a.steps, a.warmup, world, lambda: torch.cuda.synchronize(dev), profile_on)
    c.check(c.lib.tetra_mark(c.handle, 2), "mark")   # ... and before this one (after the clock stopped)
    prof = read_profile(ctxs)
    for x in ctxs:
        x.check(x.lib.tetra_profile(x.handle, 0), "profile")
    # slowest rank (RCCL all_reduce MAX); identity at N=1
    elapsed = max_over_ranks(elapsed, dev if backend == "nccl" else None, force=force)
    ms_step = elapsed / a.steps * 1e3
    value = aggregate_msps(C * N, world, a.steps, elapsed)
    if a.dump_outputs:   # rank 0's files in the directory itself, the other ranks' beside them
        dump_outputs(step, a.dump_outputs if rank == 0 else os.path.join(a.dump_outputs, f"rank{rank}"), dev)

    if rank == 0:
        if hasattr(step, "stage_bytes"):   # several comparable stages: the slowest one is dominant
            sb = step.stage_bytes()
            name = max(sb, key=lambda k: prof.get(k, (0.0, 0))[0])
            per_sample, ksym = sb[name]
        else:
            name, per_sample, ksym = step.dominant()
        kms, kcnt = prof.get(name, (0.0, 0))
        launch_ms = kms / max(1, kcnt)
        units_per_launch = C * N
        achieved = per_sample * units_per_launch / (launch_ms * 1e-3) / 1e9 if launch_ms > 0 else 0.0
        # --full only: launches, file reads and host work of their own, after the clock stopped
        floor = read_floor(c, step) if a.full and hasattr(step, "floor_args") else None
        cpu = None if a.no_cpu or not a.full else cpu_baseline(a, step)
        traffic = traffic_from_profiles(ksym, step.workload_key() if hasattr(step, "workload_key") else
                                        f"{C} channels x {N} {a.iq if a.chain == 'etsi' else 'cf32'}") if a.full else None
        out = {
            "metric": "IQ Msamples/s demod+Viterbi; real-time 25 kHz TETRA channels @1/2/4/8 GPU",
            "value": round(value, 3),
            "unit": "Msamples/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(ms_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": step.dtype if hasattr(step, "dtype") else "f32/f64",
            "data": "synthetic (device-generated, seeded per rank)",
            "config": step.config(world) if hasattr(step, "config") else {
                "workload": f"C5 shard: {C} channels x {N} {a.iq if a.chain == 'etsi' else 'cf32'} samples "
                            f"@2.4 MSps per GPU, chain={a.chain}",
                "channels_per_gpu": C, "samples_per_channel": N, "sample_rate": FS,
                "parallelism": f"channel-sharded x{world}",
                "pipeline": bool(getattr(step, "pipelined", False)),
                **({"input": "host-fed over PCIe (pinned, double-buffered copy stream)"}
                   if getattr(step, "hostfed", False) else {}),
                **({"demod": step.demod_mode} if hasattr(step, "demod_mode") else {}),
                **({"cells": step.cells_mode} if hasattr(step, "cells_mode") else {}),
                **({"chunks_per_channel": step.chunks} if getattr(step, "chunks", 1) > 1 else {}),
            },
            # the process group the timing reduction ran over (None: single process, no collective)
            "dist": ({"backend": dist.get_backend(), "world": dist.get_world_size(),
                      "reduce_tensor": "cuda" if backend == "nccl" else "cpu"} if dist.is_initialized() else None),
            "realtime_channels": int(step.realtime_channels(value) if hasattr(step, "realtime_channels")
                                     else value * 1e6 / FS),
            "roofline": {
                "bound": "hbm", "kernel": name, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                # HBM bytes per launch from this round's PMC summary of the same sources (or null), and
                # where that number came from (or why there is none)
                **({"traffic": traffic["bytes"], "traffic_source": traffic} if traffic else {}),
                "launch_ms": round(launch_ms, 4), "algorithmic_bytes_per_launch": per_sample * units_per_launch,
                "kernel_symbol": ksym,
                # the same HBM read pattern with no arithmetic (k_read_floor), measured in this run:
                # the practical ceiling the dominant kernel is held against besides the 8 TB/s spec
                **({"measured_read_floor_GBs": floor, "frac_of_floor": round(achieved / floor, 4)} if floor else {}),
            },
            "stages_ms_per_step": {k: round(v[0] / a.steps, 4) for k, v in prof.items()},
            # the last step's decoded blocks (read back after the timed region): the chain's work done
            **({"decoded_last_step": step.quality()} if a.full and hasattr(step, "quality") else {}),
            **({"cpu_baseline": cpu} if a.full else {}),
            "full": a.full,
        }
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
