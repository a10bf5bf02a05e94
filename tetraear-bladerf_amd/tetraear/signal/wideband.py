"""Wideband channeliser on the GPU (BASELINE.json configs[2]).

The reference receives one carrier per capture: the BladeRF is tuned to it and 2.4 MSps IQ goes
to SignalProcessor.process (/root/reference/tetraear/ui/modern.py:1886-1887, 2029).  The north
star's "polyphase FIR channeliser" instead takes a 20 MSps capture holding 800 carriers at 25 kHz
spacing and splits it on the device: a polyphase filter bank (libtetra_hip.so k_pfb_analysis2: fold
+ 800-point FFT fused, two blocks per iteration; D = M / 2 by default, so every carrier comes out at
50 kHz), then per carrier an RRC(0.35) matched-filter resampler to 72 kHz (k_pfb_resamp_fix), which
is exactly the sample stream the ETSI timing stage takes (4 samples per symbol, tetra_etsi_timing),
followed by the ETSI lower MAC.  The capture goes in as complex64 or as the radio's SC16 ([Nw, 2]
int16, scaled 1/32768 in the analysis kernel's loader).  This module designs the filters and moves arrays;
oracle/wideband.py is the float64 specification the tests hold it to.
"""
import collections
import ctypes
import dataclasses
import functools
import os

import numpy as np
from scipy import signal as _design

from tetraear import _hip
from tetraear.core.etsi import Carried, Geometry, LowerMac, carrier_key, cell_of, chain_options, run_chain
from tetraear.signal.etsi import etsi_plan, rrc

FS_WB = 20e6
M_WB = 800
M2_CHUNK = 3932     # 72 kHz samples per timing chunk (as a 128 Ki chunk at 2.4 MSps)
# samples consecutive timing chunks share: a whole burst (255 symbols = 1020 samples at 72 kHz) plus
# 15 symbols, so a burst that starts in one chunk ends in it too (TETRA_WB_OVERLAP=0: chunks tile the
# row, the round-1..6 form that loses the burst across every seam -- A/B only)
OV_CHUNK = int(os.environ.get("TETRA_WB_OVERLAP", "1080"))
BURST_SAMPLES = 1020   # one 255-symbol slot at 72 kHz
# Two filter-bank designs (the carrier's output rate fs / D and what it implies):
#   oversample 2 (default): D = M / 2 -> 50 kHz carriers.  A carrier's band aliases onto itself from
#     37.5 kHz, so the prototype is 5 branches long (cut-off 25 kHz, Kaiser 8: 0.003 dB ripple over
#     +-12.5 kHz, 74 dB down from 37.5 kHz); resampler 50 -> 72 kHz = 36 / 25 with 828 RRC taps (23 per
#     output).  Half the blocks of oversample 4: half the FFTs, half the filter-bank output Y.
#   oversample 4 (round 1-3): D = M / 4 -> 100 kHz carriers, 2 branches (cut-off 2 spacings, 72 dB
#     down from 87.5 kHz), resampler 18 / 25 with 810 taps (45 per output).
DESIGNS = {2: dict(P=5, cut=25e3, beta=8.0, up=36, down=25, Lg=828),
           4: dict(P=2, cut=None, beta=7.0, up=18, down=25, Lg=810)}
OVERSAMPLE = int(os.environ.get("TETRA_WB_OVERSAMPLE", "2"))   # 4: the round-3 design (A/B)
# the default design's constants (module attributes the tests and the bench read)
P_WB, UP, DOWN, LG = (DESIGNS[OVERSAMPLE][k] for k in ("P", "up", "down", "Lg"))


@functools.lru_cache(maxsize=8)
def wb_design(fs=FS_WB, M=M_WB, oversample=None):
    """Prototype lowpass h [M P] (unity DC gain, flat over +-12.5 kHz, and down >= 72 dB from the
    first band that aliases onto a carrier at fs / D) and the resampler RRC g [Lg] at up * fs / D."""
    ov = OVERSAMPLE if oversample is None else oversample
    d = DESIGNS[ov]
    D = M // ov
    if abs(fs / D * d["up"] / d["down"] - 72000.0) > 1e-6:
        raise ValueError(f"the channeliser is built for fs / (M / {ov}) = {72000.0 * d['down'] / d['up']:.0f} Hz carriers")
    cut = d["cut"] if d["cut"] is not None else 2.0 * fs / M
    h = _design.firwin(M * d["P"], cut, fs=fs, window=("kaiser", d["beta"])).astype(np.float32)
    sps = fs / D * d["up"] / 18000.0
    g = rrc((np.arange(d["Lg"]) - (d["Lg"] - 1) / 2.0) / sps).astype(np.float32)
    return h, g


class WbPlan:
    """tetra_wb_plan plus the tap arrays it points at."""

    def __init__(self, fs=FS_WB, M=M_WB, oversample=None):
        ov = OVERSAMPLE if oversample is None else oversample
        d = DESIGNS[ov]
        self.h, self.g = wb_design(fs, M, ov)
        p = _hip.WbPlan()
        p.M, p.D, p.P, p.up, p.down, p.Lg, p.fs = M, M // ov, d["P"], d["up"], d["down"], d["Lg"], fs
        p.h = self.h.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        p.g = self.g.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        self.c = p
        self.M, self.D, self.fs, self.oversample = M, M // ov, fs, ov

    def lengths(self, Nw):
        nb, n72 = ctypes.c_int64(), ctypes.c_int64()
        _hip.lib().tetra_wb_lengths(self.c, Nw, ctypes.byref(nb), ctypes.byref(n72))
        return nb.value, n72.value


@functools.lru_cache(maxsize=8)
def wb_plan(fs=FS_WB, M=M_WB, oversample=None):
    return WbPlan(fs, M, oversample)


Chunks = collections.namedtuple("Chunks", "nchunk stride length rowlen")


def chunking(plan, Nw, m2=M2_CHUNK, ov=None):
    """Each carrier's 72 kHz row (rowlen samples kept) is cut into nchunk timing chunks: chunk c is
    row[c m2, min(c m2 + length, rowlen)), length = m2 + ov, so consecutive chunks share ov samples
    and the last one runs to the row's end (tetra_etsi_timing_chunks).  ov = 0: nchunk = n72 // m2
    chunks tiling the first nchunk m2 samples (tetra_etsi_timing_om's layout)."""
    ov = OV_CHUNK if ov is None else ov
    _, n72 = plan.lengths(Nw)
    if ov == 0:
        nchunk = n72 // m2
        if nchunk < 1:
            raise ValueError(f"{Nw} wideband samples give {n72} samples per carrier, less than one chunk of {m2}")
        return Chunks(nchunk, m2, m2, nchunk * m2)
    if ov < 0 or ov % 4 or n72 < 16:
        raise ValueError(f"overlap {ov} (a multiple of 4 >= 0) over {n72} samples per carrier")
    nchunk = max(1, -(-(n72 - ov) // m2))
    return Chunks(nchunk, m2, min(m2 + ov, n72), n72)


def merge_chunks(nburst, bursts, nblock, blocks, M, nchunk, stride, tol=64):
    """The lower MAC's bursts per (carrier, chunk) -> each burst once.  A burst in the ov samples two
    chunks share is found by both; its position in the carrier row (chunk start + 2 x start bit, to
    within the timing phase) tells the copies apart from the next burst (>= BURST_SAMPLES later).
    Returns (keep [C, MAXB] bool: the first copy of every burst, in row order; keep_blocks [C, MAXJ]
    bool: the blocks of kept bursts).  nburst [C], bursts [C][MAXB][2], nblock [C], blocks
    [C][MAXJ][4] as tetra_lmac_etsi leaves them (host arrays)."""
    nburst, bursts = np.asarray(nburst), np.asarray(bursts)
    nblock, blocks = np.asarray(nblock), np.asarray(blocks)
    C, maxb = bursts.shape[:2]
    valid = np.arange(maxb)[None, :] < nburst[:, None]
    ch = np.broadcast_to(np.arange(C)[:, None], (C, maxb))
    pos = (ch % nchunk) * stride + 2 * bursts[..., 0].astype(np.int64)
    car = ch // nchunk
    ci, ji = np.nonzero(valid)
    order = np.lexsort((ci, pos[ci, ji], car[ci, ji]))   # by carrier, row position, then chunk
    ci, ji = ci[order], ji[order]
    pc, cc = pos[ci, ji], car[ci, ji]
    first = np.ones(len(ci), bool)
    first[1:] = (cc[1:] != cc[:-1]) | (pc[1:] - pc[:-1] > tol)
    keep = np.zeros((C, maxb), bool)
    keep[ci[first], ji[first]] = True
    maxj = blocks.shape[1]
    jv = np.arange(maxj)[None, :] < nblock[:, None]
    bi = np.clip(blocks[..., 2], 0, maxb - 1)
    keep_blocks = jv & keep[np.arange(C)[:, None], bi]
    return keep, keep_blocks


def grouped_om(plan, m2=M2_CHUNK):
    """The wideband timing takes its Oerder-Meyr class sums from the resampler's group partials
    (tetra_channelize_om + tetra_etsi_timing_om) where the plan's output groups hold whole classes
    (up a multiple of 4: the D = M / 2 design) and TETRA_WB_OM is not 0."""
    return (plan.c.up % 4 == 0 and plan.c.up <= 64 and m2 % 4 == 0 and m2 >= 16
            and os.environ.get("TETRA_WB_OM", "1") != "0")


def sc16_to_cf32(x):
    """[Nw, 2] int16 -> [Nw] complex64 scaled 1/32768 (exact): the capture the SC16 kernels compute on."""
    return ((x[..., 0].astype(np.float32) + 1j * x[..., 1].astype(np.float32)) / np.float32(32768)).astype(
        np.complex64)


def _capture(x):
    """A capture as the library takes it: int16 input is SC16, [Nw, 2] (I, Q) as the radio delivers
    it, and goes in as it is; anything else becomes [Nw] complex64.  Returns (array, iq_fmt)."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        if x.ndim != 2 or x.shape[-1] != 2:
            raise ValueError("SC16 input must be [Nw, 2] int16")
        return np.ascontiguousarray(x), _hip.TETRA_SC16
    return np.ascontiguousarray(x, np.complex64), _hip.TETRA_CF32


def row_keys(plan, center_hz):
    """follow=True: the carrier key (core/etsi.py carrier_key, Hz / 6250) of every row of the plan.  Row k is FFT
    bin k of a capture centred on center_hz: carrier_key(center_hz) + 4 (k if k < M / 2 else k - M).  ValueError
    without center_hz, and unless the rows lie 25 kHz apart exactly (fs / M), as the carrier numbering does."""
    if center_hz is None:
        raise ValueError("follow=True maps carrier numbers to rows: it needs center_hz")
    if plan.fs != 25000.0 * plan.M:
        raise ValueError(f"follow=True needs rows 25 kHz apart: fs / M is {plan.fs / plan.M} Hz")
    k = np.arange(plan.M)
    return (carrier_key(center_hz) + 4 * np.where(k < plan.M // 2, k, k - plan.M)).astype(np.int32)


@dataclasses.dataclass
class CarrierState(Carried):
    """What the wideband chain carries per carrier from buffer to buffer beside the Carried timebases, scores
    and fragment chains ([M] each, updated in place; a fresh one is a new stream per carrier): the acquisition's
    cell_state (scrambling inits; None: the cells are given), acquired (bool: the carrier had a cell before
    the call) and cell_score (int32; None: no vote), and ``advance``, the bits a carrier's stream moves on by
    after the call."""
    cell_state: np.ndarray = None
    acquired: np.ndarray = None
    cell_score: np.ndarray = None
    advance: int = 0
    keys: np.ndarray = None   # follow: the carriers' keys (row_keys)


class WidebandReceiver:
    """Channeliser + per-carrier ETSI demod (timing, decision) for host or device arrays.  Every
    method that takes a capture x takes it as [Nw] complex or as [Nw, 2] int16 (SC16, scaled 1/32768 on
    the device): the results are those of the complex64 capture x / 32768, bit for bit."""

    def __init__(self, fs=FS_WB, M=M_WB, m2=M2_CHUNK, oversample=None):
        self.plan = wb_plan(fs, M, oversample)
        self.etsi = etsi_plan(2.4e6)   # timing-loop constants (the channel-filter taps are not used)
        self.m2 = m2
        self.tvote = None   # [M, 4] int32: the ballots of the last decode with timebase="vote"
        self.frag_stats = None   # dict(dropped [M], orphans [M]) of the last decode with sdu=True
        self.assign_stats = None   # dict(expired [M], released [M]) of the last decode with follow=True

    def channelize(self, x, n_keep=None):
        """x [Nw] complex64 or [Nw, 2] int16 -> y [M][n_keep] complex64 at 72 kHz."""
        x, fmt = _capture(x)
        c = _hip.ctx()
        _, n72 = self.plan.lengths(len(x))
        n_keep = n72 if n_keep is None else n_keep
        y = np.empty((self.plan.M, n_keep), np.complex64)
        if n_keep == 0:   # a capture shorter than one 72 kHz output (the oracle's [M, 0])
            return y
        c.check(c.lib.tetra_channelize_fmt(c.handle, self.plan.c, _hip.ptr(x), fmt, len(x), _hip.ptr(y), n_keep),
                "channelize")
        return y

    def channelize_om(self, x, n_keep=None):
        """channelize plus the resampler's Oerder-Meyr group partials: (y [M][n_keep] complex64,
        om [M][ceil(n_keep / up)][4] float32) -- D = M / 2 plan only (tetra_channelize_om)."""
        x, fmt = _capture(x)
        c = _hip.ctx()
        _, n72 = self.plan.lengths(len(x))
        n_keep = n72 if n_keep is None else n_keep
        y = np.empty((self.plan.M, n_keep), np.complex64)
        om = np.empty((self.plan.M, -(-n_keep // self.plan.c.up), 4), np.float32)
        if n_keep == 0:
            return y, om
        c.check(c.lib.tetra_channelize_om_fmt(c.handle, self.plan.c, _hip.ptr(x), fmt, len(x), _hip.ptr(y), n_keep,
                                              _hip.ptr(om)), "channelize_om")
        return y, om

    def grouped_om(self):
        """Whether demod forms the timing's Oerder-Meyr sums in the resampler (the D = M / 2 plan;
        TETRA_WB_OM=0 keeps the timing's own pass over y, for A/B)."""
        return grouped_om(self.plan, self.m2)

    def demod(self, x):
        """x [Nw] -> (hard, soft_bits, sym, nsym) per (carrier, chunk) of chunking(): [M, nchunk,
        smax] uint8, [M, nchunk, 2 smax] int8, [M, nchunk, smax] complex64, [M, nchunk] int32."""
        x, _ = _capture(x)
        ck = chunking(self.plan, len(x), self.m2)
        om = None
        if self.grouped_om():
            y, om = self.channelize_om(x, ck.rowlen)
        else:
            y = self.channelize(x, ck.rowlen)
        c = _hip.ctx()
        M = self.plan.M
        C = M * ck.nchunk
        sm = ck.length // 4 + 2
        sym = np.empty((C, sm), np.complex64)
        soft = np.empty((C, 2 * sm), np.int8)
        hard = np.empty((C, sm), np.uint8)
        ns = np.empty(C, np.int32)
        c.check(c.lib.tetra_etsi_timing_chunks(c.handle, self.etsi, _hip.ptr(y), M, ck.rowlen, ck.nchunk, ck.stride,
                                               ck.length, _hip.ptr(om) if om is not None else None,
                                               om.shape[1] if om is not None else 0, self.plan.c.up, _hip.ptr(sym),
                                               _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(ns), sm, None),
                "etsi_timing_chunks")
        return (hard.reshape(M, ck.nchunk, sm), soft.reshape(M, ck.nchunk, 2 * sm), sym.reshape(M, ck.nchunk, sm),
                ns.reshape(M, ck.nchunk))


    def decode(self, x, cells, mac=False, timebase=False, tol=64, link_quality=False,
               tdma_cap=_hip.TETRA_TDMA_VOTE_CAP_DEFAULT, traffic=False, sdu=False, llc=False, follow=False,
               center_hz=None):
        """x [Nw] -> per carrier the frames decoded from it, each burst once (merge_chunks), in row
        order: demod, then the ETSI lower MAC on every (carrier, chunk) with carrier k's scrambling
        init cells[k].  A frame is the lower MAC's dict (core/etsi.py) plus "chunk" and "sample" (its
        start in the carrier's 72 kHz row, to within the timing phase).  mac=True: every block gains
        ``npdu`` / ``pdus`` (tetra_etsi_mac's PDU walk, per block; the frames get no tn / fn / mn --
        that takes timebase=True).  timebase=True (implies the PDU walk): tetra_etsi_mac_groups merges
        each carrier's chunk rows on the device (its keep replaces merge_chunks') and runs one TDMA
        timebase per carrier over them, a new stream per call: every frame gains ``tn`` / ``fn`` /
        ``mn`` / ``slot_flags`` as EtsiLowerMac's frames carry them (None before the carrier's first
        CRC-good SYNC).  tol: the duplicate distance in 72 kHz samples (merge_chunks'); timebase=True
        needs it and m2 even (the device works in bits), else ValueError.  link_quality=True: the
        frames and blocks gain EtsiLowerMac(link_quality=True)'s keys, from one tetra_etsi_link_quality
        call over all (carrier, chunk) rows with G = chunks per carrier (core/etsi.py carrier_quality
        totals them per carrier).  timebase="vote": as timebase=True by tetra_etsi_mac_vote_groups -- a
        SYNC moves a carrier's slot grid only if its soft-bit weight outvotes the score the grid has
        gathered (bounded by tdma_cap), a burst that two chunks share casts one ballot, and of its copies
        the one that decoded best is kept (most CRC-good blocks, then fewest known-bit errors, then the
        strongest soft bits) instead of the earlier row's.  tetra_etsi_link_quality runs first, on the
        intact rows, for the weights; its keys appear on the frames only with link_quality=True.
        ``slot_flags`` bit 2: the burst's own SYNC was outvoted.  ``tvote`` [M, 4] holds the last call's
        ballots per carrier (cast, agreed, outvoted, won).  traffic=True: every frame gains ``usage`` and
        ``traffic`` as EtsiLowerMac(traffic=True)'s frames carry them, from one tetra_etsi_traffic call over
        all (carrier, chunk) rows with G = chunks per carrier; with timebase=True or "vote" that call's
        slots and keep are passed in (frame 18 reads "control", and a burst two chunks share is exported
        from the copy kept).  sdu=True (needs mac=True and timebase=True or "vote", else ValueError): one
        tetra_etsi_sdu call over all rows with G = chunks per carrier and the MAC call's keep, a new stream
        per call: every pdu dict gains ``sdu`` / ``sdu_bits`` / ``sdu_status`` / ``role`` and its optional
        elements, and the frame whose MAC-END completed a chain of fragments gains ``sdus``, as
        EtsiLowerMac(sdu=True)'s frames carry them (core/etsi.py messages() lists a carrier's finished
        TM-SDUs); ``frag_stats`` holds the call's dropped / orphans per carrier and ``lost``, the messages
        completed beyond the SDU_MAXD (core/etsi.py) a call returns per carrier, which reach no frame.
        llc=True (needs sdu=True, else ValueError): one tetra_etsi_llc call over the same groups; every pdu
        dict and every entry of ``sdus`` gains ``llc`` (core/etsi.py llc_keys; link_messages() lists the
        messages whose LLC PDU reads well).
        follow=True (needs sdu=True and center_hz, the capture's centre frequency in Hz, else ValueError): one
        tetra_etsi_assign call over the same groups joins the carriers of the capture -- row k is the carrier at
        center_hz + 25 kHz x (k if k < M / 2 else k - M), the rows count one sample clock, so a channel
        allocation heard on one carrier marks the timeslot it names on the row of the carrier it names.  Every
        frame gains ``assigned`` / ``assignment`` / ``allocations`` as EtsiLowerMac(follow=True)'s frames carry
        them (``from_hz``: the carrier that announced it; ``target_row``: the row an allocation names);
        ``assign_stats`` holds expired / released per carrier.  An announcement, not the AACH: see EtsiLowerMac."""
        opt = chain_options(mac, timebase, link_quality, traffic, sdu, llc, tdma_cap, grouped=True, follow=follow)
        keys = row_keys(self.plan, center_hz) if opt.follow else None
        return self._decode(x, np.asarray(cells, np.uint32), opt, tol, CarrierState(keys=keys))[0]

    def decode_acquire(self, x, cell_init, mac=False, timebase=False, tol=64, link_quality=False, score=None,
                       vote_cap=_hip.TETRA_ETSI_VOTE_CAP_DEFAULT, tdma_cap=_hip.TETRA_TDMA_VOTE_CAP_DEFAULT,
                       traffic=False, acquired=None, sdu=False, llc=False, follow=False, center_hz=None):
        """decode without given cells: cell_init [M] holds each carrier's scrambling init before the
        capture (3 = unknown); every carrier's cell comes from the last CRC-good BSCH over all of its
        chunk rows, and all of its rows are descrambled with it (tetra_lmac_etsi_acquire_groups, G =
        chunks per carrier).  Returns (frames as decode's, the inits after the capture [M] uint32,
        ngood [M] int32: the CRC-good BSCH blocks seen per carrier, copies in two chunks counted twice).
        link_quality=True scores every carrier's blocks with the cell acquired for it.
        score [M] int32 (C-contiguous, updated in place): the cell is chosen by the vote instead
        (tetra_lmac_etsi_vote_groups: every CRC-good BSCH weighed by its soft bits, cell_init[k] defending
        with score[k], scores bounded by vote_cap); at most 32 chunks per carrier.  The return is the same.
        timebase="vote": decode's, the blocks scored with the cell acquired for the carrier.
        traffic=True: decode's, every carrier's slots descrambled with the cell acquired for it; a carrier
        without a cell -- no CRC-good BSCH in this capture, and none before it: acquired [M] bool, or by
        default cell_init[k] == 3 -- reports ``usage`` None (its blocks were descrambled with no cell, so
        a failed CRC says nothing).  The default misreads a carrier whose known cell is all zero (MCC =
        MNC = colour code = 0), which has the init of "unknown": pass ``acquired`` for such a carrier, as
        WidebandStream does from piece to piece.  sdu=True, llc=True, follow=True with center_hz: decode's."""
        state = np.array(cell_init, np.uint32)
        if state.shape != (self.plan.M,):
            raise ValueError(f"cell_init holds {state.shape} inits, the receiver has {self.plan.M} carriers")
        if score is not None and not (isinstance(score, np.ndarray) and score.dtype == np.int32 and
                                      score.shape == (self.plan.M,) and score.flags["C_CONTIGUOUS"]):
            raise ValueError(f"score must be a C-contiguous int32 array of {self.plan.M} (it is updated in place)")
        had = state != 3 if acquired is None else np.asarray(acquired, bool)
        opt = chain_options(mac, timebase, link_quality, traffic, sdu, llc, tdma_cap,
                            None if score is None else vote_cap, grouped=True, follow=follow)
        keys = row_keys(self.plan, center_hz) if opt.follow else None
        frames, ngood = self._decode(x, None, opt, tol, CarrierState(cell_state=state, acquired=had, cell_score=score,
                                                                    keys=keys))
        return frames, state, ngood

    def _decode(self, x, cells, opt, tol, st):
        """The chain behind decode (cells [M]; st.cell_state None) and decode_acquire (st.cell_state [M], updated
        in place, and st.cell_score [M] int32 or None, likewise: the vote): (frames, ngood or None).  opt: the
        ChainOptions; st: the CarrierState, updated in place -- a fresh one a new stream per carrier (st.keys [M]:
        the carriers' keys, row_keys, with opt.follow)."""
        if opt.timebase in ("groups", "vote") and (self.m2 % 2 or tol % 2 or tol < 0):
            raise ValueError(f"timebase=True works in bits: m2 ({self.m2}) and tol ({tol}) must be even")
        hard, soft, _, ns = self.demod(x)
        M, nchunk, sm = hard.shape
        C = M * nchunk
        soft, hard, ns = soft.reshape(C, -1), hard.reshape(C, -1), np.ascontiguousarray(ns.reshape(-1))
        lm = LowerMac.zeros(C)
        c = _hip.ctx()
        rows = (c.handle, _hip.ptr(soft), _hip.ptr(hard), _hip.ptr(ns), C, sm)
        ngood, has = None, np.ones(M, bool)
        if st.cell_state is None:
            cc = np.ascontiguousarray(np.repeat(cells, nchunk))
            c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(cc), C), "tetra_etsi_set_cells")
            c.check(c.lib.tetra_lmac_etsi(*rows, *lm.ptrs()), "tetra_lmac_etsi")
        else:
            cells, ngood = st.cell_state, np.zeros(M, np.int32)
            if st.cell_score is not None:
                agree = np.zeros(M, np.int32)
                c.check(c.lib.tetra_lmac_etsi_vote_groups(*rows, nchunk, opt.vote_cap, _hip.ptr(cells),
                                                          _hip.ptr(st.cell_score), _hip.ptr(ngood), _hip.ptr(agree),
                                                          *lm.ptrs()), "tetra_lmac_etsi_vote_groups")
            else:
                c.check(c.lib.tetra_lmac_etsi_acquire_groups(*rows, nchunk, _hip.ptr(cells), _hip.ptr(ngood), *lm.ptrs()),
                        "tetra_lmac_etsi_acquire_groups")
            has = (ngood > 0) | st.acquired
        frames, mac, sd, votes = run_chain(c, opt, Geometry(nchunk, self.m2 // 2, tol // 2, st.advance), soft, hard, ns,
                                           0, cells, np.repeat(has, nchunk), lm, st, st.keys, True)
        if opt.follow:
            self.assign_stats = {"expired": st.assign["expired"].copy(), "released": st.assign["released"].copy()}
        if votes is not None:
            self.tvote = votes
        if sd is not None:
            self.frag_stats = {"dropped": st.frag["dropped"].copy(), "orphans": st.frag["orphans"].copy(),
                               "lost": np.maximum(sd.ndone.astype(np.int64) - sd.done.shape[1], 0)}
        if mac is not None and mac.keep is not None:   # merged on the device
            keep = mac.keep.astype(bool)
        else:
            keep, _ = merge_chunks(lm.nb, lm.bursts, lm.nk, lm.blocks, M, nchunk, self.m2, tol)
        out = [[] for _ in range(M)]
        for ch in range(C):
            for b, f in enumerate(frames[ch]):
                if keep[ch, b]:
                    f["chunk"] = ch % nchunk
                    f["sample"] = (ch % nchunk) * self.m2 + 2 * f["position"]
                    out[ch // nchunk].append(f)
        for fr in out:
            fr.sort(key=lambda f: f["sample"])
        return out, ngood


class WidebandStream:
    """Consecutive pieces of one continuous wideband capture decoded as one stream (the C3 form of the
    ETSI receiver's streaming, signal/etsi.py EtsiStream): each call channelises the new samples
    behind a tail of the previous ones and WidebandReceiver.decode's frames are kept once per carrier
    by their position in the carrier's whole 72 kHz stream, so a burst across the seam between two
    pieces is decoded too.  The tail starts a whole number of resampler periods (D x down input
    samples -> up outputs) into the buffer, so its outputs are the previous buffer's at the same
    stream positions, bit for bit, and it holds the last CARRY_Y outputs' input: every burst that the
    buffer's end cut is whole in the next one.  The period also holds the filter bank's mixer term
    ((-1)^(k j) at D = M / 2, (-i)^(k j) at M / 4: whole cycles of it), else odd carriers would
    come out negated.

    ``cells`` [M] scrambling inits: every carrier is descrambled with its own.  ``cells=None``: the
    stream acquires them (WidebandReceiver.decode_acquire): a carrier's cell is the last CRC-good
    BSCH of the buffers so far, kept from piece to piece in ``cell_state`` / ``acquired`` (reset()
    clears them) and read as ``cells``: per carrier (MCC, MNC, colour code), None before the first
    BSCH -- EtsiLowerMac.cells per carrier.  A burst is reported once, as first decoded: one that a
    buffer decoded before its carrier's cell was known is not reported again from the next buffer.
    ``mac=True``: the blocks carry ``npdu`` / ``pdus`` (WidebandReceiver.decode).  ``timebase=True``
    (implies it): the frames carry ``tn`` / ``fn`` / ``mn`` / ``slot_flags`` from one TDMA timebase per
    carrier, carried from piece to piece in ``tdma`` [M] (reset() clears it): a buffer's carried tail
    is decoded again behind the anchor, which places those bursts without moving it.
    ``timebase="vote"``: the timebases by tetra_etsi_mac_vote_groups (WidebandReceiver.decode): the score
    each carrier's slot grid has gathered is carried beside ``tdma`` in ``tdma_score`` [M] and read as
    ``tdma_scores`` (reset() clears it); ``tdma_cap`` bounds it.  Within a buffer the best copy of a burst
    is kept; the choice between a burst's copies in two successive buffers stays "first decoded" (``last``).
    ``link_quality=True``: the frames and blocks carry the link-quality keys (WidebandReceiver.decode).
    ``traffic=True``: the frames carry ``usage`` / ``traffic`` (WidebandReceiver.decode); in acquisition a
    carrier reports ``usage`` None until a buffer holds its first CRC-good BSCH.
    ``sdu=True`` (with ``mac=True`` and a timebase): the pdu dicts carry their TM-SDU and a frame whose
    MAC-END completed a chain carries ``sdus`` (WidebandReceiver.decode); one fragment state per carrier
    is carried from piece to piece in ``frag`` [M] with the advance of ``tdma`` (reset() clears it), and
    the carried tail's bursts, decoded again, feed nothing a second time.  ``frag_stats``: the chains
    dropped and the orphans per carrier since reset().
    ``llc=True`` (with ``sdu=True``): the pdu dicts and the ``sdus`` entries carry ``llc`` (WidebandReceiver.decode).
    ``follow=True`` (with ``sdu=True`` and ``center_hz``): the frames carry ``assigned`` / ``assignment`` /
    ``allocations`` (WidebandReceiver.decode); one assignment state per carrier is carried from piece to piece in
    ``assign`` [M] with the advance of ``tdma`` (reset() clears it), so a call announced in one piece marks the
    traffic of the next; ``assign_stats``: the entries expired and released per carrier since reset().
    ``vote=True`` (acquisition only): a carrier's cell is chosen by the vote over each buffer's BSCH
    blocks (WidebandReceiver.decode_acquire(score=...)), the score it gathers carried from piece to piece
    in ``cell_score`` and read as ``cell_scores`` (reset() clears it).  A burst in the carried tail is
    decoded again in the next buffer and votes again there, as it does in two overlapping chunks.

    The pieces may be [n, 2] int16 (SC16, a recording or the radio's buffer as it is): the tail is
    then kept in int16 and the buffer goes to the device in 4 B per sample.  If the pieces change
    format, whichever of tail and piece is int16 is converted (x / 32768, exact) and the buffer is
    complex64, so a mixed stream gives what the complex64 stream does."""
    CARRY_Y = 2 * BURST_SAMPLES

    def __init__(self, cells=None, fs=FS_WB, M=M_WB, m2=M2_CHUNK, oversample=None, tol=64, mac=False, timebase=False,
                 link_quality=False, vote=False, vote_cap=_hip.TETRA_ETSI_VOTE_CAP_DEFAULT,
                 tdma_cap=_hip.TETRA_TDMA_VOTE_CAP_DEFAULT, traffic=False, sdu=False, llc=False, follow=False,
                 center_hz=None):
        self.opt = chain_options(mac, timebase, link_quality, traffic, sdu, llc, tdma_cap, vote_cap if vote else None,
                                 grouped=True, follow=follow)
        self.follow = self.opt.follow
        self.traffic, self.sdu, self.llc = self.opt.traffic, self.opt.sdu, self.opt.llc
        self.link_quality = self.opt.link_quality
        self.rx = WidebandReceiver(fs, M, m2, oversample)
        self.acquire, self.mac, self.timebase = cells is None, bool(mac), bool(timebase)
        self.tdma_vote, self.tdma_cap = timebase == "vote", int(tdma_cap)
        self.vote, self.vote_cap = bool(vote), int(vote_cap)
        if self.vote and not self.acquire:
            raise ValueError("vote=True chooses among acquired cells: it takes no given cells")
        if self.timebase and m2 % 2:
            raise ValueError(f"timebase=True works in bits: m2 ({m2}) must be even")
        self._cells = None if self.acquire else np.ascontiguousarray(cells, np.uint32)
        p = self.rx.plan
        blocks = int(np.lcm(p.c.down, p.oversample))   # filter-bank blocks per period
        self.per, self.ups, self.M, self.tol = p.D * blocks, p.c.up * blocks // p.c.down, p.M, tol
        self.keys = row_keys(p, center_hz) if self.follow else None
        self.reset()

    @property
    def cells(self):
        """Given cells: their scrambling inits [M].  Acquisition: per carrier the (MCC, MNC, colour
        code) acquired so far, None where no BSCH decoded yet."""
        if not self.acquire:
            return self._cells
        return [cell_of(v) if a else None for v, a in zip(self.cell_state, self.acquired)]

    @property
    def cell_scores(self):
        """vote=True: the score each carrier's cell has gathered ([M] int32, a copy); else None."""
        return None if self.cell_score is None else self.cell_score.copy()

    @property
    def tdma_scores(self):
        """timebase="vote": the score each carrier's timebase has gathered ([M] int32, a copy); else None."""
        return None if self.tdma_score is None else self.tdma_score.copy()

    def reset(self):
        self.tail = np.zeros(0, np.complex64)
        self.y0 = 0                                    # stream position of the buffer's first output
        self.last = np.full(self.M, -(1 << 62), np.int64)   # stream position of each carrier's last frame
        # acquisition: each carrier's scrambling init (3 = unknown) and whether a CRC-good BSCH was
        # decoded on it (an all-zero cell has the init of "unknown")
        self.cell_state = np.full(self.M, 3, np.uint32) if self.acquire else None
        self.acquired = np.zeros(self.M, bool) if self.acquire else None
        self.cell_score = np.zeros(self.M, np.int32) if self.vote else None   # the vote's score per carrier
        # timebase: each carrier's tetra_etsi_tdma; bit0 = the stream bit of the buffer's first output
        self.tdma = np.zeros(self.M, _hip.ETSI_TDMA) if self.timebase else None
        self.tdma_score = np.zeros(self.M, np.int32) if self.tdma_vote else None   # timebase="vote"
        self.frag = np.zeros(self.M, _hip.ETSI_FRAG) if self.sdu else None   # sdu=True: the fragment chains
        self.lost_sdus = np.zeros(self.M, np.int64)
        self.assign = np.zeros(self.M, _hip.ETSI_ASSIGN) if self.follow else None   # follow=True: the assigned timeslots

    @property
    def assign_stats(self):
        """follow=True: dict(expired [M], released [M]) since reset(); else None."""
        return None if self.assign is None else {"expired": self.assign["expired"].copy(),
                                                 "released": self.assign["released"].copy()}

    @property
    def frag_stats(self):
        """sdu=True: dict(dropped [M], orphans [M], lost [M]: completions beyond a buffer's SDU_MAXD per
        carrier, which reach no frame) since reset(); else None."""
        return None if self.frag is None else {"dropped": self.frag["dropped"].copy(),
                                               "orphans": self.frag["orphans"].copy(), "lost": self.lost_sdus.copy()}

    def _decode_buffer(self, buf, advance=0):
        if self.timebase:
            # the stream's attributes as they are now (one assigned from outside counts); cell_state a new array a
            # buffer, so that one read before the call stays as it was
            st = CarrierState(self.tdma, self.tdma_score, self.frag, self.last - self.y0 + self.tol if self.sdu else None,
                              self.assign, np.array(self.cell_state, np.uint32) if self.acquire else None, self.acquired,
                              self.cell_score, advance, self.keys)
            frames, ngood = self.rx._decode(buf, self._cells, self.opt, 64, st)
            self.tdma, self.tdma_score, self.frag, self.assign = st.tdma, st.tdma_score, st.frag, st.assign
            if self.acquire:
                self.cell_state = st.cell_state
                self.acquired |= ngood > 0
            if self.sdu:
                self.lost_sdus += self.rx.frag_stats["lost"]
            return frames
        kw = {"mac": True} if self.mac else {}
        if self.link_quality:
            kw["link_quality"] = True
        if self.traffic:
            kw["traffic"] = True
        if not self.acquire:
            return self.rx.decode(buf, self._cells, **kw)
        if self.vote:
            kw.update(score=self.cell_score, vote_cap=self.vote_cap)
        if self.traffic:
            kw["acquired"] = self.acquired
        frames, self.cell_state, ngood = self.rx.decode_acquire(buf, self.cell_state, **kw)
        self.acquired |= ngood > 0
        return frames

    def decode(self, x):
        """x: the next samples of the capture -> per carrier the frames first decoded now, each with
        "stream_sample" (its start in the carrier's 72 kHz stream)."""
        x, _ = _capture(x)
        tail = self.tail
        if len(tail) and tail.dtype != x.dtype:   # the format changed: go on in complex64
            tail, x = (sc16_to_cf32(a) if a.dtype == np.int16 else a for a in (tail, x))
        buf = np.concatenate([tail, x]) if len(tail) else x
        _, n72 = self.rx.plan.lengths(len(buf))
        out = [[] for _ in range(self.M)]
        T = max(0, (n72 - self.CARRY_Y) // self.ups) * self.per   # the next buffer starts here
        dy = self.ups * (T // self.per)                            # ... this many 72 kHz outputs on
        assert not self.timebase or dy % 2 == 0, "a buffer starts a whole number of bits after the previous one"
        if n72 < 16 and self.timebase:   # (nothing decoded: no burst, no expiry, the scores stay)
            self.tdma["bit0"] += dy // 2
            if self.sdu:
                self.frag["bit0"] += dy // 2
            if self.follow:
                self.assign["bit0"] += dy // 2
        if n72 >= 16:
            for k, fr in enumerate(self._decode_buffer(buf, dy // 2)):
                for f in fr:
                    a = self.y0 + f["sample"]
                    if a > self.last[k] + self.tol:
                        f["stream_sample"] = int(a)
                        out[k].append(f)
                        self.last[k] = a
        self.tail = buf[T:].copy()   # (the buffer may be the caller's array)
        self.y0 += dy
        return out


def planted_slots(seed, M, nb):
    """[M, nb] slot counts the synthesiser's slot grid (tetra_synth_set_grid) plants: carrier k's burst
    b carries (tetra_synth_slot0(seed, k) + b) mod 4320 in its SYNC PDU, when it is an SB."""
    L = _hip.lib()
    s0 = np.array([L.tetra_synth_slot0(seed, k) for k in range(M)], np.int64)
    return (s0[:, None] + np.arange(nb)[None, :]) % _hip.TDMA_SLOTS


def synth_wideband(Nw, seed=1, snr_db=30.0, cfo_max=300.0, fs=FS_WB, M=M_WB, oversample=None, grid=False):
    """Synthetic capture (device-generated, copied to the host): x [Nw] complex64, cells [M],
    kinds [M][NB], payload [M][NB][2][268], t0 [M] (carrier k is FFT bin k, at +k fs/M).  grid=True:
    the SBs' SYNC PDUs carry consecutive slot counts (planted_slots) instead of random TN / FN / MN."""
    plan = wb_plan(fs, M, oversample)
    c = _hip.ctx()
    nbb = Nw // plan.D + 1
    nb = c.lib.tetra_synth_bursts_per_channel(nbb, fs / plan.D)
    x = np.empty(Nw, np.complex64)
    cells = np.empty(M, np.uint32)
    kinds = np.empty((M, nb), np.int32)
    payload = np.empty((M, nb, 2, 268), np.uint8)
    t0 = np.empty(M, np.float64)
    if grid:
        c.check(c.lib.tetra_synth_set_grid(c.handle, 1), "synth_set_grid")
    try:
        c.check(c.lib.tetra_synth_wideband(c.handle, plan.c, Nw, seed, snr_db, cfo_max, _hip.ptr(x), _hip.ptr(cells),
                                           _hip.ptr(kinds), _hip.ptr(payload), _hip.ptr(t0)), "synth_wideband")
    finally:
        if grid:
            c.check(c.lib.tetra_synth_set_grid(c.handle, 0), "synth_set_grid")
    return x, cells, kinds, payload, t0


class BenchStep:
    """bench.py --chain wideband (C3): one step = the capture's waterfall rows (2048-pt Hann, hop
    2048), channelise the device-resident 20 MSps capture, timing + decision on every (carrier,
    chunk), lower MAC (sync, Viterbi, CRC) on all of them.  TETRA_WB_CELLS=acquire (default
    "given": every carrier's synthesised cell is configured): the lower MAC acquires each carrier's
    cell itself over all of its chunks (tetra_lmac_etsi_acquire_groups), the M inits kept on the
    device from step to step with the context that runs the lower MAC; TETRA_WB_CELLS=vote: the same
    by tetra_lmac_etsi_vote_groups, the scores in cell_score [M].  TETRA_WB_MAC=timebase: the
    capture is synthesised on the slot grid and tetra_etsi_mac_groups follows the lower MAC on the same
    context (PDU headers, the merge of each carrier's chunk rows, one TDMA timebase per carrier resident
    on the device; every step decodes the same capture, so bit0 does not advance).  TETRA_WB_MAC=vote: the
    same with tetra_etsi_link_quality and then tetra_etsi_mac_vote_groups in its place (the scores in
    tdma_score [M], the ballots in tvote [M, 4]; for tools/probe_tdma_vote.py).  TETRA_WB_IQ=sc16
    (default cf32): the capture is resident as the radio's int16 pairs -- the synthesised sum of 800
    carriers scaled by the smallest power of two that brings it into full scale, rounded -- and the
    channeliser and the waterfall take it as TETRA_SC16."""
    dtype = "f32 (DSP), int8/int32 (Viterbi)"

    @staticmethod
    def iq_format():
        """TETRA_WB_IQ: "cf32" (default) or "sc16"."""
        iq = os.environ.get("TETRA_WB_IQ", "cf32")
        if iq not in ("cf32", "sc16"):
            raise ValueError(f"TETRA_WB_IQ={iq!r}: cf32 or sc16")
        return iq

    @staticmethod
    def sc16_shift(peak):
        """The smallest k >= 0 with peak * 2^-k * 32768 <= 32767 (peak = max(|re|, |im|) of the capture)."""
        k = 0
        while peak * 2.0 ** -k * 32768.0 > 32767.0:
            k += 1
        return k

    def __init__(self, c, Nw, seed, device, snr_db=30.0, fs=FS_WB, M=M_WB):
        import torch
        self.c, self.Nw, self.fs = c, Nw, fs
        self.iq_name = self.iq_format()
        self.fmt = _hip.TETRA_SC16 if self.iq_name == "sc16" else _hip.TETRA_CF32
        self.plan = wb_plan(fs, M)
        self.etsi = etsi_plan(2.4e6)
        self.ck = chunking(self.plan, Nw)
        self.nchunk, self.m2 = self.ck.nchunk, self.ck.stride
        self.C = M * self.nchunk
        self.sm = self.ck.length // 4 + 2
        nbb = Nw // self.plan.D + 1
        nb = c.lib.tetra_synth_bursts_per_channel(nbb, fs / self.plan.D)
        self.x = torch.empty((Nw, 2), dtype=torch.float32, device=device)
        cells = torch.empty(M, dtype=torch.int32, device=device)
        self.kinds = torch.empty((M, nb), dtype=torch.int32, device=device)
        self.payload = torch.empty((M, nb, 2, 268), dtype=torch.uint8, device=device)
        mac = os.environ.get("TETRA_WB_MAC", "")
        if mac not in ("", "timebase", "vote"):
            raise ValueError(f"TETRA_WB_MAC={mac!r}: timebase, vote, or unset")
        self.timebase, self.seed = mac in ("timebase", "vote"), seed
        self.tdma_vote = mac == "vote"   # the timebase by tetra_etsi_mac_vote_groups
        if self.timebase:
            c.check(c.lib.tetra_synth_set_grid(c.handle, 1), "synth_set_grid")
        c.check(c.lib.tetra_synth_wideband(c.handle, self.plan.c, Nw, seed, snr_db, 300.0, _hip.ptr(self.x),
                                           _hip.ptr(cells), _hip.ptr(self.kinds), _hip.ptr(self.payload), None),
                "synth_wideband")
        if self.timebase:
            c.check(c.lib.tetra_synth_set_grid(c.handle, 0), "synth_set_grid")
        c.synchronize()   # torch's ops below need not share the context's stream
        if self.iq_name == "sc16":   # only the int16 capture is kept
            self.sc16_k = self.sc16_shift(float(self.x.abs().max()))
            self.x = torch.round(self.x * (32768.0 * 2.0 ** -self.sc16_k)).clamp_(-32768, 32767).to(torch.int16)
        # every chunk of carrier k uses carrier k's scrambling code
        self.cells = cells.repeat_interleave(self.nchunk).contiguous()
        self.cells_carrier = cells
        mode = os.environ.get("TETRA_WB_CELLS", "given")
        if mode not in ("given", "acquire", "vote"):
            raise ValueError(f"TETRA_WB_CELLS={mode!r}: given, acquire or vote")
        self.acquire = mode in ("acquire", "vote")
        self.vote = mode == "vote"   # acquisition by tetra_lmac_etsi_vote_groups, the scores in cell_score [M]
        if self.vote:
            self.cell_score = torch.zeros(M, dtype=torch.int32, device=device)
            self.agree = torch.zeros(M, dtype=torch.int32, device=device)
        if self.acquire:   # the acquisition state: one init per carrier (3 = unknown), CRC-good BSCH counts
            self.cells_mode = mode
            self.cells_true = cells
            self.cell_state = torch.full((M,), 3, dtype=torch.int32, device=device)
            self.ngood = torch.zeros(M, dtype=torch.int32, device=device)
        torch.cuda.current_stream(device).synchronize()
        if not self.acquire:
            c.check(c.lib.tetra_etsi_set_cells(c.handle, _hip.ptr(self.cells), self.C), "set_cells")
        self.y = torch.empty((M, self.ck.rowlen, 2), dtype=torch.float32, device=device)
        # the timing's Oerder-Meyr class sums from the resampler (grouped_om): its group partials
        self.om_grouped = grouped_om(self.plan, self.m2)
        self.ngrp = -(-self.ck.rowlen // self.plan.c.up)
        self.om = torch.empty((M, self.ngrp, 4), dtype=torch.float32, device=device) if self.om_grouped else None
        self.sym = torch.empty((self.C, self.sm, 2), dtype=torch.float32, device=device)
        self.soft = torch.empty((self.C, 2 * self.sm), dtype=torch.int8, device=device)
        self.hard = torch.empty((self.C, self.sm), dtype=torch.uint8, device=device)
        self.nsym = torch.empty(self.C, dtype=torch.int32, device=device)
        self.nburst = torch.empty(self.C, dtype=torch.int32, device=device)
        self.bursts = torch.empty((self.C, _hip.ETSI_MAXB, 2), dtype=torch.int32, device=device)
        self.nblock = torch.empty(self.C, dtype=torch.int32, device=device)
        self.blocks = torch.empty((self.C, _hip.ETSI_MAXJ, 4), dtype=torch.int32, device=device)
        self.type1 = torch.empty((self.C, _hip.ETSI_MAXJ, 268), dtype=torch.uint8, device=device)
        if self.timebase:
            if self.m2 % 2:
                raise ValueError(f"TETRA_WB_MAC=timebase works in bits: m2 ({self.m2}) must be even")
            self.tdma = torch.zeros((M, 3), dtype=torch.int64, device=device)   # struct tetra_etsi_tdma per carrier
            self.keep = torch.zeros((self.C, _hip.ETSI_MAXB), dtype=torch.int32, device=device)
            self.slots = torch.zeros((self.C, _hip.ETSI_MAXB, _hip.SLOT_FIELDS), dtype=torch.int32, device=device)
            self.npdu = torch.zeros((self.C, _hip.ETSI_MAXJ), dtype=torch.int32, device=device)
            self.pdus = torch.zeros((self.C, _hip.ETSI_MAXJ, _hip.ETSI_MAXPDU, _hip.PDU_FIELDS), dtype=torch.int32,
                                    device=device)
            if self.tdma_vote:
                self.bq = torch.zeros((self.C, _hip.ETSI_MAXB, _hip.LQ_FIELDS), dtype=torch.int32, device=device)
                self.kq = torch.zeros((self.C, _hip.ETSI_MAXJ, _hip.LQ_FIELDS), dtype=torch.int32, device=device)
                self.tdma_score = torch.zeros(M, dtype=torch.int32, device=device)
                self.tvote = torch.zeros((M, _hip.TV_FIELDS), dtype=torch.int32, device=device)
            torch.cuda.current_stream(device).synchronize()
        self.nfr = Nw // 2048   # waterfall rows of the capture (2048-pt Hann frames, hop 2048)
        self.wf = torch.empty((self.nfr, 2048), dtype=torch.float32, device=device)
        self.pipelined = False
        self.mid = None

    def pipeline(self):
        """Software pipeline over consecutive captures: the channeliser of step k+2 on the front
        stream while the per-carrier timing of step k+1 runs on a middle stream and the waterfall rows
        and the lower MAC of step k on a back stream (each its own context).  The carrier samples y
        (with their Oerder-Meyr partials) and the timing's outputs are what crosses the streams:
        double-buffered, each stage waits only on the events that protect its buffers.  Every step
        still does the whole chain."""
        import torch
        dev = self.x.device
        self.back = _hip.Context()
        # the waterfall rows go on the back stream, beside the channeliser (the front stream, the longer
        # of the two): 0.436 against 0.446 ms per step, same box (profiles/r04_ab_wideband_streams.txt);
        # TETRA_WB_WF_BACK=0 keeps them on the front.  TETRA_WB_FRONT_PRIO=1 runs the channeliser on a
        # high-priority stream of its own (no gain)
        self.wf_back = os.environ.get("TETRA_WB_WF_BACK", "1") == "1"
        if os.environ.get("TETRA_WB_FRONT_PRIO") == "1":
            self.s_front = torch.cuda.Stream(device=dev, priority=-1)
            self.c.check(self.c.lib.tetra_set_stream(self.c.handle, ctypes.c_void_p(self.s_front.cuda_stream)),
                         "set_stream")
        else:
            self.s_front = torch.cuda.current_stream(dev)
        self.s_back = torch.cuda.Stream(device=dev)
        self.back.check(self.back.lib.tetra_set_stream(self.back.handle, ctypes.c_void_p(self.s_back.cuda_stream)),
                        "set_stream")
        if not self.acquire:   # (acquisition: the back context builds its table from the state it is handed)
            self.back.check(self.back.lib.tetra_etsi_set_cells(self.back.handle, _hip.ptr(self.cells), self.C),
                            "set_cells")
        self.ys = [self.y, torch.empty_like(self.y)]
        self.oms = [self.om, torch.empty_like(self.om) if self.om is not None else None]
        self.ev_front = [torch.cuda.Event() for _ in range(2)]
        self.ev_back = [torch.cuda.Event() for _ in range(2)]
        for e in self.ev_back:
            e.record(self.s_back)
        # three streams (default): the timing on a middle stream of its own, the lower MAC (and the
        # waterfall rows) on the back stream -- three captures in flight; the timing's outputs (symbols,
        # soft bits, dibits, counts) are then double-buffered too.  Same box: 0.386-0.387 ms per step
        # against 0.397-0.415 with two streams (profiles/r04_ab_wb_stages.txt).  TETRA_WB_STAGES=2: the
        # two-stream form (timing + lower MAC on the back stream)
        self.mid = None
        if os.environ.get("TETRA_WB_STAGES", "3") == "3":
            self.mid = _hip.Context()
            self.s_mid = torch.cuda.Stream(device=dev)
            self.mid.check(self.mid.lib.tetra_set_stream(self.mid.handle, ctypes.c_void_p(self.s_mid.cuda_stream)),
                           "set_stream")
            self.outs = [(self.sym, self.soft, self.hard, self.nsym)]
            self.outs.append(tuple(torch.empty_like(t) for t in self.outs[0]))
            self.ev_mid = [torch.cuda.Event() for _ in range(2)]
            for e in self.ev_mid:
                e.record(self.s_mid)
        self.k = 0
        self.pipelined = True
        return self

    def contexts(self):
        return [self.c] + ([self.back] if self.pipelined else []) + ([self.mid] if self.mid is not None else [])

    def _waterfall(self, c):
        c.check(c.lib.tetra_waterfall(c.handle, _hip.ptr(self.x), self.fmt, 1, self.Nw, 2048, 2048, self.nfr,
                                      _hip.ptr(self.wf)), "waterfall")

    def _front(self, c, y, om):
        if not (self.pipelined and self.wf_back):
            self._waterfall(c)
        if om is not None:
            c.check(c.lib.tetra_channelize_om_fmt(c.handle, self.plan.c, _hip.ptr(self.x), self.fmt, self.Nw,
                                                  _hip.ptr(y), self.ck.rowlen, _hip.ptr(om)), "channelize_om")
        else:
            c.check(c.lib.tetra_channelize_fmt(c.handle, self.plan.c, _hip.ptr(self.x), self.fmt, self.Nw,
                                               _hip.ptr(y), self.ck.rowlen), "channelize")

    def _timing(self, c, y, om):
        ck = self.ck
        c.check(c.lib.tetra_etsi_timing_chunks(c.handle, self.etsi, _hip.ptr(y), self.plan.M, ck.rowlen, ck.nchunk,
                                               ck.stride, ck.length, _hip.ptr(om), self.ngrp if om is not None else 0,
                                               self.plan.c.up, _hip.ptr(self.sym), _hip.ptr(self.soft),
                                               _hip.ptr(self.hard), _hip.ptr(self.nsym), self.sm, None),
                "etsi_timing_chunks")

    def _quality(self, c):
        """tetra_etsi_link_quality on the rows the lower MAC read (intact: origin 0), every carrier's rows
        with its configured or acquired cell."""
        c.check(c.lib.tetra_etsi_link_quality(c.handle, _hip.ptr(self.soft), _hip.ptr(self.hard), self.C, self.sm, 0,
                                              self.nchunk, _hip.ptr(self.cell_state if self.acquire else
                                                                    self.cells_carrier),
                                              _hip.ptr(self.nburst), _hip.ptr(self.bursts), _hip.ptr(self.nblock),
                                              _hip.ptr(self.blocks), _hip.ptr(self.type1), _hip.ptr(self.bq),
                                              _hip.ptr(self.kq)), "etsi_link_quality")

    def _mac_vote(self, c):
        c.check(c.lib.tetra_etsi_mac_vote_groups(c.handle, _hip.ptr(self.nsym), self.C, self.nchunk, self.m2 // 2, 32, 0,
                                                 _hip.TETRA_TDMA_VOTE_CAP_DEFAULT, _hip.ptr(self.nburst),
                                                 _hip.ptr(self.bursts), _hip.ptr(self.nblock), _hip.ptr(self.blocks),
                                                 _hip.ptr(self.type1), _hip.ptr(self.bq), _hip.ptr(self.kq),
                                                 _hip.ptr(self.tdma), _hip.ptr(self.tdma_score), _hip.ptr(self.keep),
                                                 _hip.ptr(self.slots), _hip.ptr(self.npdu), _hip.ptr(self.pdus),
                                                 _hip.ptr(self.tvote)), "etsi_mac_vote_groups")

    def _mac(self, c):
        c.check(c.lib.tetra_etsi_mac_groups(c.handle, _hip.ptr(self.nsym), self.C, self.nchunk, self.m2 // 2, 32, 0,
                                            _hip.ptr(self.nburst), _hip.ptr(self.bursts), _hip.ptr(self.nblock),
                                            _hip.ptr(self.blocks), _hip.ptr(self.type1), _hip.ptr(self.tdma),
                                            _hip.ptr(self.keep), _hip.ptr(self.slots), _hip.ptr(self.npdu),
                                            _hip.ptr(self.pdus)), "etsi_mac_groups")

    def _lmac(self, c):
        self._lmac_rows(c)
        if self.tdma_vote:
            self._quality(c)
            self._mac_vote(c)
        elif self.timebase:
            self._mac(c)

    def _lmac_rows(self, c):
        if self.acquire and self.vote:
            c.check(c.lib.tetra_lmac_etsi_vote_groups(c.handle, _hip.ptr(self.soft), _hip.ptr(self.hard),
                                                      _hip.ptr(self.nsym), self.C, self.sm, self.nchunk,
                                                      _hip.TETRA_ETSI_VOTE_CAP_DEFAULT, _hip.ptr(self.cell_state),
                                                      _hip.ptr(self.cell_score), _hip.ptr(self.ngood),
                                                      _hip.ptr(self.agree), _hip.ptr(self.nburst), _hip.ptr(self.bursts),
                                                      _hip.ptr(self.nblock), _hip.ptr(self.blocks),
                                                      _hip.ptr(self.type1)), "lmac_etsi_vote_groups")
            return
        if self.acquire:
            c.check(c.lib.tetra_lmac_etsi_acquire_groups(c.handle, _hip.ptr(self.soft), _hip.ptr(self.hard),
                                                         _hip.ptr(self.nsym), self.C, self.sm, self.nchunk,
                                                         _hip.ptr(self.cell_state), _hip.ptr(self.ngood),
                                                         _hip.ptr(self.nburst), _hip.ptr(self.bursts),
                                                         _hip.ptr(self.nblock), _hip.ptr(self.blocks),
                                                         _hip.ptr(self.type1)), "lmac_etsi_acquire_groups")
            return
        c.check(c.lib.tetra_lmac_etsi(c.handle, _hip.ptr(self.soft), _hip.ptr(self.hard), _hip.ptr(self.nsym), self.C,
                                      self.sm, _hip.ptr(self.nburst), _hip.ptr(self.bursts), _hip.ptr(self.nblock),
                                      _hip.ptr(self.blocks), _hip.ptr(self.type1)), "lmac_etsi")

    def _back(self, c, y, om):
        if self.pipelined and self.wf_back:
            self._waterfall(c)
        self._timing(c, y, om)
        self._lmac(c)

    def __call__(self):
        if not self.pipelined:
            self._front(self.c, self.y, self.om)
            self._back(self.c, self.y, self.om)
            return
        i = self.k & 1
        self.k += 1
        y, om = self.ys[i], self.oms[i]
        self.s_front.wait_event(self.ev_back[i] if self.mid is None else self.ev_mid[i])   # y[i], om[i] consumed
        self._front(self.c, y, om)
        self.ev_front[i].record(self.s_front)
        if self.mid is None:
            self.s_back.wait_event(self.ev_front[i])
            self._back(self.back, y, om)
            self.ev_back[i].record(self.s_back)
            return
        # three streams: timing of this capture on the middle one once its channeliser is done and the
        # lower MAC two captures back has consumed output buffer i; the lower MAC on the back one
        self.sym, self.soft, self.hard, self.nsym = self.outs[i]
        self.s_mid.wait_event(self.ev_front[i])
        self.s_mid.wait_event(self.ev_back[i])
        self._timing(self.mid, y, om)
        self.ev_mid[i].record(self.s_mid)
        self.s_back.wait_event(self.ev_mid[i])
        if self.wf_back:
            self._waterfall(self.back)
        self._lmac(self.back)
        self.ev_back[i].record(self.s_back)

    def stage_bytes(self):
        """Algorithmic bytes per wideband input sample of each timed stage (cf32 = 8 B, SC16 = 4 B in):
        the fused analysis (M = 800) and the fold read x and write Y (M per D samples), the FFT reads and writes Y, the resampler reads
        Y and writes y (M carriers at 72 kHz), the timing stage reads y and writes per symbol an
        8 B symbol, 2 soft bits and a hard dibit -- the samples two chunks share twice (cover =
        the chunks' total length over the row's).  bench.py reports the slowest of them."""
        M, D, fs, ck = self.plan.M, self.plan.D, self.fs, self.ck
        yb = 8.0 * M * 72000.0 / fs
        cover = ((ck.nchunk - 1) * ck.length + ck.rowlen - (ck.nchunk - 1) * ck.stride) / ck.rowlen
        xb = 4.0 if self.iq_name == "sc16" else 8.0   # input bytes per sample
        # (SC16 in front of the two-block form: its conversion pass is the stage "wb_sc16", not counted)
        ana = "k_pfb_analysis2" if os.environ.get("TETRA_WB_ANALYSIS") == "2" else \
            (("k_pfb_analysis1" if self.plan.oversample == 2 else "k_pfb_analysis") + ("_sc16" if self.iq_name == "sc16" else ""))
        return {"waterfall": ((xb + 4.0) * self.nfr * 2048 / self.Nw, "k_waterfall"),
                "wb_analysis": (xb + 8.0 * M / D, ana),   # fused fold + FFT: x in, Y out
                "wb_fold": (xb + 8.0 * M / D, "k_pfb_fold"), "wb_fft": (2 * 8.0 * M / D, None),
                "wb_resamp": (8.0 * M / D + yb + (yb * 2.0 / self.plan.c.up if self.om_grouped else 0.0),
                              "k_pfb_resamp_fix"),
                "etsi_timing": (cover * (yb + 11.0 * M * 18000.0 / fs), "k_timing")}

    def config(self, world):
        return {"workload": f"C3: {self.Nw} {'SC16 ' if self.iq_name == 'sc16' else ''}samples of a {self.fs / 1e6:g} MSps capture per GPU, "
                            f"{self.plan.M} carriers x {self.nchunk} timing chunks of {self.ck.length} "
                            f"every {self.m2}",
                "wideband_samples_per_gpu": self.Nw, "sample_rate": self.fs, "carriers": self.plan.M,
                "timing_chunks_per_carrier": self.nchunk, "timing_chunk_overlap": self.ck.length - self.m2,
                "parallelism": f"capture-sharded x{world}",
                "filter_bank": f"D = M / {self.plan.oversample} ({self.fs / self.plan.D / 1e3:g} kHz carriers)",
                "pipeline": self.pipelined,
                # (bench.py adds cells_mode itself only to the config it builds for steps without one)
                **({"cells": self.cells_mode} if self.acquire else {}),
                **({"mac": "vote" if self.tdma_vote else "timebase"} if self.timebase else {}),
                **({"iq": "sc16", "sc16_scale": f"2^-{self.sc16_k}"} if self.iq_name == "sc16" else {})}

    def realtime_channels(self, value_msps):
        return value_msps * 1e6 / self.fs * self.plan.M   # carriers served at real time

    def workload_key(self):
        # a substring of config()["workload"]; an SC16 step's says so ("... SC16 samples"), and neither
        # key is a substring of the other's workload, so a profile summary of one format is never read
        # for the other
        return f"C3: {self.Nw} samples" if self.iq_name == "cf32" else f"C3: {self.Nw} SC16 samples"

    def quality(self):
        """The last step's decoded work, each burst once (merge_chunks): bursts, blocks, CRC-good
        blocks, and decoded_frac = bursts / the slots on air (M rows of rowlen samples, 1020 per
        slot; a slot cut by the capture's start or end cannot be decoded, so ~0.97-0.99 is whole).
        TETRA_WB_CELLS=acquire adds cells_acquired: the carriers whose state is the synthesised cell.
        TETRA_WB_MAC=timebase adds timebase_known, the share of kept bursts with a slot (tn != 0), and
        timebase_wrong, the kept, known bursts whose slot is not the planted one (a burst is matched
        to its planted one by its first block's type-1 bits, so only CRC-good ones are judged;
        timebase_checked counts them)."""
        nb, bursts = self.nburst.cpu().numpy(), self.bursts.cpu().numpy()
        nk, blocks = self.nblock.cpu().numpy(), self.blocks.cpu().numpy()
        keep, kb = merge_chunks(nb, bursts, nk, blocks, self.plan.M, self.nchunk, self.m2)
        tb = {}
        if self.timebase:
            dkeep = self.keep.cpu().numpy().astype(bool) & (np.arange(keep.shape[1])[None, :] < nb[:, None])
            if self.tdma_vote:   # the vote keeps a burst's best copy: one per burst as merge_chunks, maybe another
                if dkeep.sum() != keep.sum():
                    raise RuntimeError("tetra_etsi_mac_vote_groups keeps another number of bursts than merge_chunks")
                tb = dict(keep_differs=int((dkeep != keep).sum() // 2), tvote=self.tvote.cpu().numpy().sum(axis=0).tolist())
                keep = dkeep
                live = np.arange(kb.shape[1])[None, :] < np.clip(nk, 0, kb.shape[1])[:, None]
                kb = live & np.take_along_axis(keep, np.clip(blocks[..., 2], 0, keep.shape[1] - 1), axis=1)
            elif not np.array_equal(dkeep, keep):
                raise RuntimeError("tetra_etsi_mac_groups' keep differs from merge_chunks'")
            tb.update(self._timebase_quality(keep, nk, blocks))
        slots = self.plan.M * self.ck.rowlen / BURST_SAMPLES
        return dict(blocks=int(kb.sum()), crc_ok=int((blocks[..., 1].astype(bool) & kb).sum()),
                    bursts=int(keep.sum()), decoded_frac=round(float(keep.sum()) / slots, 4),
                    per_chunk=dict(bursts=int(nb.sum()), blocks=int(nk.sum())),
                    **({"cells_acquired": int((self.cell_state == self.cells_true).sum())} if self.acquire else {}),
                    **tb)

    def _timebase_quality(self, keep, nk, blocks):
        slots, t1 = self.slots.cpu().numpy(), self.type1.cpu().numpy()
        kinds, payload = self.kinds.cpu().numpy(), self.payload.cpu().numpy()
        planted = planted_slots(self.seed, self.plan.M, kinds.shape[1])
        known = slots[..., 0] != 0
        wrong = checked = 0
        for ch, b in zip(*np.nonzero(keep & known)):
            k = ch // self.nchunk
            j = next((j for j in range(min(int(nk[ch]), _hip.ETSI_MAXJ)) if blocks[ch, j, 2] == b and blocks[ch, j, 3] == 0), None)
            if j is None or not blocks[ch, j, 1]:
                continue
            n1 = (268, 124, 60)[int(blocks[ch, j, 0])]
            hit = np.nonzero((payload[k, :, 0, :n1] == (t1[ch, j, :n1] & 1)).all(axis=1))[0]
            if len(hit) != 1:
                continue
            s = int(planted[k, hit[0]])
            checked += 1
            wrong += slots[ch, b, :3].tolist() != [s % 4 + 1, s // 4 % 18 + 1, s // 72 + 1]
        return dict(timebase_known=round(float((keep & known).sum()) / max(int(keep.sum()), 1), 4),
                    timebase_wrong=int(wrong), timebase_checked=int(checked))
