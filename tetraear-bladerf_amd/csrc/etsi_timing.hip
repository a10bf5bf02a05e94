// etsi_timing.hip -- the ETSI timing stage as a kernel of its own, and the small kernels beside it.
//
//   k_timing     one wave per channel: Oerder-Meyr timing phase (wave reduction), block Gardner
//                tracking (64 symbols per block = one per lane; error summed by xor-butterfly),
//                cubic interpolation, differential decision, 4th-power CFO estimate, int8 soft bits
//                (the loop itself: etsi_timing.h, shared with the fused demod).
//   k_track_skip a streaming window too short for the filter: the carried loops' positions move on.
//   k_etsi_decide  the differential decision alone, on given symbol-spaced samples.
#include <cstdlib>

#include "etsi_timing.h"

namespace {

// clk (probe, TETRA_TIMING_PROBE=1 with a diag buffer): the wave's wall-clock stamps at its start, after
// the Oerder-Meyr pass, after the Gardner loop and at its end, in place of the diagnostics
template <int RING = 0, bool LEAN = false, bool OMC = false>
__device__ __forceinline__ void timing_wave(const float2 *y, int M2, float gain, float soft_scale, float2 *sp,
                                            float2 *dp, int8_t *sb, uint8_t *hp, int32_t *nsym_ch, float4 *diag_ch,
                                            int smax, int lane, float2 *ring = nullptr, uint32_t *clk = nullptr,
                                            float4 omc = float4{}, tetra_etsi_track *trk = nullptr, int yoff = 0) {
    if (!OMC && clk && lane == 0) clk[0] = (uint32_t)wall_clock64();   // OMC: stamped before the class sums
    const TrackIn ti = track_in(trk, yoff);
    const TrackOut o = timing_track<false, RING, LEAN, OMC>(y, M2, gain, soft_scale, sp, dp, smax, lane, nullptr,
                                                            nullptr, ring, clk, omc, ti);
    if (trk && lane == 0) track_store(trk, ti, o, M2);
    if (clk && lane == 0) clk[2] = (uint32_t)wall_clock64();
    __threadfence_block();   // dp / sp written by other lanes is read below
    if constexpr (LEAN)
        timing_decide_sym(o, sp, sb, hp, lane);
    else
        timing_decide(o, dp, sb, hp, 0, 1, lane);
    if (lane == 0) {
        *nsym_ch = o.S;
        if (clk) {
            __builtin_amdgcn_s_waitcnt(0);   // the decision pass's stores issued and done
            clk[3] = (uint32_t)wall_clock64();
        } else if (diag_ch) {   // fewer than 16 samples: no timing ran, zeros (not what the buffer held)
            *diag_ch = M2 >= 16 ? make_float4(o.base, o.delta, o.rr, o.ri) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// The Oerder-Meyr class sums of the chunk row[s, e) in the wideband grouped order (oracle
// eo_om_grouped): P holds the carrier row's resampler group partials (U outputs per group, s a
// multiple of 4).  Lane l sums the whole groups g0 + l, g0 + l + 64, ... then a wave butterfly; the
// head [s, U g0) and the tail [U g1, e) (each < U <= 64 samples, one per lane) are summed class by
// class in ascending n.
__device__ __forceinline__ float4 om_grouped(const float2 *__restrict__ row, const float4 *__restrict__ P, long s,
                                             long e, int U, int lane) {
    const long g0 = (s + U - 1) / U, g1 = e / U;
    const long hend = min((long)U * g0, e), tbeg = max((long)U * g1, hend);
    // head and tail samples first (their loads in flight with the partials')
    const long hi = s + lane, ti = tbeg + lane;
    const float2 hv = hi < hend ? row[hi] : make_float2(0.f, 0.f);
    const float2 tv = ti < e ? row[ti] : make_float2(0.f, 0.f);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long g = g0 + lane; g < g1; g += 64) {
        const float4 p = P[g];
        v.x = v.x + p.x;
        v.y = v.y + p.y;
        v.z = v.z + p.z;
        v.w = v.w + p.w;
    }
    const float ph = fmaf(hv.x, hv.x, hv.y * hv.y), pt = fmaf(tv.x, tv.x, tv.y * tv.y);
    wave_sum2(v.x, v.y);
    wave_sum2(v.z, v.w);
    float h[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f};
    const int nh = (int)(hend - s), nt = (int)(e - tbeg);   // < U <= 64
    for (int i = 0; i < nh; ++i) h[i & 3] = h[i & 3] + lane_f(ph, i);
    for (int i = 0; i < nt; ++i) t[i & 3] = t[i & 3] + lane_f(pt, i);
    return make_float4((h[0] + v.x) + t[0], (h[1] + v.y) + t[1], (h[2] + v.z) + t[2], (h[3] + v.w) + t[3]);
}

// Chunked rows (cstride > 0: tetra_etsi_timing_chunks / _om): block ch is chunk c = ch mod nchunk of
// carrier k = ch / nchunk, the samples yall[k rowlen + c cstride, ...) up to M2 of them or the row's
// end (chunks may overlap); cstride = 0: block ch is yall[ch M2, (ch + 1) M2).
// OMG (the _om forms): the Oerder-Meyr class sums from the resampler's group partials (om: ngrp
// float4 per carrier row)
template <int RING, bool LEAN, bool OMG = false>
__global__ __launch_bounds__(64) void k_timing(const float2 *__restrict__ yall, int M2, float gain, float soft_scale,
                                               float2 *__restrict__ sym, float2 *__restrict__ dscr,
                                               int8_t *__restrict__ softbits, uint8_t *__restrict__ hard,
                                               int32_t *__restrict__ nsym, int smax, float4 *__restrict__ diag,
                                               int probe, const float4 *__restrict__ om, int nchunk, int ngrp, int U,
                                               tetra_etsi_track *__restrict__ trk, int yoff, int ostride, int cstride,
                                               long rowlen) {
    __shared__ float2 ring[RING ? TRING : 1];
    const int ch = blockIdx.x;
    uint32_t *clk = probe && diag ? reinterpret_cast<uint32_t *>(diag + ch) : nullptr;
    const float2 *y = yall + (size_t)ch * M2;
    int L = M2;
    float4 omc = float4{};
    if (cstride > 0) {
        const int k = ch / nchunk;
        const long s = (long)(ch - k * nchunk) * cstride;
        L = (int)min((long)M2, rowlen - s);
        const float2 *row = yall + (size_t)k * rowlen;
        y = row + s;
        if constexpr (OMG) {
            if (clk && threadIdx.x == 0) clk[0] = (uint32_t)wall_clock64();
            omc = om_grouped(row, om + (size_t)k * ngrp, s, s + L, U, threadIdx.x);
        }
    }
    const size_t os = ostride ? (size_t)ostride : (size_t)smax;   // output rows (streaming: reserve + smax)
    timing_wave<RING, LEAN, OMG>(y, L, gain, soft_scale, sym + (size_t)ch * os,
                                 dscr ? dscr + (size_t)ch * smax : nullptr, softbits + (size_t)ch * 2 * os,
                                 hard + (size_t)ch * os, nsym + ch, diag ? diag + ch : nullptr, smax, threadIdx.x, ring,
                                 clk, omc, trk ? trk + ch : nullptr, yoff);
}
// k_timing's form (same-box A/B): TETRA_TIMING_RING = 0 (the Gardner windows read straight from
// global memory), 1 (one block ahead, default) or 2 (two); TETRA_TIMING_LEAN = 0 keeps om_part per
// quarter for the Oerder-Meyr pass and the d_j round trip through dscr (default 1: om_all, d_j
// recomputed from the symbols)
using timing_fn = void (*)(const float2 *, int, float, float, float2 *, float2 *, int8_t *, uint8_t *, int32_t *, int,
                           float4 *, int, const float4 *, int, int, int, tetra_etsi_track *, int, int, int, long);
static timing_fn timing_kernel(size_t M2, size_t smax, bool omg = false) {
    const char *r = getenv("TETRA_TIMING_RING"), *o = getenv("TETRA_TIMING_LEAN");
    // the ring form addresses y and the symbols through buffer resources (32-bit byte ranges)
    const bool fits = 8 * M2 < ((size_t)1 << 31) && 8 * smax < ((size_t)1 << 31);
    const int ring = !fits ? 0 : (r ? atoi(r) : 1);
    const bool lean = !(o && atoi(o) == 0);
    if (omg) return ring <= 0 ? k_timing<0, true, true> : k_timing<1, true, true>;
    if (ring <= 0) return lean ? k_timing<0, true> : k_timing<0, false>;
    if (ring == 1) return lean ? k_timing<1, true> : k_timing<1, false>;
    return lean ? k_timing<2, true> : k_timing<2, false>;
}

// ETSI differential decision on given symbol-spaced samples (SignalProcessor(mode="etsi")
// .demodulate_dqpsk): d = x[k] conj(x[k-1]), dibit = (Im d < 0, Re d < 0) -- EN 300 392-2 Table 5.1
// (00 +pi/4, 01 +3pi/4, 11 -3pi/4, 10 -pi/4), the fused demod's decision without its CFO rotation.
template <typename T>
__global__ __launch_bounds__(256) void k_etsi_decide(const T *__restrict__ x, long n, uint8_t *__restrict__ hard) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x + 1;
    if (k >= n) return;
    const float ar = (float)x[k].x, ai = (float)x[k].y, br = (float)x[k - 1].x, bi = (float)x[k - 1].y;
    const float dr = fmaf(ar, br, ai * bi), di = fmaf(ai, br, -(ar * bi));
    hard[k - 1] = (uint8_t)(((di < 0.0f) << 1) | (dr < 0.0f));
}

// A streaming window too short for the channel filter (M2 <= 0): no symbols, the acquired loops'
// positions move to the end of the (empty) window (track_store's M2 < 16 rule).
__global__ __launch_bounds__(256) void k_track_skip(tetra_etsi_track *__restrict__ tr, int C, int yoff, int M2) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch < C && tr[ch].acquired) tr[ch].base = tr[ch].base + (float)(yoff - M2);
}

}  // namespace

// TETRA_TIMING_PROBE=1: with a diag buffer, each chunk's diag entry holds four 32-bit wall-clock stamps
// (start, Oerder-Meyr done, Gardner done, end) instead of the diagnostics -- a latency probe
int timing_probe() {
    const char *e = getenv("TETRA_TIMING_PROBE");
    return e && atoi(e) == 1;
}

void launch_track_skip(tetra_ctx *ctx, tetra_etsi_track *tr, size_t C, int yoff, int M2) {
    hipLaunchKernelGGL(k_track_skip, dim3(grid_for(C, 256)), dim3(256), 0, ctx->stream, tr, (int)C, yoff, M2);
}

DemodOut stage_demod_out(Staging &st, void *soft, int8_t *softbits, uint8_t *hard, int32_t *nsym, float *diag,
                         size_t C, size_t stride) {
    return {(float2 *)st.out(soft, C * stride * 8), (int8_t *)st.out(softbits, C * stride * 2),
            (uint8_t *)st.out(hard, C * stride), (int32_t *)st.out(nsym, C * 4),
            diag ? (float4 *)st.out(diag, C * 16) : nullptr};   // (a braced list is evaluated in order)
}

void launch_timing(tetra_ctx *ctx, const tetra_etsi_plan *P, const float2 *y, size_t C, size_t M2, const DemodOut &o,
                   float2 *dscr, size_t smax, const TimingOpt &t) {
    PROF(ctx, "etsi_timing");
    hipLaunchKernelGGL(timing_kernel(M2, smax, t.om != nullptr), dim3((unsigned)C), dim3(64), 0, ctx->stream, y,
                       (int)M2, P->gain, P->soft_scale, o.sym, dscr, o.softbits, o.hard, o.nsym, (int)smax, o.diag,
                       timing_probe(), t.om, t.nchunk, t.ngrp, t.U, t.track, t.yoff, t.ostride, t.cstride, t.rowlen);
}

// The chunked timing both wideband entry points launch (cstride = the chunk stride, rowlen = the
// carrier rows' length): tetra_etsi_timing_om's chunks tile the rows, tetra_etsi_timing_chunks' overlap.
static int launch_timing_chunks(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *y, size_t M, size_t rowlen,
                                size_t nchunk, size_t stride, size_t len, const void *om, size_t ngrp, int U,
                                void *soft, int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax, float *diag) {
    const size_t C = M * nchunk;
    Staging st(ctx);
    const void *yd = st.in(y, M * rowlen * 8);
    const void *omd = om ? st.in(om, M * ngrp * 16) : nullptr;
    const DemodOut o = stage_demod_out(st, soft, softbits, hard, nsym, diag, C, smax);
    // the grouped form needs no d_j scratch: the LEAN form recomputes d_j from the stored symbols
    float2 *dscr = om ? nullptr : (float2 *)ws(ctx, S_W4, C * smax * 8);
    if (!yd || (om && !omd) || !o.ok() || (!om && !dscr)) return st.finish();
    TimingOpt t;
    t.om = (const float4 *)omd;
    t.ngrp = (int)ngrp;
    t.U = U;
    t.nchunk = (int)nchunk;
    t.cstride = (int)stride;
    t.rowlen = (long)rowlen;
    launch_timing(ctx, P, (const float2 *)yd, C, len, o, dscr, smax, t);
    return st.finish();
}

extern "C" {

int tetra_etsi_timing(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *y, size_t C, size_t M2, void *soft,
                      int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax, float *diag) {
    if (!ctx || !P || C == 0) return TETRA_E_INVALID;
    Staging st(ctx);
    const void *yd = st.in(y, C * M2 * 8);
    const DemodOut o = stage_demod_out(st, soft, softbits, hard, nsym, diag, C, smax);
    float2 *dscr = (float2 *)ws(ctx, S_W4, C * smax * 8);
    if (!yd || !o.ok() || !dscr) return st.finish();
    launch_timing(ctx, P, (const float2 *)yd, C, M2, o, dscr, smax);
    return st.finish();
}

int tetra_etsi_timing_om(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *y, size_t C, size_t M2,
                         const void *om, size_t nchunk, size_t ngrp, int U, void *soft, int8_t *softbits,
                         uint8_t *hard, int32_t *nsym, size_t smax, float *diag) {
    if (!ctx || !P || C == 0 || !om) return TETRA_E_INVALID;
    if (nchunk == 0 || C % nchunk || M2 % 4 || U < 4 || U > 64 || U % 4 || ngrp * (size_t)U < nchunk * M2 ||
        M2 < 16 || nchunk * M2 * 8 >= ((size_t)1 << 31))
        return tetra_fail(ctx, TETRA_E_INVALID, "timing_om: C a multiple of nchunk, M2 >= 16 a multiple of 4, "
                                                "4 <= U <= 64 a multiple of 4, ngrp U >= nchunk M2");
    return launch_timing_chunks(ctx, P, y, C / nchunk, nchunk * M2, nchunk, M2, M2, om, ngrp, U, soft, softbits, hard,
                                nsym, smax, diag);
}

int tetra_etsi_timing_chunks(tetra_ctx *ctx, const tetra_etsi_plan *P, const void *y, size_t M, size_t rowlen,
                             size_t nchunk, size_t stride, size_t len, const void *om, size_t ngrp, int U, void *soft,
                             int8_t *softbits, uint8_t *hard, int32_t *nsym, size_t smax, float *diag) {
    if (!ctx || !P || M == 0) return TETRA_E_INVALID;
    if (nchunk == 0 || stride == 0 || len < 16 || (nchunk - 1) * stride + 16 > rowlen ||
        rowlen * 8 >= ((size_t)1 << 31) || M * nchunk > INT32_MAX || smax < len / 4 + 2)
        return tetra_fail(ctx, TETRA_E_INVALID, "timing_chunks: nchunk >= 1, stride >= 1, len >= 16, every chunk "
                                                ">= 16 samples of the row, rows < 2^28 samples, smax >= len / 4 + 2");
    if (om && (stride % 4 || U < 4 || U > 64 || U % 4 || ngrp * (size_t)U < rowlen))
        return tetra_fail(ctx, TETRA_E_INVALID, "timing_chunks with om: stride a multiple of 4, 4 <= U <= 64 a "
                                                "multiple of 4, ngrp U >= rowlen");
    return launch_timing_chunks(ctx, P, y, M, rowlen, nchunk, stride, len, om, ngrp, U, soft, softbits, hard, nsym,
                                smax, diag);
}

int tetra_etsi_decide(tetra_ctx *ctx, const void *x, int fmt, size_t n, uint8_t *hard) {
    if (!ctx || (fmt != TETRA_CF32 && fmt != TETRA_CF64)) return TETRA_E_INVALID;
    if (n < 2) return TETRA_OK;
    Staging st(ctx);
    const void *xd = st.in(x, n * (fmt == TETRA_CF64 ? 16 : 8));
    uint8_t *h = (uint8_t *)st.out(hard, n - 1);
    if (!xd || !h) return st.finish();
    if (fmt == TETRA_CF32)
        hipLaunchKernelGGL(k_etsi_decide<float2>, dim3(grid_for(n - 1, 256)), dim3(256), 0, ctx->stream,
                           (const float2 *)xd, (long)n, h);
    else
        hipLaunchKernelGGL(k_etsi_decide<double2>, dim3(grid_for(n - 1, 256)), dim3(256), 0, ctx->stream,
                           (const double2 *)xd, (long)n, h);
    return st.finish();
}

}  // extern "C"
