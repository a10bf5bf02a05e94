// etsi_chanfilt.h -- what the two canonical-rate channel filters (etsi_chanfilt.hip: k_chanfilt,
// etsi_chanfilt_r.hip: k_chanfilt_r) and the host chain (etsi_demod.hip) share: the filter's geometry,
// the packed-fp32 helpers, the fused demod's timing tail (the timing stage of etsi_timing.h on y in
// LDS, after the filter's last tile) and the two kernel-pointer functions the host chain calls.
#pragma once
#include "etsi_timing.h"

namespace {

constexpr int TILE_K = 256;    // stage-1 outputs per tile (one per thread)
constexpr int TILE_IN = TILE_K * 10;   // new input samples per tile (q1 = 10)
constexpr int HALO = 48;
// k_chanfilt's stage 2 runs every S2_EVERY tiles (~205 output triples at 8).  Measured for cf32 (same box):
// serial demod every 12 tiles (LR 3336, 79.6 KB) 0.8 % faster than every 8 (1.569 vs 1.581 ms;
// 10 and 8 equal, 6 and 4 slower), but the pipelined step 0.7 % slower (1.694 vs 1.683 ms): at
// 2 x 79.6 KB the CU has no LDS left for the lower MAC's 7 KB workgroups, which then wait for a
// demod workgroup to retire.  The bench's pipelined step decides: 8 (16 KB free per CU).
constexpr int S2_EVERY = 8;
constexpr int TPP = 107;        // RRC taps per polyphase branch (Lp = 321 = 3 x 107)
constexpr int YLDS = 3968;      // cf32: stage-2 outputs held in LDS (a 131072-sample chunk has 3899; a
                                // streaming window of one, the previous chunk's last samples included, <= 3945)
// Stage 2 on the matrix cores (v_mfma_f32_16x16x4_f32: bit-for-bit a k-ordered fmaf chain).  One
// MFMA tile: 16 columns = 8 segments x (re, im), each segment S2Q consecutive triples; row
// i = 3q + c of a column is output 3(U + q) + c; A[i][s] = tap of x240[10U + s] for that output
// (zero outside its 107: leading zeros keep the accumulator +0, trailing ones add +-0), so every
// output is the oracle's ascending-j fma chain.
constexpr int S2Q = 5;          // triples per column (rows 0..14; row 15 all-zero taps)
constexpr int S2T = 8 * S2Q;    // triples per MFMA tile
constexpr int S2K = 39;         // k-steps of 4: window 10 (S2Q - 1) + 114 = 154 -> 156 stage-1 outputs
// k_chanfilt's linear stage-1 buffer (float2): S2_EVERY tiles of 256 outputs + the next triples' windows
constexpr int CF_LR = 2312;
constexpr int XIN4 = (HALO + TILE_IN) / 2;   // float4 entries of the input image
constexpr int CF_LDS4 = XIN4 + CF_LR / 2;    // image + stage-1 buffer (float4)
constexpr int CF_LDS2_SC16 = 2 * CF_LDS4;    // SC16 fused: y + timing scratch (float2)
static_assert(CF_LDS4 == 2460, "SC16 LDS: 39,360 B, four workgroups per CU");
static_assert((CF_LDS4 + 12) * 16 + 4096 * 8 <= 72 * 1024, "cf32 LDS: two workgroups per CU + 16 KB");
constexpr int CF_COEF = 128 + S2K * 64;      // device tap image: h1 (64), h1 * 2^-15 (64, SC16) + A fragments [S2K][64 lanes]

// Packed fp32 (v_pk_fma_f32): one real tap times a complex sample, each half a correctly rounded
// fma -- the same per-component arithmetic as two fmaf calls.
typedef float pf2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ pf2 pfma(float h, pf2 x, pf2 acc) { return __builtin_elementwise_fma(pf2{h, h}, x, acc); }
typedef float f4 __attribute__((ext_vector_type(4)));

// h1[48] stage-1 taps (wave-uniform, scalar loads); stage 2: branch c, output m = 3u + c =
// sum_j hp[i0(c) - 3j] * x240[10u + off_c + j] with i0 = {320, 318, 319}, off_c = {0, 4, 7}, held
// as the MFMA A fragments (one VGPR per k-step per lane, loaded once).
// Input pairs: one load = two complex samples -- float4 for cf32, uint2 (4 x int16) for SC16, the
// BladeRF wire format (capture.py:241-269 scales by 1/32768, exact in fp32), so an SC16 capture is
// filtered straight from its 4 B/sample form.
__device__ __forceinline__ float4 pair_f32(float4 v) { return v; }
__device__ __forceinline__ float4 pair_f32(uint2 v) {
    constexpr float s = 1.0f / 32768.0f;
    return make_float4((float)(int16_t)(v.x & 0xffffu) * s, (float)(int16_t)(v.x >> 16) * s,
                       (float)(int16_t)(v.y & 0xffffu) * s, (float)(int16_t)(v.y >> 16) * s);
}

// Timing outputs of the fused demod (FUSE = true: y never leaves LDS; wave 0 runs the timing
// stage on it after the last tile, with the input image as its scratch).
struct TimingOut {
    float gain, soft_scale;
    float2 *sym;
    int8_t *softbits;
    uint8_t *hard;
    int32_t *nsym;
    float4 *diag;
    int smax;
    int probe;   // TETRA_TIMING_PROBE: diag holds wall-clock stamps (start, tail start, tracking done, end)
    int ostride;                // row stride of sym / hard (softbits: 2x) -- 0: smax (streaming: reserve + smax)
    int yoff;                   // streaming: the window index of the first new 72 kHz output
    tetra_etsi_track *track;    // streaming: the channels' timing state (in/out), or null
};

constexpr int CPOL_SC1 = 16;   // gfx940+ cache-policy bits: sc0 1, nt 2, sc1 16 (copy_out)

// LDS -> global copy of n bytes by the workgroup's 256 threads, as device-scope (sc1) stores
// through a buffer resource over the row: 16-B stores where the row is 16-B aligned (the LDS image
// is), 8-B stores where it is 8-B aligned, byte stores for the rest.  sc1 writes the lines through
// to memory as they are stored; with the default policy the dirty lines sit in L2 and are evicted
// one by one into the channel filter's read stream (same box: demod 1.500 -> 1.423-1.437 ms; nt
// stores no better than the default; sc0 sc1 / nt sc1 / sc0 sc1 nt 1.43-1.45).
__device__ __forceinline__ void copy_out(uint8_t *g, const uint8_t *l, int n, int tid) {
    if (n <= 0) return;
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(g, 0, n, 0x00020000);   // n: the range check
    const uintptr_t al = reinterpret_cast<uintptr_t>(g);
    int done = 0;
    if ((al & 15) == 0) {
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
        const int n16 = n >> 4;
        for (int i = tid; i < n16; i += 256) {
            const uint4 v = reinterpret_cast<const uint4 *>(l)[i];
            __builtin_amdgcn_raw_buffer_store_b128(u4v{v.x, v.y, v.z, v.w}, r, 16 * i, 0, CPOL_SC1);
        }
        done = 16 * n16;
    } else if ((al & 7) == 0) {
        typedef unsigned u2v __attribute__((ext_vector_type(2)));
        const int n8 = n >> 3;
        for (int i = tid; i < n8; i += 256) {
            const uint2 v = reinterpret_cast<const uint2 *>(l)[i];
            __builtin_amdgcn_raw_buffer_store_b64(u2v{v.x, v.y}, r, 8 * i, 0, CPOL_SC1);
        }
        done = 8 * n8;
    }
    for (int i = done + tid; i < n; i += 256) __builtin_amdgcn_raw_buffer_store_b8(l[i], r, i, 0, CPOL_SC1);
}

// Output staging of the fused demod's tail (stage != nullptr): the symbols, soft bits and hard
// dibits of the channel collect in LDS and leave in wide stores once the channel is decided --
// per-block float2 stores from the tracking loop and byte stores from the decision pass cost
// 0.155 ms per 8192-channel batch (same box: 1.505 -> 1.350 ms with the stores left out).
struct TailStage {
    float2 *sym;     // [sm] (LDS)
    int8_t *sb;      // [2 sm]
    uint8_t *hard;   // [sm]
};

// The fused demod's timing stage for channel ch on y in LDS (ly), after the workgroup's last barrier:
// the tracking is the serial tail (wave 0, prioritised on its SIMD); the decision pass after it is
// shared by all four waves (the rotation and scale go through LDS, *tro).
__device__ __forceinline__ void timing_tail(const float2 *ly, float2 *scr, const TimingOut &to, int M2, int ch,
                                            int tid, TrackOut *tro, int *prog, const TailStage *stage, float *om,
                                            uint32_t t0) {
    const size_t so = (size_t)ch * (to.ostride ? to.ostride : to.smax);
    const bool probe = to.probe && to.diag;
    uint32_t t1 = 0, t2 = 0;
    if (probe && tid == 0) t1 = (uint32_t)wall_clock64();
    const TrackIn ti = track_in(to.track ? to.track + ch : nullptr, to.yoff);
    // the four Oerder-Meyr parts at once (not for a continued stream: no acquisition)
    if (om && M2 >= 16 && !ti.acq) om[tid] = om_part(ly, M2, tid >> 6, tid & 63);
    if (tid == 0) *prog = 0;
    __syncthreads();
    if (tid < 64) {
        __builtin_amdgcn_s_setprio(3);
        // S <= M2 / 4 + 1 < the staging size either way: the bound only guards the LDS buffer
        const TrackOut o = timing_track<true>(ly, M2, to.gain, to.soft_scale, stage ? stage->sym : to.sym + so, scr,
                                              stage ? min(to.smax, M2 / 4 + 3) : to.smax, tid, prog, om, nullptr,
                                              nullptr, float4{}, ti);
        if (tid == 0) {
            tro->S = o.S;
            tro->base = o.base;
            tro->delta = o.delta;
            to.nsym[ch] = o.S;
            if (to.track) track_store(to.track + ch, ti, o, M2);
            if (probe) t2 = (uint32_t)wall_clock64();
        }
    } else if (tid < 128) {
        cfo_consumer(scr, to.soft_scale, prog, tro, tid & 63, ti.acq ? 1 : 0);
    }
    __syncthreads();
    const TrackOut o = *tro;
    if (tid == 0 && to.diag && !probe)   // fewer than 16 samples: no timing ran, zeros (not what the buffer held)
        to.diag[ch] = M2 >= 16 ? make_float4(o.base, o.delta, o.rr, o.ri) : make_float4(0.f, 0.f, 0.f, 0.f);
    auto stamp = [&]() {
        if (probe && tid == 0) {
            __builtin_amdgcn_s_waitcnt(0);
            const uint32_t t3 = (uint32_t)wall_clock64();
            to.diag[ch] = make_float4(__uint_as_float(t0), __uint_as_float(t1), __uint_as_float(t2), __uint_as_float(t3));
        }
    };
    if (!stage) {
        timing_decide(o, scr, to.softbits + 2 * so, to.hard + so, tid >> 6, 4, tid & 63);
        stamp();
        return;
    }
    timing_decide(o, scr, stage->sb, stage->hard, tid >> 6, 4, tid & 63);
    __syncthreads();
    const int nd = o.S > 1 ? o.S - 1 : 0;
    copy_out(reinterpret_cast<uint8_t *>(to.sym + so), reinterpret_cast<const uint8_t *>(stage->sym), 8 * o.S, tid);
    copy_out(reinterpret_cast<uint8_t *>(to.softbits + 2 * so), reinterpret_cast<const uint8_t *>(stage->sb), 2 * nd,
             tid);
    copy_out(to.hard + so, stage->hard, nd, tid);
    stamp();
}
// The tail without staging, Oerder-Meyr scratch or start stamp (k_chanfilt).  The three absent arguments
// go through memory on purpose: as literal nulls a unit whose only tail is this one has them folded into
// timing_tail before it is inlined, and the kernel then compiles to other code than beside the staged
// tails of k_chanfilt_r (same results, different schedule); through a reference they are folded after
// inlining in every unit alike.  This rests on the compiler's pass order, not on the language.  Before
// simplifying it, or after a compiler update, build device assembly of etsi_chanfilt.hip before and after
// (the Makefile's flags plus --offload-device-only -S) and compare k_chanfilt<uint2, true>'s instruction
// text, labels renumbered, and its .amdhsa_ lines: they were identical to the unsplit etsi_demod.hip's.
struct TailNone {
    const TailStage *stage = nullptr;
    float *om = nullptr;
    uint32_t t0 = 0;
};
__device__ __forceinline__ void timing_tail(const float2 *ly, float2 *scr, const TimingOut &to, int M2, int ch,
                                            int tid, TrackOut *tro, int *prog, const TailNone &none = TailNone{}) {
    timing_tail(ly, scr, to, M2, ch, tid, tro, prog, none.stage, none.om, none.t0);
}

constexpr int WTAIL_SM = YLDS / 4 + 3;      // the fused tail's symbols per channel at most (+1: a continued
                                            // stream's carried symbol 0)

}  // namespace

// --------------------------------------------------------------------------- between the units
// The kernel for a sample format (TETRA_CF32 / TETRA_SC16) and the fused flag: k_chanfilt
// (etsi_chanfilt.hip; cf32 has no fused form there: nullptr) and k_chanfilt_r (etsi_chanfilt_r.hip).
const void *chanfilt_fn(int fmt, bool fused);
const void *chanfilt_r_fn(int fmt, bool fused);
